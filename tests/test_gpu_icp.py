"""GPU tests of the depth refinement (libpvicp.so: pv_icp_iterate) and its Python layer, bit for bit
against the numpy restatement tests/icp_ref.py on pose, status, iters, cnt, stats and neq (uint64
views: no tolerance anywhere).

The cases are tests/icp_cases.py's; tests/test_icp_ref.py shows on the CPU that they reach what their
names say.  Sizes: k_linearise gives a block of 256 lanes 1024 consecutive pixels, a lane a run of 4;
25 x 41 is one pixel more than a block with a width that is no multiple of 4, 17 x 64 one row more."""
import numpy as np
import pytest
import torch

from tests import icp_cases as C
from tests import icp_ref as R

pytestmark = pytest.mark.gpu

CASES = C.call_cases()
KEYS = ("pose", "status", "iters", "cnt", "stats", "neq")


@pytest.fixture(scope="module")
def icp(device):
    from pvnet_amd import build, icp
    build.build()
    return icp


@pytest.fixture(scope="module")
def refs():
    """The reference's final state of every call case, computed once."""
    return {name: C.run_ref(c) for name, c in CASES.items()}


def cu(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, keys=KEYS, what=""):
    for k in keys:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        np.testing.assert_array_equal(bits(g), bits(want[k]), err_msg=f"{what}: {k}")


def run_device(icp, device, c, neq=True):
    st = icp.new_state(cu(c["poses"], device), neq=neq)
    dt, K = cu(c["depth_test"], device), cu(c["K"], device)
    iid = None if c["img_id"] is None else cu(c["img_id"], device)
    for k in range(c["calls"]):
        de = c["second"] if (k > 0 and c["second"] is not None) else c["depth_est"]
        icp.iterate(st, cu(de, device), dt, K, iid, **c["params"])
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("name", list(CASES))
def test_call_case_equals_reference(device, icp, refs, name):
    got = run_device(icp, device, CASES[name])
    same(got, refs[name], what=name)


def test_neq_null_and_two_runs_bit_identical(device, icp, refs):
    for name in ("three_blocks", "mixed_batch"):
        a = run_device(icp, device, CASES[name], neq=False)
        assert "neq" not in a
        same(a, refs[name], keys=KEYS[:5], what=name)
        b = run_device(icp, device, CASES[name])
        c = run_device(icp, device, CASES[name])
        same(b, {k: c[k].cpu().numpy() for k in KEYS}, what=name + " twice")


def test_empty_batch(device, icp):
    st = icp.new_state(torch.zeros((0, 3, 4), dtype=torch.float64, device=device), neq=True)
    icp.iterate(st, torch.zeros((0, 5, 7), device=device), torch.zeros((1, 5, 7), device=device), cu(C.K_SKEW, device))
    torch.cuda.synchronize()
    assert st["pose"].shape == (0, 3, 4) and st["neq"].shape == (0, 28)


def test_four_calls_in_one_graph(device, icp):
    """Four pv_icp_iterate calls captured on one stream; two replays from the same start equal four plain calls."""
    c = CASES["mixed_batch"]
    want = R.new_state(c["poses"])
    for _ in range(4):
        R.iterate(want, c["depth_est"], c["depth_test"], c["K"], c["img_id"], **c["params"])
    assert want["iters"].max() == 4 and (want["status"] == R.BAD_INPUT).sum() == 5
    de, dt, K, iid = (cu(c[k], device) for k in ("depth_est", "depth_test", "K", "img_id"))
    start = icp.new_state(cu(c["poses"], device), neq=True)
    plain = {k: v.clone() for k, v in start.items()}
    for _ in range(4):
        icp.iterate(plain, de, dt, K, iid, **c["params"])
    torch.cuda.synchronize()
    same(plain, want, what="four plain calls")
    st = {k: v.clone() for k, v in start.items()}
    gph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gph, stream=side):
            for _ in range(4):
                icp.iterate(st, de, dt, K, iid, **c["params"])
    for _ in range(2):
        for k in st:
            st[k].copy_(start[k])
        gph.replay()
        torch.cuda.synchronize()
        same(st, want, what="replay")


# ---------------------------------------------------------------- through the renderer
def scene_tables(device, models):
    from pvnet_amd.render import MeshTable
    return MeshTable(models, device=device)


def test_refine_depth_equals_reference_chain(device, icp):
    """96 x 128, two objects in one batch, four rounds.  Every round's device render is first held to
    tests/render_ref.py on every pixel; only then can the poses agree bit for bit."""
    from pvnet_amd.render import render_labels
    H, W, iters = 96, 128, 4
    K = C.K_PLAIN * np.array([[2.0], [2.0], [1.0]])
    scenes = [C.convergence_scene(w) for w in (0, 1)]                   # for the poses; the sensor map is rendered at this size
    models = scenes[0]["models"]
    gt = np.stack([s["gt"] for s in scenes])
    start = np.stack([s["start"] for s in scenes])
    mid = np.array([0, 1], np.int32)
    depth = R.render_depth(models, mid, gt, K, H, W)
    depth = np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)
    kw = dict(eps_rot=1e-9, eps_trans=1e-9)                              # keep both running for all four rounds
    table = scene_tables(device, models)
    want = R.new_state(start)
    got = icp.new_state(cu(start, device), neq=True)
    Kd, dd, midd = cu(K, device), cu(depth, device), cu(mid, device)
    for it in range(iters):
        ref_map = R.render_depth(models, mid, want["pose"], K, H, W)
        dev_map = render_labels(table, got["pose"][:, None], midd[:, None], None, Kd, H, W, want=("depth",))["depth"]
        np.testing.assert_array_equal(dev_map.cpu().numpy().view(np.uint32), ref_map.view(np.uint32), err_msg=f"render {it}")
        assert np.isfinite(ref_map).sum() > 4000
        R.iterate(want, ref_map, depth, K, **{**icp.DEFAULTS, **kw})
        icp.iterate(got, dev_map, dd, Kd, None, **kw)
        torch.cuda.synchronize()
        same(got, want, what=f"round {it}")
    assert (want["iters"] == iters).all() and (want["status"] == R.RUNNING).all()
    poses, info = icp.refine_depth(table, cu(start, device), midd, dd, Kd, iters=iters, **kw)
    torch.cuda.synchronize()
    same(dict(pose=poses, status=info["status"], iters=info["iters"], cnt=info["cnt"],
              stats=torch.cat([info["rms"][:, None], info["step"]], 1)), want, keys=KEYS[:5], what="refine_depth")
    # chunked: one pose per chunk gives the same bits
    poses1, info1 = icp.refine_depth(table, cu(start, device), midd, dd, Kd, iters=iters, max_frames=1, **kw)
    np.testing.assert_array_equal(bits(poses1.cpu().numpy()), bits(want["pose"]))
    lin = icp.linearise(table, cu(start, device), midd, dd, Kd, **kw)
    one = R.new_state(start)
    R.iterate(one, R.render_depth(models, mid, start, K, H, W), depth, K, **{**icp.DEFAULTS, **kw})
    same(lin, one, keys=("neq", "cnt", "status", "stats", "pose"), what="linearise")


@pytest.mark.parametrize("kind", ["clean", "occluder", "missing"])
def test_convergence_through_the_evaluator(device, icp, kind):
    """tests/test_icp_ref.py's convergence case on the box, through Evaluator.refine_depth: ADD falls below
    a tenth of its start in 10 rounds, and the result is the reference chain's."""
    from pvnet_amd.evaluation_utils import Evaluator, ModelTable
    s = C.convergence_scene(1, occluder=kind == "occluder", missing=0.3 if kind == "missing" else 0.0)
    verts = np.asarray(s["models"][1][0], np.float64)
    ev = Evaluator(ModelTable([(verts, 0.14, False)], device=device), np.zeros((1, 9, 3)))
    table = scene_tables(device, s["models"])
    poses, info = ev.refine_depth(cu(s["start"][None], device), cu(s["model_id"], device), cu(s["depth"], device),
                                  cu(s["K"], device), table, iters=10)
    torch.cuda.synchronize()
    got = poses.cpu().numpy()[0]
    ratio = C.add_metric(verts, got, s["gt"]) / C.add_metric(verts, s["start"], s["gt"])
    print(f"box {kind}: ADD ratio {ratio:.2e}, status {int(info['status'][0])}, iters {int(info['iters'][0])}")
    assert ratio < 0.1
    want = R.refine(s["models"], [s["start"]], s["model_id"], s["depth"], s["K"], iters=10, **icp.DEFAULTS)
    np.testing.assert_array_equal(bits(got), bits(want["pose"][0]))
    assert int(info["status"][0]) == want["status"][0] and int(info["iters"][0]) == want["iters"][0]
    assert int(info["cnt"][0]) == want["cnt"][0]
