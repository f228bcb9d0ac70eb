"""GPU tests of the BOP pose errors (libpvbop.so: pv_bop_sym_errors, pv_bop_vsd) and their Python
layer, bit for bit against the numpy restatement tests/bop_ref.py (uint64 views: no tolerance).

Sizes: k_sym_partial gives a block of 256 threads a chunk of C = 1024 vertices (V = 4 per lane) and
walks the symmetries in LDS tiles of T = 32; k_sym_finish gives a pose one wave of 64 lanes, lane l
taking symmetries l, l + 64, ...; k_vsd gives a block of 256 threads P = 1024 pixels (4 per lane).
The shapes below sit on and around each of these."""
import copy

import numpy as np
import pytest
import torch

from tests import bop_ref as R
from tests import render_ref as RR

pytestmark = pytest.mark.gpu

C, V, T, P = 1024, 4, 32, 1024
PNS = (1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1)
NSS = (1, 2, T - 1, T, T + 1, 315)
B = 3
K_SKEW = np.array([[572.4, 0.7, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])
IDENT = np.eye(4)[None, :3]


@pytest.fixture(scope="module")
def bop(device):
    from pvnet_amd import build, bop
    build.build()
    return bop


def cu(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def random_syms(rng, ns):
    """The identity, then ns - 1 rigid transformations."""
    out = [IDENT[0]]
    for _ in range(ns - 1):
        out.append(RR.pose(RR.random_rotation(rng), rng.normal(size=3) * 0.01))
    return np.stack(out)


def compose(Pg, S):
    return RR.pose(Pg[:, :3] @ S[:, :3], Pg[:, :3] @ S[:, 3] + Pg[:, 3])


def small_turn(rng, scale=0.02):
    w = rng.normal(size=3) * scale
    return R.axis_rotation(w, float(np.linalg.norm(w))) if scale > 0 else np.eye(3)


def poses_for(rng, S, b):
    """Ground truths in front of the camera, and estimates near the ground truth after one of its symmetries."""
    Pg = np.stack([RR.pose(RR.random_rotation(rng), [rng.normal() * 0.05, rng.normal() * 0.05, 0.6 + 0.4 * rng.random()])
                   for _ in range(b)])
    Pe = []
    for i in range(b):
        g = compose(Pg[i], S[int(rng.integers(len(S)))])
        Pe.append(RR.pose(small_turn(rng) @ g[:, :3], g[:, 3] + rng.normal(size=3) * 0.003))
    return np.stack(Pe), Pg


def tables(bop, device, models, syms):
    from pvnet_amd.evaluation_utils import ModelTable
    return (ModelTable([(m, 0.1, False) for m in models], device=device), bop.SymmetryTable.from_arrays(syms, device=device))


def run_sym(bop, device, models, syms, Pe, Pg, K, model_id=None, metrics=("mssd", "mspd"), tabs=None, out=None):
    mt, st = tabs or tables(bop, device, models, syms)
    r = bop.sym_errors(cu(Pe, device), cu(Pg, device), mt, st, cu(K, device), None if model_id is None else cu(
        np.asarray(model_id, np.int32), device), metrics, out=out)
    return {k: v.cpu().numpy() for k, v in r.items()}


def assert_sym_equal(got, models, syms, Pe, Pg, K, model_id=None, what="", **kw):
    err, best = R.sym_errors(models, syms, Pe, Pg, K, model_id, **kw)
    for c, m in enumerate(("mssd", "mspd")):
        if m in got:
            assert got[m].dtype == np.float64 and got["best_" + m].dtype == np.int32
            np.testing.assert_array_equal(bits(got[m]), bits(err[:, c]), err_msg=f"{what} {m}: {got[m]} != {err[:, c]}")
            np.testing.assert_array_equal(got["best_" + m], best[:, c], err_msg=f"{what} best_{m}")
    return err, best


# ----------------------------------------------------------------------------
# pv_bop_sym_errors
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("ns", NSS)
def test_sym_errors_bit_equal(device, bop, ns):
    rng = np.random.default_rng(100 + ns)
    S = random_syms(rng, ns)
    cases = []
    for pn in PNS:
        Pm = (rng.normal(size=(pn, 3)) * 0.05).astype(np.float32)
        Pe, Pg = poses_for(rng, S, B)
        cases.append((Pm, Pe, Pg, run_sym(bop, device, [Pm], [S], Pe, Pg, K_SKEW)))
    for Pm, Pe, Pg, got in cases:
        err, best = assert_sym_equal(got, [Pm], [S], Pe, Pg, K_SKEW, what=f"pn={len(Pm)} ns={ns}")
        assert np.isfinite(err).all() and (err > 0).all() and (best >= 0).all() and (best < ns).all()


def test_sym_errors_table_of_three_models_and_per_pose_camera(device, bop):
    rng = np.random.default_rng(7)
    models = [(rng.normal(size=(pn, 3)) * 0.05).astype(np.float32) for pn in (65, C + 1, 300)]
    syms = [random_syms(rng, ns) for ns in (1, T + 1, 315)]
    mid = np.array([2, 0, 1, 1, 2, 0, 2], np.int32)
    Pe, Pg = (np.stack(x) for x in zip(*[[a[0] for a in poses_for(rng, syms[m], 1)] for m in mid]))
    Ks = np.stack([K_SKEW + np.array([[3.0 * i, 0.1 * i, -2.0 * i], [0, 2.0 * i, 1.5 * i], [0, 0, 0]]) for i in range(len(mid))])
    tabs = tables(bop, device, models, syms)
    got = run_sym(bop, device, models, syms, Pe, Pg, Ks, mid, tabs=tabs)
    err, best = assert_sym_equal(got, models, syms, Pe, Pg, Ks, mid, what="per-pose K")
    assert np.isfinite(err).all() and len({tuple(e) for e in err}) == len(mid)
    got = run_sym(bop, device, models, syms, Pe, Pg, K_SKEW, mid, tabs=tabs)
    assert_sym_equal(got, models, syms, Pe, Pg, K_SKEW, mid, what="shared K")
    # the skew is honoured: without it MSPD differs
    K0 = K_SKEW.copy()
    K0[0, 1] = 0.0
    assert (run_sym(bop, device, models, syms, Pe, Pg, K0, mid, tabs=tabs)["mspd"] != got["mspd"]).any()
    # Evaluator.bop_errors is the same call
    from pvnet_amd.evaluation_utils import Evaluator
    ev = Evaluator(tabs[0], np.zeros((3, 9, 3)))
    r = ev.bop_errors(cu(Pe, device), cu(Pg, device), tabs[1], cu(K_SKEW, device), cu(mid, device))
    np.testing.assert_array_equal(bits(r["mssd"].cpu().numpy()), bits(got["mssd"]))
    assert not ev.add_recorder


def test_sym_errors_ties_zero_and_behind_the_camera(device, bop):
    rng = np.random.default_rng(11)
    Pm = (rng.normal(size=(C + 7, 3)) * 0.05).astype(np.float32)
    S = random_syms(rng, 70)
    # rows 3, 40 and 69 are one transformation: lanes 3, 40 and 5 of the finishing wave, two tiles apart
    S[40] = S[3]
    S[69] = S[3]
    Pg = np.stack([RR.pose(RR.random_rotation(rng), [0.01, 0.02, 0.8]) for _ in range(B)])
    near = compose(Pg[0], S[3])
    Pe = np.stack([RR.pose(small_turn(rng, 1e-3) @ near[:, :3], near[:, 3]),      # nearest to the duplicated row
                   compose(Pg[1], S[0]),                                            # the ground truth itself
                   RR.pose(Pg[2][:, :3], [0.01, 0.02, 0.03])])                      # inside the cloud: vertices behind
    got = run_sym(bop, device, [Pm], [S], Pe, Pg, K_SKEW)
    err, best = assert_sym_equal(got, [Pm], [S], Pe, Pg, K_SKEW, what="ties")
    assert got["best_mssd"][0] == got["best_mspd"][0] == 3                          # the lowest of 3, 40, 69
    assert bits(got["mssd"])[1] == 0 and bits(got["mspd"])[1] == 0                  # exactly +0.0
    assert got["best_mssd"][1] == got["best_mspd"][1] == 0
    assert got["mspd"][2] == np.inf and got["best_mspd"][2] == 0 and np.isfinite(got["mssd"][2])
    # every symmetry the same: the first wins both columns
    S1 = np.repeat(S[5:6], 2 * T + 1, 0)
    got = run_sym(bop, device, [Pm], [S1], Pe[:1], Pg[:1], K_SKEW)
    assert_sym_equal(got, [Pm], [S1], Pe[:1], Pg[:1], K_SKEW, what="all equal")
    assert got["best_mssd"][0] == got["best_mspd"][0] == 0


def test_sym_errors_nan_rules(device, bop):
    rng = np.random.default_rng(13)
    models = [(rng.normal(size=(pn, 3)) * 0.05).astype(np.float32) for pn in (70, 40, 9)]
    syms = [random_syms(rng, ns) for ns in (3, T + 2, 1)]
    syms[1][T + 1, 1, 2] = np.nan                                   # the last symmetry of model 1, in its second tile
    mid = np.array([0, 0, 0, 1, 2, -1, 3, 0, 2], np.int32)
    Pe, Pg = poses_for(rng, IDENT, len(mid))
    Pe[1, 2, 3] = np.inf
    Pg[2, 0, 0] = np.nan
    tabs = tables(bop, device, models, syms)
    got = run_sym(bop, device, models, syms, Pe, Pg, K_SKEW, mid, tabs=tabs)
    assert_sym_equal(got, models, syms, Pe, Pg, K_SKEW, mid, what="nan rules")
    nan = np.isnan(got["mssd"])
    assert nan.tolist() == [False, True, True, True, False, True, True, False, False]
    assert (np.isnan(got["mspd"]) == nan).all()
    assert ((got["best_mssd"] == -1) == nan).all() and ((got["best_mspd"] == -1) == nan).all()
    # a camera that is not finite: MSPD alone, and only for the poses that read it
    Ks = np.repeat(K_SKEW[None], len(mid), 0)
    for i, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2))):
        Kb = Ks.copy()
        Kb[0, r, c] = np.inf if i % 2 else np.nan
        g2 = run_sym(bop, device, models, syms, Pe, Pg, Kb, mid, tabs=tabs)
        assert_sym_equal(g2, models, syms, Pe, Pg, Kb, mid, what=f"K[{r},{c}]")
        assert np.isnan(g2["mspd"][0]) and g2["best_mspd"][0] == -1 and g2["mssd"][0] == got["mssd"][0]
        np.testing.assert_array_equal(bits(g2["mspd"][1:]), bits(got["mspd"][1:]))
    Kb = Ks.copy()
    Kb[:, 1, 0] = Kb[:, 2, 1] = np.nan                              # entries that are not read
    np.testing.assert_array_equal(bits(run_sym(bop, device, models, syms, Pe, Pg, Kb, mid, tabs=tabs)["mspd"]), bits(got["mspd"]))
    # ranges the host does not vouch for: a model larger than max_pn, a symmetry set larger than
    # max_ns, rows beyond total / total_s
    for attr, which, value, lost in (("max_pn", 0, 69, [0, 7]), ("max_ns", 1, 2, [0, 7]), ("total", 0, 110, [4, 8]),
                                     ("total", 1, 3 + T + 2, [4, 8])):                  # the symmetry table's total is the batch's total_s
        t2 = [copy.copy(t) for t in tabs]
        setattr(t2[which], attr, value)
        g2 = run_sym(bop, device, models, syms, Pe, Pg, K_SKEW, mid, tabs=t2)
        for i in range(len(mid)):
            if i in lost:
                assert np.isnan(g2["mssd"][i]) and np.isnan(g2["mspd"][i]), (attr, which, i)
                assert g2["best_mssd"][i] == g2["best_mspd"][i] == -1
            else:
                assert bits(g2["mssd"])[i] == bits(got["mssd"])[i] and bits(g2["mspd"])[i] == bits(got["mspd"])[i], (attr, which, i)
    # an empty model and an empty symmetry set
    models2 = [models[0], np.zeros((0, 3), np.float32), models[2]]
    syms2 = [syms[0], syms[1][:1], np.zeros((0, 3, 4))]
    g2 = run_sym(bop, device, models2, syms2, Pe, Pg, K_SKEW, mid)
    assert np.isnan(g2["mssd"])[[3, 4, 8]].all() and (g2["best_mspd"][[3, 4, 8]] == -1).all()
    assert bits(g2["mssd"])[0] == bits(got["mssd"])[0] and bits(g2["mspd"])[7] == bits(got["mspd"])[7]


def test_sym_errors_overflow_is_infinite(device, bop):
    rng = np.random.default_rng(17)
    Pm = (rng.normal(size=(66, 3)) * 0.05).astype(np.float32)
    Pe, Pg = poses_for(rng, IDENT, 3)
    Pe[0, 0, 3] = 2.0 ** 300                                        # c_s on the bound: +inf
    Pe[1, 0, 3] = np.nextafter(2.0 ** 300, 0.0)                     # below it: finite
    Pe[2, 1, 1] = -1e200
    got = run_sym(bop, device, [Pm], [IDENT], Pe, Pg, K_SKEW)
    assert_sym_equal(got, [Pm], [IDENT], Pe, Pg, K_SKEW, what="overflow")
    assert got["mssd"][0] == np.inf and np.isfinite(got["mssd"][1]) and got["mssd"][2] == np.inf
    assert got["best_mssd"].tolist() == [0, 0, 0]


def test_sym_errors_one_metric_leaves_the_other_column(device, bop):
    rng = np.random.default_rng(19)
    Pm = (rng.normal(size=(C + 3, 3)) * 0.05).astype(np.float32)
    S = random_syms(rng, T + 3)
    Pe, Pg = poses_for(rng, S, B)
    tabs = tables(bop, device, [Pm], [S])
    full = run_sym(bop, device, [Pm], [S], Pe, Pg, K_SKEW, tabs=tabs)
    for m, c in (("mssd", 0), ("mspd", 1)):
        out = {"err": torch.full((B, 2), -7.0, dtype=torch.float64, device=device),
               "best": torch.full((B, 2), -7, dtype=torch.int32, device=device)}
        got = run_sym(bop, device, [Pm], [S], Pe, Pg, K_SKEW, metrics=(m,), tabs=tabs, out=out)
        assert set(got) == {m, "best_" + m}
        np.testing.assert_array_equal(bits(got[m]), bits(full[m]))
        np.testing.assert_array_equal(got["best_" + m], full["best_" + m])
        assert (out["err"][:, 1 - c] == -7.0).all() and (out["best"][:, 1 - c] == -7).all()
    # MSSD alone reads no camera
    got = run_sym(bop, device, [Pm], [S], Pe, Pg, np.full((3, 3), np.nan), metrics=("mssd",), tabs=tabs)
    np.testing.assert_array_equal(bits(got["mssd"]), bits(full["mssd"]))
    assert bop.sym_errors(cu(Pe[:0], device), cu(Pg[:0], device), *tabs, cu(K_SKEW, device))["mssd"].shape == (0,)


# ----------------------------------------------------------------------------
# pv_bop_vsd
# ----------------------------------------------------------------------------
def camera(H, W):
    """A camera that puts the objects, 0.5 away and 0.1 across, over most of an H x W image."""
    return np.array([[2.6 * W, 0.0, (W - 1) / 2 + 0.13], [0.0, 2.4 * H, (H - 1) / 2 - 0.21], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def meshes(device, bop):
    from pvnet_amd.render import MeshTable
    models = [RR.bumpy_ellipsoid(level=1), RR.icosphere(1, 0.045)]      # 80 faces each: two small meshes that overlap
    return models, MeshTable(models, device=device)


def rendered(device, meshes, poses, mid, K, H, W):
    from pvnet_amd.render import render_labels
    return render_labels(meshes[1], cu(poses, device)[:, None], cu(np.asarray(mid, np.int32), device)[:, None], None,
                         cu(K, device), H, W, want=("depth",))["depth"]


def vsd_scene(device, meshes, H, W, seed):
    """b = 3 poses of two overlapping meshes, their rendered maps, and two sensor maps with holes and an occluder."""
    rng = np.random.default_rng(seed)
    K = camera(H, W)
    mid = [0, 1, 0]
    Pg = np.stack([RR.pose(RR.random_rotation(rng), [0.01 * rng.normal(), 0.01 * rng.normal(), 0.5]) for _ in mid])
    Pe = np.stack([RR.pose(small_turn(rng, 0.2) @ p[:, :3], p[:, 3] + rng.normal(size=3) * [0.01, 0.01, 0.004]) for p in Pg])
    de, dg = (rendered(device, meshes, p, mid, K, H, W) for p in (Pe, Pg))
    g = dg.cpu().numpy()
    sensor = np.empty((2, H, W), np.float32)
    for j in range(2):
        s = np.where(np.isfinite(g[j]), g[j] + rng.normal(size=(H, W)).astype(np.float32) * 0.002, np.float32(0.9))
        s[rng.random((H, W)) < 0.15] = 0.0                              # holes
        s[:, : W // 3] = 0.3                                            # an occluder in front of the left third
        if H > 2:
            s[0, -1], s[1, -1], s[2, -1] = np.nan, -1.0, np.inf         # the other ways to be missing
        sensor[j] = s
    return K, Pe, Pg, de, dg, sensor


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (37, 67), (31, 33), (32, 32), (25, 41)])
@pytest.mark.parametrize("ntau", [1, 10])
def test_vsd_bit_equal(device, bop, meshes, hw, ntau):
    H, W = hw
    assert (31 * 33, 32 * 32, 25 * 41) == (P - 1, P, P + 1)
    K, Pe, Pg, de, dg, sensor = vsd_scene(device, meshes, H, W, 1000 * H + W)
    img_id = np.array([1, 1, 2 if ntau == 1 else -1], np.int32)       # image 1 twice, and one outside [0, 2)
    delta = 0.015
    e, g = de.cpu().numpy(), dg.cpu().numpy()
    # taus placed exactly on attained |dg - de| values of pose 0, the rest generic
    probe = R.vsd(sensor, e, g, K, delta, np.zeros((B, 1)), img_id)[0]
    ax, ay = (np.arange(W)[None, :] - K[0, 2]) / K[0, 0], (np.arange(H)[:, None] - K[1, 2]) / K[1, 1]
    r = np.sqrt((ax * ax + ay * ay) + 1.0)
    both = np.isfinite(e[0]) & np.isfinite(g[0])
    with np.errstate(invalid="ignore"):
        attained = np.unique(np.abs(g[0].astype(np.float64) * r - e[0].astype(np.float64) * r)[both])
    taus = np.sort(np.random.default_rng(5).random((B, ntau)) * 0.02, 1)
    if len(attained):
        taus[0, : min(ntau, len(attained))] = attained[np.linspace(0, len(attained) - 1, min(ntau, len(attained))).astype(int)]
    if ntau == 10:
        taus[1, 3] = np.nan                                             # counts nothing
    got = bop.vsd_maps(cu(sensor, device), de, dg, cu(K, device), cu(taus, device), delta, cu(img_id, device))
    counts, err = R.vsd(sensor, e, g, K, delta, taus, img_id)
    gc, ge = got["counts"].cpu().numpy(), got["err"].cpu().numpy()
    assert gc.dtype == np.int64 and gc.shape == (B, 2 + ntau) and ge.dtype == np.float64 and ge.shape == (B, ntau)
    np.testing.assert_array_equal(gc, counts)
    np.testing.assert_array_equal(bits(ge), bits(err))
    assert (gc[2] == -1).all() and np.isnan(ge[2]).all()
    if H * W > 100:
        assert 0 < counts[0, 1] <= counts[0, 0] and counts[0, 2] == counts[0, 1]        # a tau on the smallest attained value
        assert probe[0, 0] == counts[0, 0] and len(attained) > ntau
        if ntau == 10:
            assert counts[1, 2 + 3] == 0 and len(set(counts[0, 2:])) > 3


def test_vsd_cameras_and_default_images(device, bop, meshes):
    H, W = 37, 67
    K, Pe, Pg, de, dg, sensor = vsd_scene(device, meshes, H, W, 3)
    sensor = np.concatenate([sensor, sensor[:1]])
    e, g = de.cpu().numpy(), dg.cpu().numpy()
    taus = np.full((B, 2), 0.004) * [1.0, 3.0]
    Ks = np.stack([K, K * [[1.1, 1, 1], [1, 0.9, 1], [1, 1, 1]], K])
    Ks[0, 0, 1] = np.nan                                                # the skew is not read
    Ks[2, 1, 2] = np.inf                                                # cy is
    got = bop.vsd_maps(cu(sensor, device), de, dg, cu(Ks, device), cu(taus, device), 0.015)      # img_id None: image i
    counts, err = R.vsd(sensor, e, g, Ks, 0.015, taus)
    np.testing.assert_array_equal(got["counts"].cpu().numpy(), counts)
    np.testing.assert_array_equal(bits(got["err"].cpu().numpy()), bits(err))
    assert (counts[2] == -1).all() and counts[0, 0] > 0 and counts[1, 0] > 0
    # identical maps: zero at every tau; nothing rendered: exactly 1
    same = bop.vsd_maps(cu(sensor, device), dg, dg, cu(K, device), cu(taus, device), 0.015)
    assert (same["err"] == 0).all() and (same["counts"][:, 0] == same["counts"][:, 1]).all() and (same["counts"][:, 2:] == 0).all()
    empty = torch.full_like(dg, float("inf"))
    none = bop.vsd_maps(cu(sensor, device), empty, empty, cu(K, device), cu(taus, device), 0.015)
    assert (none["err"] == 1.0).all() and (none["counts"] == 0).all()


def test_vsd_and_average_recall_end_to_end(device, bop, meshes):
    """vsd() and average_recall() on 8 poses at 48 x 64 against render_ref and bop_ref composed the
    same way.  The device's depth may differ from render_ref's by one f32 ulp (tests/test_gpu_render.py),
    which moves a count only if a pixel sits within that ulp of delta or of a tau: the taus are
    generic fractions of the diameter, so the counts are compared exactly."""
    from pvnet_amd.evaluation_utils import ModelTable
    H, W, b = 48, 64, 8
    rng = np.random.default_rng(23)
    models, mesh_table = meshes
    K = camera(H, W)
    mid = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.int32)
    Pg = np.stack([RR.pose(RR.random_rotation(rng), [0.01 * rng.normal(), 0.01 * rng.normal(), 0.5]) for _ in mid])
    scale = np.array([0.0, 0.01, 0.03, 0.08, 0.15, 0.3, 0.6, 1.0])       # from exact to plainly wrong
    Pe = np.stack([RR.pose(small_turn(rng, s) @ p[:, :3], p[:, 3] + rng.normal(size=3) * 0.02 * s) for p, s in zip(Pg, scale)])
    ref_e = np.stack([RR.render(models, [(m, 1, p)], K, H, W)["depth"] for m, p in zip(mid, Pe)])
    ref_g = np.stack([RR.render(models, [(m, 1, p)], K, H, W)["depth"] for m, p in zip(mid, Pg)])
    sensor = np.where(np.isfinite(ref_g), ref_g + np.float32(0.001), np.float32(0.9)).astype(np.float32)
    sensor[:, ::5, ::7] = 0.0
    table = ModelTable.from_meshes(mesh_table)
    dia = table.diameter.cpu().numpy()
    syms = bop.SymmetryTable.identity(2, device=device)
    got = bop.vsd(cu(sensor, device), cu(Pe, device), cu(Pg, device), mesh_table, cu(K, device), cu(mid, device), table.diameter,
                  delta=0.015, max_frames=3)                              # chunks of 3, 3 and 2
    taus = dia[mid][:, None] * np.asarray(bop.FRACTIONS)[None, :]
    counts, err = R.vsd(sensor, ref_e, ref_g, K, 0.015, taus)
    np.testing.assert_array_equal(got["counts"].cpu().numpy(), counts)
    np.testing.assert_array_equal(bits(got["err"].cpu().numpy()), bits(err))
    assert err[0].max() == 0.0 and err[-1].max() > 0.0
    se = bop.sym_errors(cu(Pe, device), cu(Pg, device), table, syms, cu(K, device), cu(mid, device))
    rerr, _ = R.sym_errors([m[0] for m in models], [IDENT, IDENT], Pe, Pg, K, mid)
    np.testing.assert_array_equal(bits(se["mssd"].cpu().numpy()), bits(rerr[:, 0]))
    np.testing.assert_array_equal(bits(se["mspd"].cpu().numpy()), bits(rerr[:, 1]))
    ar = bop.average_recall(se["mssd"], se["mspd"], got["err"], table.diameter[cu(mid, device).long()], W)
    fr = np.asarray(bop.FRACTIONS)
    want = {"ar_vsd": float(np.mean(err[:, :, None] < fr[None, None, :])),
            "ar_mssd": float(np.mean(rerr[:, 0, None] < dia[mid][:, None] * fr[None, :])),
            "ar_mspd": float(np.mean(rerr[:, 1, None] < (np.asarray(bop.MSPD_PIXELS) * (W / 640.0))[None, :]))}
    want["ar"] = (want["ar_vsd"] + want["ar_mssd"] + want["ar_mspd"]) / 3.0
    assert ar == want and 0.1 < ar["ar"] < 0.9 and ar["ar_mssd"] >= 1 / 8


def test_both_entries_in_one_graph(device, bop, meshes):
    rng = np.random.default_rng(29)
    H, W = 37, 67
    K, Pe, Pg, de, dg, sensor = vsd_scene(device, meshes, H, W, 31)
    Pm = (rng.normal(size=(C + 1, 3)) * 0.05).astype(np.float32)
    S = random_syms(rng, T + 1)
    Qe, Qg = poses_for(rng, S, B)
    tabs = tables(bop, device, [Pm], [S])
    taus = cu(np.full((B, 3), 0.004) * [1.0, 2.0, 3.0], device)
    args = (cu(Qe, device), cu(Qg, device), *tabs, cu(K_SKEW, device))
    vargs = (cu(sensor, device), de, dg, cu(K, device), taus, 0.015, cu(np.array([0, 1, 0], np.int32), device))
    eager = bop.sym_errors(*args)                                         # also warms the workspace up
    eager_v = bop.vsd_maps(*vargs)
    want = [eager["mssd"].clone(), eager["mspd"].clone(), eager["best_mssd"].clone(), eager_v["err"].clone(), eager_v["counts"].clone()]
    out = {"err": torch.zeros((B, 2), dtype=torch.float64, device=device), "best": torch.zeros((B, 2), dtype=torch.int32, device=device)}
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = bop.sym_errors(*args, out=out)
        v = bop.vsd_maps(*vargs)
    for _ in range(2):
        out["err"].fill_(-1.0)
        out["best"].fill_(-9)
        v["err"].fill_(-1.0)
        v["counts"].fill_(-9)
        graph.replay()
        torch.cuda.synchronize(device)
        got = [r["mssd"], r["mspd"], r["best_mssd"], v["err"], v["counts"]]
        for a, w in zip(got, want):
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, w.view(torch.int64) if w.dtype == torch.float64 else w)
