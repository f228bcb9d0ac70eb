"""pv_epnp / pv_rt6_to_Rt (include/pvpose.h) and their Python layers on the device against the
numpy EPnP of tests/epnp_ref.py, which tests/test_epnp_ref.py pins on the CPU.

TOL = 1e-7 is the tolerance tests/test_gpu_pnp.py uses for device against oracle poses; two CPU
restatements of EPnP through eigen solvers of different families agree to about 1e-10
(test_epnp_ref.py), so the gate carries three orders of margin."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pnp as O
from tests import epnp_ref as E
from tests.test_pnp_oracle import K_LM, K_SELF

pytestmark = pytest.mark.gpu

TOL = 1e-7
NOISES = (0.0, 1.0, 3.0)
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
# (pn, b, float64 points, per-image models and cameras): every pn with both point types and both
# layouts, b = 1 / 3 / 130 (more blocks than one CU holds); the noise level cycles over the images
CASES = [(6, 1, True, False), (6, 3, False, True), (7, 3, True, True), (7, 1, False, False),
         (9, 130, True, True), (9, 3, False, False), (21, 130, False, True), (21, 1, True, False),
         (63, 3, True, True), (63, 1, False, False), (64, 130, True, False), (64, 3, False, True)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def make_batch(seed, pn, b, per_image):
    """Synthetic poses: p3 [pn, 3] or [b, pn, 3], K [3, 3] or [b, 3, 3] (a different K per image, so
    a wrong stride shows), p2 f64 [b, pn, 2] with noise NOISES[(seed + i) % 3] on image i."""
    rng = np.random.default_rng(seed)
    if per_image:
        p3 = np.stack([E.random_model(rng, pn) for _ in range(b)])
        K = np.stack([K_LM * np.array([[1 + 0.1 * rng.uniform(-1, 1)], [1 + 0.1 * rng.uniform(-1, 1)], [1.0]])
                      for _ in range(b)])
        K[:, 0, 2] += rng.uniform(-20, 20, b)
        K[:, 1, 2] += rng.uniform(-20, 20, b)
    else:
        p3 = E.cuboid_model() if pn == 9 else E.random_model(rng, pn)
        K = K_SELF if seed % 2 else K_LM
    Rt = np.stack([E.random_pose(rng, 3.0) for _ in range(b)])
    p2 = np.empty((b, pn, 2))
    for i in range(b):
        p2[i] = E.project(Rt[i], p3[i] if per_image else p3, K[i] if per_image else K)
        p2[i] += NOISES[(seed + i) % 3] * rng.standard_normal((pn, 2))
    return dict(p3=p3, K=K, p2=p2, Rt=Rt, per_image=per_image)


def reference(bt, p2):
    return [E.epnp(bt["p3"][i] if bt["per_image"] else bt["p3"], p2[i], bt["K"][i] if bt["per_image"] else bt["K"])
            for i in range(p2.shape[0])]


def run_device(bt, p2, device, method="epnp"):
    from pvnet_amd import extend_utils as X
    diag = {}
    Rt = X.pnp_batch(torch.from_numpy(p2).to(device), torch.from_numpy(bt["p3"]).to(device),
                     torch.from_numpy(np.ascontiguousarray(bt["K"])).to(device), method=method, diag=diag)
    torch.cuda.synchronize()
    return Rt.cpu().numpy(), {k: v.cpu().numpy() for k, v in diag.items()}


def device_rt6(bt, p2, device):
    """pv_epnp's rt6 output (the Python layer asks for it only on the epnp_lm path)."""
    from pvnet_amd import _pose_lib as P
    b, pn = p2.shape[:2]
    t2 = torch.from_numpy(p2).to(device)
    t3 = torch.from_numpy(bt["p3"]).to(device)
    tK = torch.from_numpy(np.ascontiguousarray(bt["K"])).to(device)
    f64 = p2.dtype == np.float64
    cb = P.EpnpBatch(b, pn, None if f64 else t2.data_ptr(), t2.data_ptr() if f64 else None, t3.data_ptr(),
                     tK.data_ptr(), pn * 3 if bt["per_image"] else 0, 9 if bt["per_image"] else 0)
    Rt = torch.empty((b, 3, 4), dtype=torch.float64, device=device)
    rt6 = torch.empty((b, 6), dtype=torch.float64, device=device)
    P.check(P.load().pv_epnp(ctypes.byref(cb), Rt.data_ptr(), rt6.data_ptr(), None,
                             torch.cuda.current_stream(device).cuda_stream), "pv_epnp")
    torch.cuda.synchronize()
    return Rt.cpu().numpy(), rt6.cpu().numpy()


@pytest.mark.parametrize("pn,b,f64,per_image", CASES)
def test_device_matches_reference(pn, b, f64, per_image, device):
    bt = make_batch(100 * pn + b, pn, b, per_image)
    p2 = bt["p2"] if f64 else bt["p2"].astype(np.float32)
    ref = reference(bt, p2.astype(np.float64))
    Rt, dg = run_device(bt, p2, device)
    Rt2, rt6 = device_rt6(bt, p2, device)
    np.testing.assert_array_equal(bits(Rt), bits(Rt2))
    worst = dict(Rt=0.0, rt6=0.0, cand_err=0.0)
    compared = 0
    for i, r in enumerate(ref):
        assert r["status"] == E.OK and dg["status"][i] == E.OK, i
        worst["Rt"] = max(worst["Rt"], np.abs(Rt[i] - r["Rt"]).max())
        # the rotation vector is ill-conditioned near pi: compared as a matrix
        worst["rt6"] = max(worst["rt6"], np.abs(O.rodrigues_vec_to_mat(rt6[i, :3]) - r["Rt"][:, :3]).max(),
                           np.abs(rt6[i, 3:] - r["Rt"][:, 3]).max())
        worst["cand_err"] = max(worst["cand_err"], np.abs(dg["cand_err"][i] - r["cand_err"]).max())
        # which candidate won is compared where the reference's two best errors are apart: by more
        # than 1e-9 relative, and by more than TOL px, the resolution cand_err itself is held to.
        # Below that the order cannot be required: on exact data all three are ~1e-13 px, and under
        # noise two starts often reach the same minimum and differ in the last digits only (then the
        # pose is the same whichever wins, and Rt is compared above in any case)
        s = np.sort(r["cand_err"])
        if s[1] - s[0] > max(1e-9 * s[1], TOL):
            compared += 1
            assert dg["n_used"][i] == r["n_used"], (i, r["cand_err"], dg["cand_err"][i])
        assert 1 <= dg["n_used"][i] <= 3
    noisy = sum(NOISES[(100 * pn + b + i) % 3] > 0.0 for i in range(b))
    print(f"pn {pn} b {b} f64 {f64} per-image {per_image}: worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; n_used compared on {compared} images ({noisy} of {b} noisy)")
    # the comparison of n_used is not empty: under noise the candidates are almost always apart
    # the comparison of n_used is not empty: in a large batch at least a third of the noisy images
    # have their two best candidates apart (in the reference; this does not depend on the device)
    assert b < 100 or compared >= noisy // 3
    assert worst["Rt"] < TOL and worst["rt6"] < TOL and worst["cand_err"] < TOL
    # noise-free images recover the true pose (f32 points: to their rounding)
    for i in range(b):
        if NOISES[(100 * pn + b + i) % 3] == 0.0:
            assert np.abs(Rt[i] - bt["Rt"][i]).max() < (1e-9 if f64 else 1e-4)


def test_degenerate_images_in_a_batch(device):
    """A planar model (through the per-image stride), a NaN keypoint, an infinite one and all-zero
    keypoints between good images: [I | 0] and DEGENERATE for them, the neighbours untouched."""
    pn, b = 9, 9
    bt = make_batch(4, pn, b, True)
    bt["p3"][1, :, 2] = 0.01
    bt["p2"][3, 4, 1] = np.nan
    bt["p2"][5, 0, 0] = np.inf
    bt["p2"][7] = 0.0
    for p2 in (bt["p2"], bt["p2"].astype(np.float32)):
        ref = reference(bt, p2.astype(np.float64))
        Rt, dg = run_device(bt, p2, device)
        _, rt6 = device_rt6(bt, p2, device)
        for i in range(b):
            if i in (1, 3, 5, 7):
                assert ref[i]["status"] == E.DEGENERATE and dg["status"][i] == E.DEGENERATE, i
                np.testing.assert_array_equal(Rt[i], IDENT)
                np.testing.assert_array_equal(rt6[i], np.zeros(6))
            else:
                assert dg["status"][i] == E.OK
                assert np.abs(Rt[i] - ref[i]["Rt"]).max() < TOL and np.abs(dg["cand_err"][i] - ref[i]["cand_err"]).max() < TOL
        assert np.isfinite(Rt).all() and np.isfinite(rt6).all()
        # epnp_lm starts the refinement from the zero pose there, as the P3P path without a root
        # does; with a keypoint that is not finite the cost is not either and the start is returned
        Rl, dl = run_device(bt, p2, device, "epnp_lm")
        for i in (3, 5):
            np.testing.assert_array_equal(Rl[i], IDENT)
        # the planar model and the all-zero keypoints have a finite cost at the zero pose: the LM runs
        # from it and returns a finite pose and a status of its own; the good neighbours are refined
        assert np.isfinite(Rl).all()
        assert ((dl["lm_status"] >= 1) & (dl["lm_status"] <= 5)).all() and (dl["iterations"] >= 0).all()
        np.testing.assert_array_equal(dl["status"], dg["status"])
        good = [0, 2, 4, 6, 8]
        alone, _ = run_device(dict(bt, p3=bt["p3"][good], K=bt["K"][good]), p2[good], device, "epnp_lm")
        np.testing.assert_array_equal(bits(Rl[good]), bits(alone))


def test_two_runs_are_bit_equal(device):
    bt = make_batch(11, 21, 130, True)
    for method in ("epnp", "epnp_lm"):
        a, da = run_device(bt, bt["p2"], device, method)
        b_, db = run_device(bt, bt["p2"], device, method)
        np.testing.assert_array_equal(bits(a), bits(b_))
        for k in da:
            np.testing.assert_array_equal(da[k], db[k])
    assert set(da) == {"status", "n_used", "cand_err", "iterations", "lm_status", "cost"}


def test_epnp_lm_matches_the_cpu_chain(device):
    """EPnP -> Levenberg-Marquardt on the device against epnp_ref -> oracle.pnp.ceres_lm.  The LM stops
    on thresholds, so only images whose CPU chain is itself stable are compared: a start moved by
    1e-9 must move the oracle's result by less than 1e-8 (at most 1 image in 10 may fail that)."""
    pn, b = 9, 10
    bt = make_batch(21, pn, b, True)
    w = np.tile(np.array([1.0, 0.0, 1.0]), (pn, 1))
    want, stable = [], []
    for i, r in enumerate(reference(bt, bt["p2"])):
        assert r["status"] == E.OK
        x = O.ceres_lm(r["rt6"], bt["p2"][i], bt["p3"][i], w, bt["K"][i])
        x2 = O.ceres_lm(r["rt6"] + 1e-9 * np.array([1, -1, 1, -1, 1, -1.0]), bt["p2"][i], bt["p3"][i], w, bt["K"][i])
        stable.append(bool(np.abs(x - x2).max() < 1e-8))
        want.append(np.concatenate([O.rodrigues_vec_to_mat(x[:3]), x[3:, None]], 1))
    assert sum(stable) >= b - 1, stable
    Rt, dg = run_device(bt, bt["p2"], device, "epnp_lm")
    worst = max(np.abs(Rt[i] - want[i]).max() for i in range(b) if stable[i])
    print(f"epnp_lm vs CPU chain: worst {worst:.2e} over {sum(stable)} stable images of {b}")
    assert worst < TOL
    assert (dg["status"] == E.OK).all() and (dg["iterations"] >= 0).all() and np.isfinite(dg["cost"]).all()


def test_rt6_to_Rt(device):
    from pvnet_amd import _pose_lib as P
    rng = np.random.default_rng(3)
    r = rng.standard_normal((130, 6))
    r[0, :3] = 0.0
    r[1, :3] = 1e-17
    r[2, :3] = np.array([1.0, 0, 0]) * np.pi
    r[3, :3] = np.array([0.6, 0.0, 0.8]) * (np.pi - 1e-9)
    r[4, :3] = np.array([0.0, -1.0, 0.0]) * (np.pi + 1e-9)
    r[5, :3] = 1e-9
    src = torch.from_numpy(r).to(device)
    out = torch.empty((130, 3, 4), dtype=torch.float64, device=device)
    P.check(P.load().pv_rt6_to_Rt(src.data_ptr(), out.data_ptr(), 130, torch.cuda.current_stream(device).cuda_stream),
            "pv_rt6_to_Rt")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(130):
        assert np.abs(got[i, :, :3] - O.rodrigues_vec_to_mat(r[i, :3])).max() < 1e-12, i
        np.testing.assert_array_equal(got[i, :, 3], r[i, 3:])


def test_graph_capture(device):
    """pnp_batch(method="epnp_lm") captured on one stream after one eager call; replays are bit-equal to eager."""
    from pvnet_amd import extend_utils as X
    bt = make_batch(31, 9, 130, True)
    p2, p3, K = (torch.from_numpy(np.ascontiguousarray(bt[k])).to(device) for k in ("p2", "p3", "K"))
    ref = X.pnp_batch(p2, p3, K, method="epnp_lm").clone()
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gph, stream=s):
            out = X.pnp_batch(p2, p3, K, method="epnp_lm")
    for _ in range(2):
        out.zero_()
        gph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(ref.cpu().numpy()))
    assert np.abs(ref.cpu().numpy()[0] - bt["Rt"][0]).max() < 0.1


def test_captured_graph_survives_a_larger_eager_call(device):
    """A graph captured at one shape holds the unit-weight buffer's pointer; an eager call that needs a
    larger buffer (and others after it that allocate) must leave the graph's replays bit-equal to eager."""
    from pvnet_amd import extend_utils as X
    small = make_batch(51, 9, 130, True)
    p2, p3, K = (torch.from_numpy(np.ascontiguousarray(small[k])).to(device) for k in ("p2", "p3", "K"))
    ref = X.pnp_batch(p2, p3, K, method="epnp_lm").clone()
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gph, stream=s):
            out = X.pnp_batch(p2, p3, K, method="epnp_lm")
    rows = max(t.shape[0] for t in X._unit_weights[p2.device])
    big = make_batch(52, 64, rows // 64 + 3, False)             # b * pn above every buffer made so far
    q2, q3, qK = (torch.from_numpy(np.ascontiguousarray(big[k])).to(device) for k in ("p2", "p3", "K"))
    assert q2.shape[0] * q2.shape[1] > rows
    big_ref = X.pnp_batch(q2, q3, qK, method="epnp_lm")
    junk = [torch.full((n, 3), float("nan"), dtype=torch.float64, device=device) for n in (1024, 130 * 9, rows, 64)]
    torch.cuda.synchronize()
    assert max(t.shape[0] for t in X._unit_weights[p2.device]) > rows
    for _ in range(2):
        out.zero_()
        gph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(ref.cpu().numpy()))
    assert np.isfinite(big_ref.cpu().numpy()).all() and len(junk) == 4


def evaluator_scene(device, b=24, noise=0.0):
    """Two models (one flagged symmetric), keypoints of random poses."""
    from pvnet_amd.evaluation_utils import Evaluator, ModelTable
    rng = np.random.default_rng(9)
    kp = np.stack([E.cuboid_model(), E.random_model(rng, 9)])
    verts = [rng.uniform(-1, 1, (300, 3)) * np.array([0.06, 0.04, 0.025]) for _ in range(2)]
    table = ModelTable([(verts[0], 0.15, False), (verts[1], 0.15, True)], device=device)
    mid = rng.integers(0, 2, b)
    Rt = np.stack([E.random_pose(rng, 3.0) for _ in range(b)])
    p2 = np.stack([E.project(Rt[i], kp[mid[i]], K_LM) for i in range(b)]) + noise * rng.standard_normal((b, 9, 2))
    return Evaluator(table, kp), torch.from_numpy(p2).to(device), torch.from_numpy(Rt).to(device), mid


@pytest.mark.parametrize("method", ["epnp", "epnp_lm"])
def test_evaluator_records_all_hits(method, device):
    ev, p2, Rt, mid = evaluator_scene(device)
    pose = ev.evaluate(p2, Rt, mid, K_LM, method=method)
    assert float((pose - Rt).abs().max()) < 1e-6
    assert ev.average_precision() == (1.0, 1.0, 1.0)


def test_evaluator_default_is_unchanged(device):
    """No keyword, method="p3p_lm" and the call the default made before the keyword existed: bit-equal poses."""
    from pvnet_amd.extend_utils import uncertainty_pnp_batch
    ev, p2, Rt, mid = evaluator_scene(device, noise=0.5)
    a = ev.evaluate(p2, Rt, mid, K_LM)
    b_ = ev.evaluate(p2, Rt, mid, K_LM, method="p3p_lm")
    w = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64, device=device).expand(p2.shape[0], p2.shape[1], 3)
    c = uncertainty_pnp_batch(p2, w, ev.points_3d[torch.from_numpy(mid).to(device)], K_LM, mode="weights")
    np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(b_.cpu().numpy()))
    np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(c.cpu().numpy()))


def test_numpy_wrapper_is_row_zero_of_the_batch(device):
    from pvnet_amd import extend_utils as X
    bt = make_batch(41, 9, 3, False)
    for method in ("epnp", "epnp_lm"):
        Rt, _ = run_device(bt, bt["p2"], device, method)
        one = X.pnp(bt["p3"], bt["p2"][0], bt["K"], method=method)      # the reference's argument order
        assert one.shape == (3, 4) and one.dtype == np.float64
        np.testing.assert_array_equal(bits(one), bits(Rt[0]))
