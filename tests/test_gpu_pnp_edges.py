"""The device uncertainty PnP (pv_uncertainty_pnp, pvpnp.hip) at its edges: the
P3P against the true pose, the four-point selection under ties and NaNs, the
trust-region LM in each reachable stop state, batch isolation.  The scenes and
the CPU proofs that each one is what it is named for: tests/pnp_cases.py,
tests/test_pnp_cases.py.

P3P tolerances (pixels, all four points reprojected by the device's init_rt and
by its Rt): ten times the oracle's own largest error on the family (for the
differing root finders), at least 1e-6, never above 1e-3 (the closest wrong
candidate of the face-on scenes is 0.65 px off):

    family    oracle's largest error   tolerance   device's largest error
    generic   2.3e-07                  2.3e-06     3.8e-08
    box       3.5e-08                  1.0e-06     3.4e-09
    face_on   1.5e-06                  1.5e-05     1.2e-06
    theta_pi  1.0e-06                  1.0e-05     1.7e-06
    identity  9.8e-09                  1.0e-06     9.3e-09

Before the three cyclic orders of the solving points were pooled, 6 of the 128
face_on scenes came back 0.65 to 117 px off.

LM: iterations and status equal the oracle's on every scene (their decisions sit
at a relative margin >= 1e-6 from the thresholds, test_pnp_cases.py); the cost
within rtol 1e-9, the module's agreement between the two summation orders, plus
the rounding floor of pnp_cases.cost_floor, which matters only where the cost is
itself rounding (exact data: costs of 1e-11 and less, which differ by up to 2e-4
of themselves).  Measured: the largest relative difference of a cost above 1e-6
is 3.2e-13."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pnp as P
from tests import pnp_cases as C
from tests.test_gpu_pnp import TOL, eu  # noqa: F401 (eu is a fixture)

pytestmark = pytest.mark.gpu

P3P_ONLY, MAX_ITER = C.STOP["p3p_only"], C.STOP["max_iterations"]
EYE34 = np.eye(3, 4)


def _run(eu, device, p2, wgt, p3, mode="weights", x0=None):
    """One launch -> (out, diag as numpy)."""
    diag = {}
    out = eu.uncertainty_pnp_batch(torch.from_numpy(np.ascontiguousarray(p2)).to(device),
                                   torch.from_numpy(np.ascontiguousarray(wgt)).to(device), p3, C.K, mode=mode,
                                   init_rt=None if x0 is None else torch.from_numpy(np.ascontiguousarray(x0)).to(device),
                                   diag=diag)
    return out.cpu().numpy(), {k: v.cpu().numpy() for k, v in diag.items()}


def _rt(x):
    return P._rt(x[:3], x[3:])


# ---------------------------------------------------------------------------- P3P against the truth
@pytest.mark.parametrize("name", ["generic", "box", "face_on", "theta_pi", "identity"])
def test_p3p_recovers_the_true_pose(name, device, eu):
    f = C.p3p_family(name)
    n = len(f["p3"])
    own = max(C.p3p_error(f["p3"][i], f["p2"][i])[1] for i in range(n))
    tol = max(10.0 * own, 1e-6)
    assert tol <= 1e-3
    Rt, d = _run(eu, device, f["p2"], np.tile(C.UNIT_W, (n, 4, 1)), f["p3"])
    assert (d["p3p_ok"] == 1).all(), np.nonzero(d["p3p_ok"] != 1)[0]
    assert (d["status"] == P3P_ONLY).all() and (d["iterations"] == 0).all()
    e_init = np.array([C.four_point_error(f["p3"][i], f["p2"][i], _rt(d["init_rt"][i])) for i in range(n)])
    e_rt = np.array([C.four_point_error(f["p3"][i], f["p2"][i], Rt[i]) for i in range(n)])
    print(f"p3p {name}: oracle {own:.3g} px, tol {tol:.3g}, device init_rt {e_init.max():.3g}, Rt {e_rt.max():.3g}")
    assert e_init.max() <= tol, (np.nonzero(e_init > tol)[0], e_init.max())
    assert e_rt.max() <= tol, (np.nonzero(e_rt > tol)[0], e_rt.max())
    # the rotation itself, as a matrix (at theta = pi either axis sign is the same rotation).  The
    # reprojection above is the tight check; 1e-4 tells the true pose from any other candidate
    np.testing.assert_allclose(Rt[:, :, :3], f["R"], atol=1e-4)
    # the final cost is the P3P pose's: 0.5 sum r^2 <= 0.5 * 4 * tol^2
    assert (d["cost"] <= 2.0 * tol * tol).all()


def test_collinear_points_have_no_pose(device, eu):
    f = C.p3p_family("collinear")
    n = len(f["p3"])
    Rt, d = _run(eu, device, f["p2"], np.tile(C.UNIT_W, (n, 4, 1)), f["p3"])
    assert (d["p3p_ok"] == 0).all() and (d["status"] == P3P_ONLY).all() and (d["iterations"] == 0).all()
    assert not d["init_rt"].any()
    assert all(np.array_equal(Rt[i], EYE34) for i in range(n))
    # with a fifth point the LM starts from the zero pose, whose cost is not finite: as the oracle
    c5 = C.collinear5()
    Rt, d = _run(eu, device, c5["p2"], c5["w"], c5["p3"])
    assert (d["p3p_ok"] == 0).all() and (d["status"] == MAX_ITER).all() and (d["iterations"] == 0).all()
    assert not np.isfinite(d["cost"]).any()
    assert all(np.array_equal(Rt[i], EYE34) for i in range(n))


# ---------------------------------------------------------------------------- selection
@pytest.mark.parametrize("mode", ["weights", "cov", "cov_v2"])
def test_selection_matches_oracle(mode, device, eu):
    scenes = [s for s in C.selection_scenes() if s["mode"] == mode]
    Rt, d = _run(eu, device, np.stack([s["p2"] for s in scenes]), np.stack([s["wgt"] for s in scenes]),
                 scenes[0]["p3"], mode=mode)
    for i, sc in enumerate(scenes):
        ref, o = C.selection_oracle(sc)
        what = f"{sc['name']} seed {sc['seed']}"
        assert d["p3p_ok"][i] == 1, what
        np.testing.assert_allclose(d["init_rt"][i], o["init"], atol=1e-6, err_msg=what)
        if sc["name"] in ("nan_weights", "cov_v2_nan_c11"):     # a NaN weight: the result is the start
            assert not np.isfinite(d["cost"][i]) and d["status"][i] == MAX_ITER and d["iterations"][i] == 0, what
            np.testing.assert_allclose(Rt[i], _rt(d["init_rt"][i]), atol=1e-15, err_msg=what)
        elif not sc["name"].endswith("_gated"):                  # (two weighted points do not pin a pose)
            assert (d["iterations"][i], d["status"][i]) == (o["iterations"], C.STOP[o["status"]]), what
            np.testing.assert_allclose(Rt[i], ref, atol=TOL, err_msg=what)


# ---------------------------------------------------------------------------- LM
@pytest.mark.parametrize("kind", C.LM_KINDS)
def test_lm_takes_the_oracles_path(kind, device, eu):
    scenes = C.lm_scenes(kind)
    worst = 0.0
    for pn in C.LM_PNS:
        grp = [s for s in scenes if s[0]["pn"] == pn]
        full = grp[0][0]["x0"] is None
        out, d = _run(eu, device, np.stack([s[0]["p2"] for s in grp]), np.stack([s[0]["w"] for s in grp]),
                      np.stack([s[0]["p3"] for s in grp]), x0=None if full else np.stack([s[0]["x0"] for s in grp]))
        for i, (sc, ref, o) in enumerate(grp):
            what = f"{kind} pn {pn} seed {sc['seed']}"
            print(f"lm {what}: {o['status']} {o['iterations']} cost {o['cost']:.6g} device {d['cost'][i]:.6g} "
                  f"{d['status'][i]} {d['iterations'][i]}")
            assert d["iterations"][i] == o["iterations"], what
            assert d["status"][i] == C.STOP[o["status"]], what
            if np.isfinite(o["cost"]):
                diff = abs(d["cost"][i] - o["cost"])
                assert diff <= 1e-9 * o["cost"] + C.cost_floor(sc, o["cost"]), (what, d["cost"][i], o["cost"])
                if o["cost"] > 1e-6:
                    worst = max(worst, diff / o["cost"])
            else:
                assert not np.isfinite(d["cost"][i]), what
            np.testing.assert_allclose(out[i], ref, atol=TOL, err_msg=what)
            if full:      # (the start itself: the P3P, selection and 64-image tests)
                assert d["p3p_ok"][i] == bool(o["p3p_ok"]), what
    print(f"lm {kind}: largest relative cost difference above 1e-6: {worst:.3g}")


# ---------------------------------------------------------------------------- batch isolation
def test_batch_copies_are_bit_equal(device, eu):
    """8 scenes (two without a pose, one with NaN weights) tiled to 1,024 images: every copy
    is bit-equal to the first of its scene and to a launch of the 8 alone."""
    sel = {(s["name"], s["seed"]): s for s in C.selection_scenes()}
    scenes = [sel["all_equal", 0], sel["tie_straddles_cut", 1], sel["nan_weights", 0], sel["all_equal", 2],
              sel["tie_straddles_cut", 3]]
    p2 = [s["p2"] for s in scenes]
    w = [s["wgt"] for s in scenes]
    for c in (0, 5):          # keys 2..5 on corner, centre, opposite corner, a neighbour: the solving three on a line
        k = np.ones(9)
        k[[c, 8, 7 - c, (c + 1) % 8]] = [2.0, 3.0, 4.0, 5.0]
        p2.append(scenes[0]["p2"])
        w.append(k[:, None] * C.UNIT_W)
    p2.append(scenes[3]["p2"] + 0.5)
    w.append(sel["tie_straddles_cut", 0]["wgt"])
    p2, w, p3 = np.stack(p2), np.stack(w), scenes[0]["p3"]
    assert len(p2) == 8
    Rt8, d8 = _run(eu, device, p2, w, p3)
    assert list(d8["p3p_ok"]) == [1, 1, 1, 1, 1, 0, 0, 1]
    assert not np.isfinite(d8["cost"][2]) and (d8["status"][[2, 5, 6]] == MAX_ITER).all()
    idx = np.arange(1024) % 8
    Rt, d = _run(eu, device, p2[idx], w[idx], p3)

    def bits(a):
        return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)

    assert np.array_equal(bits(Rt), bits(Rt8)[idx])
    for k in ("init_rt", "p3p_ok", "iterations", "status", "cost"):
        assert np.array_equal(bits(d[k]), bits(d8[k])[idx]), k


# ---------------------------------------------------------------------------- input checks
def test_more_than_64_points_are_rejected(device, eu):
    from pvnet_amd import _lib
    with pytest.raises(RuntimeError, match="4 <= pn"):
        eu.uncertainty_pnp_batch(torch.zeros((2, 65, 2), device=device), torch.zeros((2, 65, 3), device=device),
                                 np.zeros((65, 3)), C.K, mode="weights")
    # the library's own check (nothing is launched or read: the shape is refused first)
    L = _lib.load()
    buf = torch.zeros(65 * 3, dtype=torch.float64, device=device)
    out = torch.zeros(12, dtype=torch.float64, device=device)
    for pn, ok in ((65, False), (3, False), (64, True)):
        bt = _lib.PnpBatch(0, pn, _lib.PV_PNP_WEIGHTS, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, 0,
                           buf.data_ptr())
        rc = L.pv_uncertainty_pnp(ctypes.byref(bt), out.data_ptr(), None, None)
        assert (rc == 0) == ok, (pn, rc)
        rc = L.pv_uncertainty_pnp_refine(ctypes.byref(bt), buf.data_ptr(), out.data_ptr(), None, None)
        assert (rc == 0) == ok, (pn, rc)
