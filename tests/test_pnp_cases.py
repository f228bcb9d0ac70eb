"""CPU proofs for tests/pnp_cases.py: every scene reaches the branch, the selection
or the stop state it is named for (by the oracle, and by the device's quartic
restated in Python), and every LM scene's decisions sit far enough from their
thresholds that the GPU test may demand the same iterations and status.

Counts that DESIGN.md 10a quotes are asserted here: the ``face_on`` family with a
single order of the three solving points (the parent's P3P) against the three
pooled cyclic orders."""
import os

import numpy as np
import pytest

from oracle import pnp as P
from tests import pnp_cases as C

SINGLE = ((0, 1, 2),)
TRUE_POSE_FAMILIES = ("generic", "box", "face_on", "theta_pi", "identity")


def _errors(name, roots, orders):
    f = C.p3p_family(name)
    res = [C.p3p_error(f["p3"][i], f["p2"][i], roots, orders) for i in range(len(f["p3"]))]
    return np.array([ok for ok, _ in res]), np.array([e for _, e in res])


# ---------------------------------------------------------------------------- the quartic's classifier
def test_device_quartic_finds_known_roots_in_each_branch():
    # (x^2 - 1)(x^2 - 4): biquadratic
    r, br = C.device_quartic([1.0, 0.0, -5.0, 0.0, 4.0])
    assert br == {"biquadratic"}
    np.testing.assert_allclose(sorted(r), [-2, -1, 1, 2], atol=1e-12)
    # (x - 1)(x - 2)(x - 3)(x - 5): Ferrari
    r, br = C.device_quartic(np.poly([1, 2, 3, 5]))
    assert br == {"ferrari"}
    np.testing.assert_allclose(sorted(r), [1, 2, 3, 5], atol=1e-10)
    # (x - 1)^2 (x + 1)(x + 2): a double root, a discriminant that is zero up to rounding
    r, br = C.device_quartic(np.poly([1, 1, -1, -2]))
    assert "ferrari" in br and len(r) == 4
    np.testing.assert_allclose(sorted(r), [-2, -1, 1, 1], atol=1e-6)
    # x^4 + 1: no real root
    assert C.device_quartic([1.0, 0.0, 0.0, 0.0, 1.0])[0] == []
    assert C.device_quartic([0.0, 1.0, 0.0, 0.0, 1.0]) == ([], set())


def test_device_quartic_agrees_with_numpy_roots_on_generic_scenes():
    f = C.p3p_family("generic")
    for i in range(32):
        A = C.grunert_coefficients(f["p3"][i, :3], f["p2"][i, :3])
        dev, br = C.device_quartic(A)
        assert br == {"ferrari"}
        ref = sorted(P.real_roots4(A))
        assert len(dev) == len(ref)
        np.testing.assert_allclose(sorted(dev), ref, rtol=1e-8, atol=1e-10)


# ---------------------------------------------------------------------------- P3P families
def test_family_sizes_and_determinism():
    for name, n in C.P3P_SIZES.items():
        f = C.p3p_family(name)
        assert f["p3"].shape == (n, 4, 3) and f["p2"].shape == (n, 4, 2) and f["p2"].dtype == np.float64
        C.p3p_family.cache_clear()
        g = C.p3p_family(name)
        assert all(np.array_equal(f[k], g[k]) for k in f)


def test_face_on_is_what_it_says():
    f = C.p3p_family("face_on")
    br = [C.scene_branches(f["p3"][i], f["p2"][i]) for i in range(len(f["p3"]))]
    assert sum("biquadratic" in b for b in br) >= 2
    assert sum("snap" in b for b in br) >= 2
    for R, t in zip(f["R"], f["t"]):
        assert set(np.abs(R).ravel()) == {0.0, 1.0} and np.linalg.det(R) == 1.0 and t[0] == t[1] == 0.0
    for name in ("generic", "box"):
        g = C.p3p_family(name)
        assert all(C.scene_branches(g["p3"][i], g["p2"][i]) == {"ferrari"} for i in range(len(g["p3"])))


def test_theta_pi_and_identity_rotations_are_exact():
    f = C.p3p_family("theta_pi")
    for R in f["R"]:
        np.testing.assert_allclose(R @ R, np.eye(3), atol=1e-15)
        assert abs(np.trace(R) + 1.0) < 1e-15
    for R in f["R"][:3]:
        assert set(np.diag(R)) == {1.0, -1.0} and np.count_nonzero(R) == 3
    assert all(np.array_equal(R, np.eye(3)) for R in C.p3p_family("identity")["R"])


@pytest.mark.parametrize("name", TRUE_POSE_FAMILIES)
def test_pooled_p3p_recovers_the_true_pose(name):
    """The fixed P3P (three pooled cyclic orders), with numpy's roots and with the
    device's: a pose for every scene, all four points within 1e-3 px.  The oracle's
    largest error times 10 (at least 1e-6 px) is the GPU test's tolerance."""
    for roots in (None, C.device_roots):
        ok, err = _errors(name, roots, P.P3P_ORDERS)
        assert ok.all()
        assert err.max() <= 1e-4, err.max()      # x10 stays within the 1e-3 px the wrong candidates start at
    print(name, "oracle max err px", _errors(name, None, P.P3P_ORDERS)[1].max(),
          "device roots", _errors(name, C.device_roots, P.P3P_ORDERS)[1].max())


def test_single_order_p3p_misses_face_on_scenes():
    """The defect the pooling fixes: one order of the three solving points (the P3P
    before the fix) loses well-posed face-on scenes, the pooled orders none."""
    for roots in (None, C.device_roots):
        ok, err = _errors("face_on", roots, SINGLE)
        assert (~ok | (err > 1e-3)).sum() == 6 and err[ok & (err > 1e-3)].min() > 0.5
    ok, err = _errors("face_on", None, SINGLE)
    assert (~ok).sum() == 2
    for name in ("generic", "box"):
        ok, err = _errors(name, C.device_roots, SINGLE)
        assert ok.all() and err.max() < 1e-3


def test_collinear_scenes_have_no_pose():
    f = C.p3p_family("collinear")
    for i in range(len(f["p3"])):
        for roots in (None, C.device_roots):
            ok, rv, t = P.p3p_pose(f["p3"][i], f["p2"][i], C.K, roots=roots)
            assert not ok and not rv.any() and not t.any()
    assert any(C.grunert_coefficients(p[:3], x[:3]) is None for p, x in zip(f["p3"], f["p2"]))   # b2 == 0
    c5 = C.collinear5()
    for i in range(len(c5["p3"])):
        d = {}
        Rt = P.uncertainty_pnp(c5["p2"][i], c5["w"][i], c5["p3"][i], C.K, diag=d)
        assert list(d["idxs"]) == [1, 2, 3, 4] and not d["p3p_ok"]
        assert d["status"] == "max_iterations" and d["iterations"] == 0 and not np.isfinite(d["cost"])
        assert np.array_equal(Rt, np.eye(3, 4))


def test_equilateral_triangle_on_its_axis_is_a_known_limit():
    """Documented, not demanded: the 3-fold symmetry makes every order degenerate alike."""
    bad = 0
    for s in range(20):
        p3, p2 = C.equilateral_scene(s)
        ok, e = C.p3p_error(p3, p2)
        bad += (not ok) or e > 1e-3
    assert bad >= 15


# ---------------------------------------------------------------------------- selection
def test_selection_scenes_select_what_they_say():
    scenes = C.selection_scenes()
    assert {s["name"] for s in scenes} == {"all_equal", "tie_straddles_cut", "nan_weights", "cov_gated",
                                           "cov_v2_gated", "cov_v2_nan_c00", "cov_v2_nan_c11"}
    for sc in scenes:
        Rt, d = C.selection_oracle(sc)
        assert [int(i) for i in d["idxs"]] == sc["expect"], sc["name"]
        assert d["p3p_ok"], sc["name"]
        if sc["name"] in ("nan_weights", "cov_v2_nan_c11"):
            assert d["status"] == "max_iterations" and d["iterations"] == 0 and not np.isfinite(d["cost"])
            np.testing.assert_array_equal(Rt, P._rt(d["init"][:3], d["init"][3:]))
        else:
            assert np.isfinite(d["cost"]) and d["iterations"] > 0
        # another four, or another order of the same four, is another start
        for other in (sc["expect"][::-1], [i for i in range(9) if i not in sc["expect"]][:4]):
            ok, rv, t = P.p3p_pose(sc["p3"][other], sc["p2"][other], C.K)
            assert not ok or np.abs(np.concatenate([rv, t]) - d["init"]).max() > 1e-4, sc["name"]


def test_weights_v2_gates_a_nan_c00_and_keeps_other_nans():
    cov = np.tile(np.eye(2, dtype=np.float32), (4, 1, 1))
    cov[0, 0, 0] = np.nan
    cov[1, 1, 1] = np.nan
    cov[2, 0, 1] = np.nan
    w = P.weights_v2(cov)
    assert np.array_equal(w[0], [0.0, 0.0, 0.0])
    assert np.isnan(w[1, 0]) and np.isnan(w[2, 0]) and w[3, 0] == 1.0
    sc = [s for s in C.selection_scenes() if s["name"] == "cov_v2_nan_c00"][0]
    top = int(np.nonzero(np.isnan(sc["wgt"][:, 0, 0]))[0][0])
    assert top not in sc["expect"]


# ---------------------------------------------------------------------------- LM scenes
@pytest.mark.parametrize("kind", C.LM_KINDS)
def test_lm_scenes_reach_their_state_with_margin(kind):
    scenes = C.lm_scenes(kind)
    assert [sc["pn"] for sc, _, _ in scenes] == [pn for pn in C.LM_PNS for _ in range(C.N_PER)]
    for sc, out, d in scenes:
        assert d["margin"] >= 1e-6, (kind, sc["pn"], sc["seed"], d["margin"])
        if kind in C.LM_EXPECT:
            assert d["status"] == C.LM_EXPECT[kind], (kind, sc["pn"], sc["seed"], d["status"])
        assert all(r["h_max"] <= 1e307 for r in d["trace"])      # the device's unscaled J^T J stays finite
    if kind in ("zero_weights", "zero_weights_full", "exact"):
        assert all(d["iterations"] == 0 for _, _, d in scenes)
    if kind == "zero_weights":
        assert all(np.array_equal(out, sc["x0"]) for sc, out, _ in scenes)
    if kind == "zero_weights_full":
        assert all(d["p3p_ok"] and np.array_equal(out, P._rt(d["init"][:3], d["init"][3:])) for _, out, d in scenes)
    if kind == "parameter":
        assert all(d["iterations"] == 1 for _, _, d in scenes)
    if kind == "identity":
        for sc, out, d in scenes:
            assert not sc["x0"][:3].any() and d["iterations"] >= 2
            assert out[:3] @ out[:3] <= P.EPS          # the solution sits in the small-angle branch of the jets
    if kind == "nonfinite":
        assert all(d["iterations"] == 0 and not np.isfinite(d["cost"]) and not out.any() for _, out, d in scenes)
    if kind in ("far", "far_overflow"):
        for sc, _, d in scenes:
            rejected, nonfinite, grew = C.far_properties(d)
            assert rejected and grew and nonfinite == (kind == "far_overflow"), (sc["pn"], sc["seed"])
            assert all(r["chol_ok"] for r in d["trace"])
    if kind == "far":
        assert sum(d["status"] == "max_iterations" and d["iterations"] == 50 for _, _, d in scenes) == 2
    if kind == "full_noisy":
        assert all(d["p3p_ok"] and d["status"] == "function" for _, _, d in scenes)


def test_lm_scenes_cover_the_stop_states():
    seen = {d["status"] for kind in C.LM_KINDS for _, _, d in C.lm_scenes(kind)}
    assert seen == {"gradient", "function", "parameter", "max_iterations"}      # RADIUS: see the module docstring
    assert set(C.STOP) == seen | {"p3p_only", "radius"}
    from pvnet_amd import _lib
    assert {v: k for k, v in C.STOP.items()} == _lib.PNP_STOP
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "pvvote.h")).read()
    names = dict(gradient="GRADIENT", parameter="PARAMETER", function="FUNCTION", max_iterations="MAX_ITER",
                 radius="RADIUS", p3p_only="P3P_ONLY")
    for k, v in C.STOP.items():
        assert f"#define PV_PNP_STOP_{names[k]} {v}" in hdr


@pytest.mark.parametrize("kind", C.LM_KINDS)
def test_lm_scenes_do_not_hang_on_rounding(kind):
    """``margin`` is relative to the tested quantity, which says little where that quantity is itself
    rounding (exact data end at residuals of 1e-9 px and less) or where a long path amplifies it.  So
    move every image point by the rounding of a projection: the oracle takes the same path, and a cost
    that is not itself rounding keeps to a tenth of the GPU test's rtol."""
    for sc, _, d in C.lm_scenes(kind):
        same, spread = C.rounding_spread(sc, d)
        assert same, (kind, sc["pn"], sc["seed"])
        if kind not in C.EXACT_KINDS:
            assert spread <= 1e-10, (kind, sc["pn"], sc["seed"], spread)


def test_bounded_search_finds_no_radius_stop():
    """A sample of pnp_cases.radius_search (the module docstring gives the 3,000-draw result)."""
    assert C.radius_search(100) == ([], [])


def test_far_seeds_are_what_the_searches_find():
    assert tuple(C.far_search(5, want=2, draws=100))[-1:] == C.SEEDS["far_overflow", 5][:1]
    found = C.max_iter_search(5, draws=60)
    assert [s for s, _, _ in found] == [6, 56] and found[0][2] > 1e-6 and found[1][2] < 1e-10


# ---------------------------------------------------------------------------- the 64 images of test_gpu_pnp.py
@pytest.mark.parametrize("mode", ["cov", "cov_v2"])
def test_full_batch_margins(mode):
    _, _, _, refs = C.full_batch(mode)
    assert len(refs) == 64
    assert min(d["margin"] for _, d in refs) >= 1e-6
    assert np.mean([bool(d["p3p_ok"]) for _, d in refs]) > 0.9
