"""tests/bop_ref.py deserves to be the reference of include/pvbop.h: on shapes whose symmetries are
known it gives what the BOP Challenge's definitions give.  CPU only, numpy only."""
import math

import numpy as np
import pytest

from tests import bop_ref as R
from tests import render_ref as RR

K = np.array([[572.4, 0.3, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])
IDENT = np.eye(4)[None, :3]


def diameter(P):
    P = P.astype(np.float64)
    return math.sqrt(max(float(np.max(np.sum((P - p) ** 2, 1))) for p in P))


def add(P, Pe, Pg):
    P = P.astype(np.float64)
    return float(np.mean(np.linalg.norm((P @ Pe[:, :3].T + Pe[:, 3]) - (P @ Pg[:, :3].T + Pg[:, 3]), axis=1)))


def one(P, S, Pe, Pg):
    err, best = R.sym_errors([P], [S], Pe[None], Pg[None], K)
    return float(err[0, 0]), float(err[0, 1]), int(best[0, 0]), int(best[0, 1])


def test_identity_table_is_the_largest_vertex_distance():
    """Against the matrix-product form the difference is rounding alone.  Measured over these cases:
    at most 2.3e-16 absolute with camera-frame coordinates between 0.5 and 1.5 (one ulp of the
    scene's scale); the bound is 4 times that."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for case in range(40):
        P = (rng.normal(size=(int(rng.integers(1, 200)), 3)) * 0.05).astype(np.float32)
        Pg = RR.pose(RR.random_rotation(rng), [rng.normal() * 0.1, rng.normal() * 0.1, 0.5 + rng.random()])
        Pe = RR.pose(RR.random_rotation(rng), [rng.normal() * 0.1, rng.normal() * 0.1, 0.5 + rng.random()])
        mssd, mspd, bs, bp = one(P, IDENT, Pe, Pg)
        P64 = P.astype(np.float64)
        a, g = P64 @ Pe[:, :3].T + Pe[:, 3], P64 @ Pg[:, :3].T + Pg[:, 3]
        want = float(np.max(np.linalg.norm(a - g, axis=1)))
        worst = max(worst, abs(mssd - want))
        pa, pg = a @ K.T, g @ K.T
        want_px = float(np.max(np.linalg.norm(pa[:, :2] / pa[:, 2:] - pg[:, :2] / pg[:, 2:], axis=1)))
        assert abs(mspd - want_px) <= 1e-9 * max(1.0, want_px)
        assert (bs, bp) == (0, 0)
    print("largest |MSSD - matrix form| =", worst)
    assert worst <= 4 * 2.3e-16


@pytest.mark.parametrize("shape", ["cube", "plate"])
def test_discrete_symmetries_score_zero_where_add_does_not(shape):
    P, rots = (R.cube(), R.cube_rotations()) if shape == "cube" else (R.plate(), R.plate_rotations())
    assert len(rots) == (24 if shape == "cube" else 8)
    S = R.symmetries(R.as_info(rots))
    assert S.shape == (len(rots), 3, 4) and np.array_equal(S[0], IDENT[0])
    dia = diameter(P)
    rng = np.random.default_rng(5)
    far = 0
    for k, Rs in enumerate(rots):
        Rg = RR.random_rotation(rng)
        t = [0.03 * rng.normal(), 0.03 * rng.normal(), 0.7]
        Pg, Pe = RR.pose(Rg, t), RR.pose(Rg @ Rs, t)
        mssd, mspd, bs, bp = one(P, S, Pe, Pg)
        assert mssd <= 1e-12 * dia and mspd <= 1e-9, (k, mssd, mspd)
        for bst in (bs, bp):
            assert np.allclose(S[bst, :, :3], Rs, atol=1e-12), (k, bst)     # S itself, or one equal to it
        if k:
            far += add(P, Pe, Pg) > 0.1 * dia
            # without the table the same pair is a wrong pose
            assert one(P, IDENT, Pe, Pg)[0] > 0.1 * dia
    assert far == len(rots) - 1                                            # ADD rejects every one of them


def test_continuous_symmetry_of_a_cup():
    P = R.cup()
    S = R.symmetries({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    assert S.shape == (315, 3, 4)
    dia = diameter(P)
    rmax = float(np.max(np.hypot(P[:, 0].astype(np.float64), P[:, 1].astype(np.float64))))    # of the f32 vertices
    rng = np.random.default_rng(7)
    Rg = RR.random_rotation(rng)
    t = [0.01, -0.02, 0.8]
    step = 2.0 * math.pi / 315
    for mult in (1, 2, 57, 157, 158, 314, 315, -3):
        Pe = RR.pose(Rg @ R.axis_rotation([0, 0, 1], mult * step), t)
        mssd, mspd, bs, bp = one(P, S, Pe, RR.pose(Rg, t))
        # the vertices are f32: the turned cloud meets itself to 2^-24 of its radius, not exactly
        assert mssd <= 1e-6 * dia and mspd <= 1e-3, (mult, mssd, mspd)
        assert bs == bp == mult % 315
    chord = 2.0 * rmax * math.sin(step / 4.0)                              # of half a step, at the largest radius
    for mult in (0.5, 10.5, 200.5):
        Pe = RR.pose(Rg @ R.axis_rotation([0, 0, 1], mult * step), t)
        mssd = one(P, S, Pe, RR.pose(Rg, t))[0]
        # the nearest symmetry is half a step away either way, so the rim moves by that chord: no more
        # than it (but for the rounding of sin, cos and the products), and not much less
        assert 0.0 < 0.99 * chord < mssd <= chord * (1 + 1e-9), (mult, mssd, chord)


def test_symmetry_table_counts_and_orthonormality():
    from pvnet_amd.bop import SymmetryTable, symmetry_transformations
    flip = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
    cont = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.01, -0.02, 0.0]}]}
    both = dict(cont, symmetries_discrete=[flip])
    tab = SymmetryTable([{}, cont, both], device="cpu")
    assert tab.counts == (1, 315, 630) and tab.max_ns == 630 and tab.total == 946 and tab.nmodels == 3
    assert tab.offsets.tolist() == [0, 1, 316, 946] and tuple(tab.syms.shape) == (946, 3, 4)
    S = tab.syms.numpy()
    for lo in tab.offsets.tolist()[:-1]:
        assert np.array_equal(S[lo], IDENT[0])                             # the identity first
    RtR = np.einsum("nij,nik->njk", S[:, :, :3], S[:, :, :3])
    assert np.abs(RtR - np.eye(3)).max() <= 1e-14
    assert np.allclose(np.linalg.det(S[:, :, :3]), 1.0, atol=1e-14)
    # the axis goes through the offset: the offset is a fixed point of every continuous step
    off = np.array([0.01, -0.02, 0.0])
    assert np.abs(S[1:316, :, :3] @ off + S[1:316, :, 3] - off).max() <= 1e-16
    # the restatement in tests/bop_ref.py agrees
    for info, lo, hi in (({}, 0, 1), (cont, 1, 316), (both, 316, 946)):
        assert np.abs(R.symmetries(info) - S[lo:hi]).max() <= 1e-15
    assert symmetry_transformations(cont, max_sym_disc_step=0.5).shape == (7, 3, 4)
    ident = SymmetryTable.identity(4, device="cpu")
    assert ident.counts == (1, 1, 1, 1) and np.array_equal(ident.syms.numpy(), np.repeat(IDENT, 4, 0))
    with pytest.raises(ValueError):
        SymmetryTable([], device="cpu")
    with pytest.raises(ValueError):
        SymmetryTable([{"symmetries_discrete": [[1, 0, 0]]}], device="cpu")


# ---- VSD ---------------------------------------------------------------------------------------------
KV = np.array([[100.0, 0.0, 3.0], [0.0, 100.0, 2.0], [0.0, 0.0, 1.0]])
INF = np.float32(np.inf)


def maps(H=5, W=7, **px):
    """Three [1, H, W] maps: est and gt all background, test all missing, then the given pixels."""
    d = {"t": np.zeros((1, H, W), np.float32), "e": np.full((1, H, W), INF), "g": np.full((1, H, W), INF)}
    for name, items in px.items():
        for (y, x), v in items.items():
            d[name][0, y, x] = v
    return d["t"], d["e"], d["g"]


def run(t, e, g, delta=15.0, taus=(20.0,), **kw):
    return R.vsd(t, e, g, KV, delta, np.asarray(taus, np.float64)[None], **kw)


def test_vsd_identical_disjoint_empty():
    rng = np.random.default_rng(1)
    e = np.full((1, 5, 7), INF)
    e[0, 1:4, 2:6] = 500.0 + 50.0 * rng.random((3, 4))
    t = np.zeros((1, 5, 7), np.float32)
    t[0, 1:3] = 520.0
    counts, err = run(t, e, e.copy(), taus=(0.0, 1e-300, 5.0, 1e9))
    assert counts[0, 0] == counts[0, 1] > 0 and err[0, 1:].tolist() == [0.0, 0.0, 0.0]
    assert err[0, 0] == 1.0                                               # |dg - de| = 0 >= tau = 0: the step cost's edge
    g = np.full((1, 5, 7), INF)
    g[0, 4, 0:2] = 510.0
    counts, err = run(np.zeros((1, 5, 7), np.float32), e, g, taus=(5.0, 1e9))
    assert counts[0].tolist() == [14, 0, 0, 0] and err[0].tolist() == [1.0, 1.0]     # disjoint masks
    counts, err = run(*maps(), taus=(5.0, 7.0))
    assert counts[0].tolist() == [0, 0, 0, 0] and err[0].tolist() == [1.0, 1.0]      # empty union: exactly 1.0
    for bad in (np.nan, -1.0, 0.0, -INF):                                 # "no model" values of a rendered map
        counts, _ = run(*maps(e={(1, 1): bad}, g={(1, 1): bad}))
        assert counts[0, 0] == 0


def test_vsd_missing_sensor_depth_counts_as_visible():
    for missing in (0.0, -5.0, np.nan, INF):
        counts, err = run(*maps(t={(2, 3): missing}, e={(2, 3): 500.0}, g={(2, 3): 500.0}))
        assert counts[0].tolist() == [1, 1, 0] and err[0, 0] == 0.0


def test_vsd_occluder_at_delta_and_beyond():
    y, x = 2, 3                                                           # the principal point: r is exactly 1
    z, delta = 500.0, 15.0
    at = dict(t={(y, x): z - delta}, e={(y, x): z}, g={(y, x): z})
    assert run(*maps(**at), delta=delta)[0][0].tolist() == [1, 1, 0]      # dg - dt == delta: still visible
    eps = np.float32(z - delta) - np.nextafter(np.float32(z - delta), np.float32(0))
    beyond = dict(at, t={(y, x): np.float32(z - delta) - eps})
    counts, err = run(*maps(**beyond), delta=delta)
    assert counts[0].tolist() == [0, 0, 0] and err[0, 0] == 1.0           # hidden in both: no pixel left
    # off the principal point the distances, not the depths, are compared
    off = dict(t={(0, 0): z - delta}, e={(0, 0): z}, g={(0, 0): z})
    r = math.sqrt((0.03 * 0.03 + 0.02 * 0.02) + 1)
    assert (z - (z - delta)) * r > delta
    assert run(*maps(**off), delta=delta)[0][0].tolist() == [0, 0, 0]


def test_vsd_the_gt_clause_of_vis_est_is_reached():
    """The estimate lies behind the sensor's surface by more than delta, the ground truth within
    it: the pixel is visible in the estimate only through `or vis_gt`."""
    px = dict(t={(2, 3): 500.0}, e={(2, 3): 540.0}, g={(2, 3): 505.0})
    counts, err = run(*maps(**px), taus=(20.0, 50.0))
    assert counts[0].tolist() == [1, 1, 1, 0] and err[0].tolist() == [1.0, 0.0]
    counts, err = run(*maps(**px), taus=(20.0, 50.0), drop_gt_clause=True)
    assert counts[0].tolist() == [1, 0, 0, 0] and err[0].tolist() == [1.0, 1.0]


def test_vsd_bad_image_and_camera():
    t, e, g = maps(e={(1, 1): 500.0}, g={(1, 1): 500.0})
    for img in (-1, 1, 99):
        counts, err = R.vsd(t, e, g, KV, 15.0, np.array([[20.0]]), img_id=[img])
        assert (counts == -1).all() and np.isnan(err).all()
    for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)):
        Kb = KV.copy()
        Kb[r, c] = np.nan
        counts, err = R.vsd(t, e, g, Kb, 15.0, np.array([[20.0]]))
        assert (counts == -1).all() and np.isnan(err).all()
    Kb = KV.copy()
    Kb[0, 1] = np.nan                                                     # the skew is not read
    assert R.vsd(t, e, g, Kb, 15.0, np.array([[20.0]]))[0][0].tolist() == [1, 1, 0]
    counts, _ = R.vsd(t, e, g, KV, 15.0, np.array([[np.nan, 0.0]]))
    assert counts[0].tolist() == [1, 1, 0, 1]                             # a NaN tau counts nothing


def test_sym_errors_nan_rules_of_the_reference():
    P = R.cube()
    Pg = RR.pose(np.eye(3), [0, 0, 0.5])
    err, best = R.sym_errors([P], [IDENT], Pg[None], Pg[None], K)
    assert err[0].tolist() == [0.0, 0.0] and best[0].tolist() == [0, 0]   # identical poses: exactly 0
    bad = Pg.copy()
    bad[1, 2] = np.inf
    for pe, pg in ((bad, Pg), (Pg, bad)):
        err, best = R.sym_errors([P], [IDENT], pe[None], pg[None], K)
        assert np.isnan(err).all() and (best == -1).all()
    Sb = np.concatenate([IDENT, IDENT])
    Sb[1, 0, 3] = np.nan
    err, best = R.sym_errors([P], [Sb], Pg[None], Pg[None], K)
    assert np.isnan(err).all() and (best == -1).all()
    Kb = K.copy()
    Kb[0, 1] = np.nan
    err, best = R.sym_errors([P], [IDENT], Pg[None], Pg[None], Kb)
    assert err[0, 0] == 0.0 and np.isnan(err[0, 1]) and best[0].tolist() == [0, -1]
    err, best = R.sym_errors([P], [IDENT], Pg[None], Pg[None], K, model_id=[1])
    assert np.isnan(err).all()
    behind = RR.pose(np.eye(3), [0, 0, 0.02])                             # the cube's near face is behind the camera
    err, best = R.sym_errors([P], [IDENT], behind[None], Pg[None], K)
    assert err[0, 1] == np.inf and best[0, 1] == 0 and np.isfinite(err[0, 0])
    huge = Pg.copy()
    huge[0, 3] = 1e200
    err, best = R.sym_errors([P], [IDENT], huge[None], Pg[None], K)
    assert err[0, 0] == np.inf and best[0, 0] == 0                        # an entry of c_s beyond 2^300
