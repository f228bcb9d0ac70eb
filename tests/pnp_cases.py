"""Scenes for the uncertainty PnP (``pvpnp.hip``) at its edges, and the restated
branch conditions of the device's quartic root finder.

Three groups, all deterministic (fixed seeds) and cached -- treat what these
functions return as read-only:

* ``p3p_family(name)``: pn = 4 scenes with exact float64 projections of a known
  pose (``generic``, ``box``, ``face_on``, ``theta_pi``, ``identity``) and
  ``collinear`` scenes that have no pose.  The GPU test holds the device's P3P
  against the *true pose*, not against the oracle, because the oracle restates
  the same Grunert formulation.
* ``selection_scenes()``: pn = 9, every image point perturbed by a few pixels, so
  that another four points or another order of them is another P3P pose.
* ``lm_scenes()``: pn in {5, 6, 63, 64}, one kind per stop state or branch of the
  trust-region LM.

``device_quartic`` is ``quartic_real_roots`` of ``pvpnp.hip`` line by line in
Python (with ``cubic_largest`` and ``polish``): it returns the roots and the set
of branches taken, so it is both the classifier of the quartic's branches and,
handed to ``oracle.pnp.p3p_pose(roots=...)``, the device's P3P on the CPU.

Stop states: GRADIENT, FUNCTION, PARAMETER and MAX_ITER (0 iterations and 50) are
reached, the first three by construction, the last by a seeded search.  RADIUS is not: ``radius_search`` (3,000 seeded draws of
far starts and extreme weights) finds no scene that ends there.  The radius falls
below 1e-32 only after 16 rejected steps in a row, and a step that small trips the
parameter tolerance first; the only other way, 16 failed Cholesky factorisations,
needs a non-finite Jacobian under a finite cost.  A failed Cholesky factorisation
is not reached by any scene for the same reason (the damped diagonal is at least
1e-6 / radius).

``tests/test_pnp_cases.py`` proves on the CPU that every scene reaches what it is
named for; ``tests/test_gpu_pnp_edges.py`` runs them on the device.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import pnp as P
from tests.test_pnp_oracle import K_LM, box_keypoints, noisy_case, project

K = K_LM
LM_PNS = (5, 6, 63, 64)
UNIT_W = np.array([1.0, 0.0, 1.0])

# PV_PNP_STOP_* of include/pvvote.h by the oracle's status string
STOP = {"gradient": 1, "parameter": 2, "function": 3, "max_iterations": 4, "radius": 5, "p3p_only": 6}


# ----------------------------------------------------------------------------
# quartic_real_roots of pvpnp.hip, restated with its branches
# ----------------------------------------------------------------------------
def _polish(a, x):
    deg = len(a) - 1
    for _ in range(3):
        p, dp = a[0], 0.0
        for i in range(1, deg + 1):
            dp = dp * x + p
            p = p * x + a[i]
        if dp == 0.0 or not math.isfinite(p / dp):
            break
        x -= p / dp
    return x


def _cubic_largest(B, C, D):
    Pc = C - B * B / 3.0
    Q = 2.0 * B * B * B / 27.0 - B * C / 3.0 + D
    disc = 0.25 * Q * Q + Pc * Pc * Pc / 27.0
    if disc > 0.0:
        sq = math.sqrt(disc)
        t = float(np.cbrt(-0.5 * Q + sq) + np.cbrt(-0.5 * Q - sq))
    elif Pc == 0.0:
        t = float(np.cbrt(-Q))
    else:
        rr = math.sqrt(-Pc / 3.0)
        arg = min(max(-0.5 * Q / (rr * rr * rr), -1.0), 1.0)
        t = 2.0 * rr * math.cos(math.acos(arg) / 3.0)
    return _polish([1.0, B, C, D], t - B / 3.0)


def device_quartic(a):
    """-> (real roots, branches).  ``branches`` holds ``"biquadratic"`` (|q| <=
    1e-14 scale) or ``"ferrari"``; with the latter ``"m_nonpositive"`` when the
    resolvent's largest root is <= 0 (no roots), and ``"snap"`` whenever a
    discriminant in (-tol, 0) was set to zero."""
    a = [float(v) for v in a]
    br = set()
    if a[0] == 0.0 or not all(math.isfinite(v) for v in a):
        return [], br
    b, c, d, e = a[1] / a[0], a[2] / a[0], a[3] / a[0], a[4] / a[0]
    b2 = b * b
    p = c - 3.0 * b2 / 8.0
    q = d - 0.5 * b * c + b2 * b / 8.0
    r = e - 0.25 * b * d + b2 * c / 16.0 - 3.0 * b2 * b2 / 256.0
    y = []

    def quad(B1, C1):
        disc = B1 * B1 - 4.0 * C1
        tol = 1e-12 * max(1.0, B1 * B1 + abs(C1))
        if -tol < disc < 0.0:
            br.add("snap")
            disc = 0.0
        if disc < 0.0:
            return
        s = math.sqrt(disc)
        y.extend([0.5 * (-B1 + s), 0.5 * (-B1 - s)])

    scale = max(1.0, abs(p), abs(q), abs(r))
    if abs(q) <= 1e-14 * scale:
        br.add("biquadratic")
        disc = p * p - 4.0 * r
        if -1e-12 * max(1.0, p * p) < disc < 0.0:
            br.add("snap")
            disc = 0.0
        if disc >= 0.0:
            s = math.sqrt(disc)
            for z in (0.5 * (-p + s), 0.5 * (-p - s)):
                if z >= 0.0:
                    y.extend([math.sqrt(z), -math.sqrt(z)])
    else:
        br.add("ferrari")
        m = _cubic_largest(p, 0.25 * p * p - r, -q * q / 8.0)
        if m > 0.0:
            s = math.sqrt(2.0 * m)
            quad(s, 0.5 * p + m - q / (2.0 * s))
            quad(-s, 0.5 * p + m + q / (2.0 * s))
        else:
            br.add("m_nonpositive")
    return [_polish(a, v - 0.25 * b) for v in y], br


def device_roots(a):
    return device_quartic(a)[0]


def grunert_coefficients(P3, x3, Kc=K):
    """A[0..4] of Grunert's quartic in v for world points P3 [3, 3] and image
    points x3 [3, 2] (p3p_pose of pvpnp.hip / p3p_candidates of the oracle);
    None when b2 == 0."""
    P3, x3 = np.asarray(P3, np.float64), np.asarray(x3, np.float64)
    j = np.stack([(x3[:, 0] - Kc[0, 2]) / Kc[0, 0], (x3[:, 1] - Kc[1, 2]) / Kc[1, 1], np.ones(3)], 1)
    j /= np.linalg.norm(j, axis=1, keepdims=True)
    a2, b2, c2 = ((P3[1] - P3[2]) ** 2).sum(), ((P3[0] - P3[2]) ** 2).sum(), ((P3[0] - P3[1]) ** 2).sum()
    if b2 == 0:
        return None
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    amc, apc = (a2 - c2) / b2, (a2 + c2) / b2
    return [(amc - 1) ** 2 - 4 * c2 / b2 * ca ** 2,
            4 * (amc * (1 - amc) * cb - (1 - apc) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb),
            2 * (amc ** 2 - 1 + 2 * amc ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 - 4 * apc * ca * cb * cg
                 + 2 * (b2 - a2) / b2 * cg ** 2),
            4 * (-amc * (1 + amc) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - apc) * ca * cg),
            (1 + amc) ** 2 - 4 * a2 / b2 * cg ** 2]


def scene_branches(p3, p2, order=(0, 1, 2)):
    """The branches the device's quartic takes for points ``order`` of a pn = 4 scene."""
    o = list(order)
    A = grunert_coefficients(p3[o], p2[o])
    return set() if A is None else device_quartic(A)[1]


def four_point_error(p3, p2, Rt):
    """Largest reprojection error (pixels) of Rt [3, 4] over the scene's points."""
    with np.errstate(all="ignore"):
        d = project(Rt[:, :3], Rt[:, 3], p3, K) - p2
        e = np.sqrt((d * d).sum(1)).max()
    return float(e) if np.isfinite(e) else np.inf


def p3p_error(p3, p2, roots=None, orders=P.P3P_ORDERS):
    """(ok, four-point error in pixels) of ``oracle.pnp.p3p_pose`` with the given root finder / orders."""
    ok, rv, t = P.p3p_pose(p3, p2, K, roots=roots, orders=orders)
    if not ok:
        return False, np.inf
    return True, four_point_error(p3, p2, np.concatenate([P.rodrigues_vec_to_mat(rv), t.reshape(3, 1)], 1))


# ----------------------------------------------------------------------------
# P3P families
# ----------------------------------------------------------------------------
def _rand_t(rng):
    return np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.0)])


def _collinear(p):
    return np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0])) < 1e-12


def _box4(rng):
    """4 of the 9 box keypoints by a seeded permutation, the first three not on a line."""
    box = box_keypoints()
    while True:
        p = box[rng.permutation(9)[:4]]
        if not _collinear(p):
            return p


def _axis_rotation(axis, k):
    """Rotation by k * 90 degrees about coordinate axis ``axis``, entries exactly 0 / +-1."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
    R = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _rot_pi(axis):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    return 2.0 * np.outer(k, k) - np.eye(3)


P3P_SIZES = {"generic": 128, "box": 128, "face_on": 128, "theta_pi": 16, "identity": 16, "collinear": 8}


@functools.lru_cache(maxsize=None)
def p3p_family(name):
    """-> dict(p3 [n, 4, 3], p2 [n, 4, 2] exact float64 projections, R [n, 3, 3], t [n, 3])."""
    n = P3P_SIZES[name]
    rng = np.random.default_rng({"generic": 101, "box": 102, "face_on": 103, "theta_pi": 104, "identity": 105,
                                 "collinear": 106}[name])
    p3s, Rs, ts = [], [], []
    box = box_keypoints()
    for i in range(n):
        if name == "generic":
            p3, R, t = rng.uniform(-0.1, 0.1, (4, 3)), P.rodrigues_vec_to_mat(rng.normal(size=3)), _rand_t(rng)
        elif name == "box":
            p3, R, t = _box4(rng), P.rodrigues_vec_to_mat(rng.normal(size=3)), _rand_t(rng)
        elif name == "face_on":
            p3, R = _box4(rng), _axis_rotation(int(rng.integers(3)), int(rng.integers(4)))
            t = np.array([0.0, 0.0, rng.uniform(0.6, 1.0)])
        elif name == "theta_pi":
            fixed = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, 0), (1, -1, 1)]
            R = _rot_pi(fixed[i] if i < len(fixed) else rng.normal(size=3))
            p3, t = (_box4(rng) if i % 2 else rng.uniform(-0.1, 0.1, (4, 3))), _rand_t(rng)
        elif name == "identity":
            R, p3, t = np.eye(3), (_box4(rng) if i % 2 else rng.uniform(-0.1, 0.1, (4, 3))), _rand_t(rng)
        else:
            R, t = P.rodrigues_vec_to_mat(rng.normal(size=3)), _rand_t(rng)
            c = int(rng.integers(8))
            if i % 2 == 0:    # corner, centre, opposite corner + a fourth point off the line
                p3 = np.stack([box[c], box[8], box[7 - c], box[(c + 1) % 8]])
                p3 = p3[[list(o) + [3] for o in P.P3P_ORDERS][(i // 2) % 3]]
            elif i % 4 == 1:  # a repeated point: b2 == 0 in the first order
                p3 = np.stack([box[c], box[(c + 3) % 8], box[c], box[8]])
            else:             # a repeated point in the other position
                p3 = np.stack([box[c], box[c], box[(c + 3) % 8], box[8]])
        p3s.append(p3)
        Rs.append(R)
        ts.append(t)
    p3s, Rs, ts = np.array(p3s), np.array(Rs), np.array(ts)
    p2 = np.stack([project(Rs[i], ts[i], p3s[i], K) for i in range(n)])
    return dict(p3=p3s, p2=p2, R=Rs, t=ts)


@functools.lru_cache(maxsize=None)
def collinear5():
    """The ``collinear`` scenes with a fifth point of lower weight in front: the four
    highest keys are points 1..4, the P3P has no pose, and the LM starts from the zero
    pose, where the box centre projects to 0 / 0.  -> dict(p3 [n, 5, 3], p2, w [n, 5, 3])."""
    f = p3p_family("collinear")
    n = f["p3"].shape[0]
    extra = box_keypoints()[np.arange(n) % 8][:, None]
    p3 = np.concatenate([extra, f["p3"]], 1)
    p2 = np.stack([project(f["R"][i], f["t"][i], p3[i], K) for i in range(n)])
    w = np.tile(UNIT_W, (n, 5, 1))
    w[:, 0] *= 0.5
    return dict(p3=p3, p2=p2, w=w)


def equilateral_scene(seed):
    """The documented limit: an equilateral triangle seen from its own axis (fails in
    every order, the 3-fold symmetry)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi) + np.arange(3) * 2 * np.pi / 3
    p3 = np.concatenate([0.08 * np.stack([np.cos(a), np.sin(a), np.zeros(3)], 1), rng.uniform(-0.1, 0.1, (1, 3))])
    t = np.array([0.0, 0.0, rng.uniform(0.6, 1.0)])
    return p3, project(np.eye(3), t, p3, K)


# ----------------------------------------------------------------------------
# selection scenes
# ----------------------------------------------------------------------------
def _cov(rng):
    a = rng.normal(size=(2, 2))
    return (a @ a.T + 0.05 * np.eye(2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def selection_scenes():
    """-> list of dict(name, mode, p3 [9, 3], p2 [9, 2] f64, wgt, expect): ``wgt`` is [9, 3] f64
    weights or [9, 2, 2] f32 covariances; ``expect`` the four selected indices in order."""
    out = []
    box = box_keypoints()
    for s in range(4):
        rng = np.random.default_rng(200 + s)
        R, t = P.rodrigues_vec_to_mat(rng.normal(size=3)), _rand_t(rng)
        p2 = project(R, t, box, K) + rng.uniform(-3.0, 3.0, (9, 2))

        def weights(keys):
            return np.asarray(keys, np.float64)[:, None] * UNIT_W

        out.append(dict(name="all_equal", mode="weights", wgt=weights([1.0] * 9), expect=[5, 6, 7, 8]))
        # ascending, ties by index: 1 7 | 2 3 4 5 | 0 8 6 -- the group of 2s ends at the cut (rank 5)
        out.append(dict(name="tie_straddles_cut", mode="weights", wgt=weights([3, 1, 2, 2, 2, 2, 5, 1, 4]),
                        expect=[5, 0, 8, 6]))
        k = np.arange(1.0, 10.0)
        k[[2, 6]] = np.nan      # NaN sorts last: ... 7 8 | 2 6
        out.append(dict(name="nan_weights", mode="weights", wgt=weights(k), expect=[7, 8, 2, 6]))
        for mode in ("cov", "cov_v2"):
            cov = np.stack([_cov(rng) for _ in range(9)])
            live = [int(v) for v in rng.permutation(9)[:2]]
            for i in range(9):
                if i not in live:
                    cov[i] = np.float32(1e-7) * np.eye(2, dtype=np.float32)
            w = P.weights_from_cov(cov) if mode == "cov" else P.weights_v2(cov)
            key = w[:, 0] + w[:, 1] if mode == "cov" else w[:, 0]
            gated = [i for i in range(9) if i not in live]
            out.append(dict(name=f"{mode}_gated", mode=mode, wgt=cov,
                            expect=gated[-2:] + sorted(live, key=lambda i: key[i])))
        # cov_v2: a NaN C[0,0] is gated (zero weight), here on the point with the largest weight
        cov = np.stack([_cov(rng) for _ in range(9)])
        w = P.weights_v2(cov)[:, 0]
        top = int(np.argmax(w))
        cov[top, 0, 0] = np.nan
        w[top] = 0.0
        out.append(dict(name="cov_v2_nan_c00", mode="cov_v2", wgt=cov,
                        expect=[int(i) for i in np.argsort(w, kind="stable")[-4:]]))
        # cov_v2: a NaN anywhere else is a NaN weight (sorts last, poisons the cost)
        cov = np.stack([_cov(rng) for _ in range(9)])
        w = P.weights_v2(cov)[:, 0]
        cov[4, 1, 1] = np.nan
        rest = [int(i) for i in np.argsort(w, kind="stable") if i != 4]
        out.append(dict(name="cov_v2_nan_c11", mode="cov_v2", wgt=cov, expect=rest[-3:] + [4]))
        for d in out[-7:]:
            d.update(p3=box, p2=p2, seed=s)
    return out


def selection_oracle(sc):
    """-> (Rt, diag) of the oracle on one selection scene."""
    d = {}
    if sc["mode"] == "weights":
        Rt = P.uncertainty_pnp(sc["p2"], sc["wgt"], sc["p3"], K, diag=d)
    elif sc["mode"] == "cov":
        Rt = P.uncertainty_pnp(sc["p2"], P.weights_from_cov(sc["wgt"]), sc["p3"], K, diag=d)
    else:
        Rt = P.uncertainty_pnp_v2(sc["p2"], sc["wgt"], sc["p3"], K, diag=d)
    return Rt, d


# ----------------------------------------------------------------------------
# LM scenes
# ----------------------------------------------------------------------------
def _model(pn, rng):
    """Model points: the box for pn <= 9, else random points in +-0.1 m with the origin first."""
    if pn <= 9:
        return box_keypoints()[[8] + [int(i) for i in rng.permutation(8)[:pn - 1]]]
    p = rng.uniform(-0.1, 0.1, (pn, 3))
    p[0] = 0.0
    return p


# (kind, pn) -> seeds, where not 0..3.
# far_overflow: the seeds of far_scene(pn, seed, overflow=True) whose oracle trace holds a rejected
# step, a non-finite candidate cost and a radius growth (far_search; 1,500 draws at pn 5 and 6 give
# 26 and 31 such scenes, 152 draws at pn 63 and 150 at pn 64 give 4 each).
# far: seed 56 at pn 5 and 66 at pn 6 run out of iterations (MAX_ITER at 50) on a path that rounding
# does not move (max_iter_search: of 18 such scenes in 500 draws each, these and three more keep their
# cost to 1e-11 when the image points move by 16 ulp; the others wander, up to 20 % in the cost).
# full_noisy at pn 64: seed 1's four points make a near-double root of the quartic, its start moves
# by 1e-5 between root finders.
SEEDS = {("far_overflow", 5): (87, 214, 355, 413), ("far_overflow", 6): (16, 55, 64, 71),
         ("far_overflow", 63): (100, 132, 139, 151), ("far_overflow", 64): (55, 80, 112, 135),
         ("far", 5): (0, 1, 2, 56), ("far", 6): (0, 1, 2, 66), ("full_noisy", 64): (0, 2, 3, 4)}

LM_KINDS = ("zero_weights", "zero_weights_full", "exact", "parameter", "identity", "far", "far_overflow",
            "nonfinite", "full_noisy")
# the status each kind is built to end in (absent: whatever the oracle says)
LM_EXPECT = {"zero_weights": "gradient", "zero_weights_full": "gradient", "exact": "gradient",
             "parameter": "parameter", "nonfinite": "max_iterations"}
# kinds whose data are exact: their last decisions are taken on residuals of 1e-9 px and less
EXACT_KINDS = ("exact", "parameter", "identity")
N_PER = 4


def far_scene(pn, seed, overflow=False):
    """A start far from the solution: rvec off by 1-2 rad, t off by 0.5 m, image noise of 1 px.

    A trial step that takes a point through z = 0 gives a huge but finite cost, so a non-finite
    candidate cost needs an overflow: with ``overflow`` the weights are scaled until the largest
    diagonal entry of J^T J at the start is 1e306 (weights of ~1e150; the start's cost and every sum
    of the solver stay finite, a candidate whose residuals are some 40 times the start's does not)."""
    rng = np.random.default_rng([300, pn, seed])
    p3 = _model(pn, rng)
    rv, t = rng.normal(size=3), _rand_t(rng)
    rv *= rng.uniform(0.3, 2.5) / np.linalg.norm(rv)
    p2 = project(P.rodrigues_vec_to_mat(rv), t, p3, K) + rng.normal(0, 1.0, (pn, 2))
    dr = rng.normal(size=3)
    dr *= rng.uniform(1.0, 2.0) / np.linalg.norm(dr)
    dt = rng.normal(size=3)
    dt *= 0.5 / np.linalg.norm(dt)
    w = rng.uniform(0.5, 2.0, pn)[:, None] * UNIT_W
    x0 = np.concatenate([rv + dr, t + dt])
    if overflow:
        _, _, J = P.evaluate(x0, p2, p3, w, K)
        w = w * np.sqrt(1e306 / (J * J).sum(0).max())
    return dict(kind="far_overflow" if overflow else "far", pn=pn, p3=p3, p2=p2, w=w, x0=x0, seed=seed)


def far_properties(d):
    """(a rejected step, a non-finite candidate cost, a radius growth) in the oracle's trace."""
    tr = d["trace"]
    return (any(r["chol_ok"] and not r["accepted"] for r in tr), any(r["cand_finite"] is False for r in tr),
            any(r["grew"] for r in tr))


def lm_scene(kind, pn, seed):
    """One LM scene: dict(kind, pn, p3, p2, w [pn, 3], x0 [6] or None (the full entry), seed)."""
    if kind in ("far", "far_overflow"):
        return far_scene(pn, seed, kind == "far_overflow")
    rng = np.random.default_rng([400 + LM_KINDS.index(kind), pn, seed])
    p3 = _model(pn, rng)
    rv, t = rng.normal(size=3), _rand_t(rng)
    rv *= rng.uniform(0.3, 2.5) / np.linalg.norm(rv)
    if kind == "identity":
        rv = np.zeros(3)
    R = P.rodrigues_vec_to_mat(rv)
    p2 = project(R, t, p3, K)
    x0 = np.concatenate([rv, t])
    if kind in ("zero_weights", "zero_weights_full"):
        p2 = p2 + rng.normal(0, 1.0, (pn, 2))
        w = np.zeros((pn, 3))
        x0 = x0 + rng.uniform(-0.05, 0.05, 6) if kind == "zero_weights" else None
    elif kind == "exact":
        # small weights: the noise of the gradient (residuals of a few ulp of 600 px) stays far below
        # the gradient tolerance, so the stop at iteration 0 does not hang on either side's rounding
        w = rng.uniform(0.005, 0.02, pn)[:, None] * UNIT_W
    elif kind == "parameter":
        # data off by 1e-9 px (10^4 times either side's rounding) under large weights: the gradient is
        # far above its tolerance and the step it asks for (~1e-12) far below the parameter tolerance
        p2 = p2 + rng.uniform(-1e-9, 1e-9, (pn, 2))
        w = rng.uniform(500.0, 2000.0, pn)[:, None] * UNIT_W
    elif kind == "identity":
        w = rng.uniform(0.005, 0.02, pn)[:, None] * UNIT_W
        x0 = np.concatenate([np.zeros(3), t + rng.uniform(-0.01, 0.01, 3)])
    elif kind == "nonfinite":
        p2 = p2 + rng.normal(0, 1.0, (pn, 2))
        w = np.tile(UNIT_W, (pn, 1))
        x0 = np.zeros(6)          # the zero pose: the model's origin projects to 0 / 0
    else:
        p2 = p2 + rng.normal(0, 1.0, (pn, 2))
        cov = np.stack([_cov(rng) for _ in range(pn)])
        w = P.weights_from_cov(cov)
        x0 = None
    return dict(kind=kind, pn=pn, p3=p3, p2=p2, w=w, x0=x0, seed=seed)


def lm_oracle(sc):
    """-> (x [6] or Rt [3, 4], diag) of the oracle on one LM scene."""
    d = {}
    if sc["x0"] is not None:
        out = P.ceres_lm(sc["x0"], sc["p2"], sc["p3"], sc["w"], K, diag=d)
    else:
        out = P.uncertainty_pnp(sc["p2"], sc["w"], sc["p3"], K, diag=d)
    return out, d


@functools.lru_cache(maxsize=None)
def lm_scenes(kind):
    """-> list of (scene, oracle result, oracle diag) for one kind, N_PER scenes per pn."""
    out = []
    for pn in LM_PNS:
        seeds = SEEDS.get((kind, pn), range(N_PER))
        for s in seeds:
            sc = lm_scene(kind, pn, s)
            out.append((sc,) + lm_oracle(sc))
    return out


def cost_floor(sc, cost):
    """What the rounding of the projection can move a scene's cost by.  With exact data the final
    residuals are 1e-9 px and less, down to pure rounding, and no relative tolerance on the cost
    can hold between two implementations of sin, cos and the summation.

    The projection fx X / Z + px of a point at X / Z <= 0.5, Z ~ 0.8 m: the rotation's entries
    carry ~4 eps each, so X, Z (sums of three products of |p| <= 0.17 m and t) ~1.5 eps, the
    quotient ~2.5 eps, times fx = 572: ~1400 eps = 3 ulp of 640 px, one more for the sums; two
    sides, rounded up to a power of two: e = 16 ulp of the largest image coordinate, times the
    largest weight.  The error vector of the 2 pn residuals has norm E <= sqrt(2 pn) e, and
    |0.5 |r + d|^2 - 0.5 |r|^2| <= |r| E + E^2 / 2 with |r| = sqrt(2 cost).  For a noisy scene
    (cost ~ pn) this adds ~1e-11 relative, a hundredth of the relative tolerance."""
    e = 16 * np.spacing(np.abs(sc["p2"]).max()) * np.abs(sc["w"]).max()
    E = np.sqrt(2 * sc["pn"]) * e
    with np.errstate(over="ignore"):
        return float(np.sqrt(2 * cost) * E + 0.5 * E * E) if np.isfinite(cost) else 0.0


def far_search(pn, want=N_PER, draws=400):
    """Seeds of far_scene(pn, ., overflow=True) whose oracle run shows all of far_properties with
    margin >= 1e-6."""
    found = []
    for s in range(draws):
        _, d = lm_oracle(far_scene(pn, s, True))
        if all(far_properties(d)) and d["margin"] >= 1e-6:
            found.append(s)
            if len(found) == want:
                break
    return found


def rounding_spread(sc, d, trials=3):
    """Move every image point by the rounding of a projection (16 ulp of the largest coordinate,
    cost_floor) and run the oracle again: -> (the same status and iterations every time, the largest
    relative change of a finite non-zero cost)."""
    rng = np.random.default_rng(sc["seed"])
    same, worst = True, 0.0
    for _ in range(trials):
        moved = dict(sc, p2=sc["p2"] + rng.uniform(-1, 1, sc["p2"].shape) * 16 * np.spacing(np.abs(sc["p2"]).max()))
        _, dm = lm_oracle(moved)
        same &= (dm["status"], dm["iterations"]) == (d["status"], d["iterations"])
        if np.isfinite(d["cost"]) and d["cost"] > 0:
            worst = max(worst, abs(dm["cost"] - d["cost"]) / d["cost"])
    return same, worst


def max_iter_search(pn, draws=500):
    """Seeds of far_scene(pn, .) that run out of iterations, with their rounding_spread."""
    out = []
    for s in range(draws):
        sc = far_scene(pn, s)
        _, d = lm_oracle(sc)
        if d["status"] == "max_iterations":
            out.append((s,) + rounding_spread(sc, d))
    return out


def radius_search(draws=3000):
    """A bounded search for a scene that stops by RADIUS (or fails a Cholesky factorisation):
    far starts at pn 5 with weights over 12 decades.  -> (radius seeds, cholesky-failure seeds)."""
    rad, chol = [], []
    for s in range(draws):
        sc = far_scene(5, 10_000 + s)
        sc["w"] = sc["w"] * 10.0 ** np.random.default_rng(s).uniform(-6, 6)
        _, d = lm_oracle(sc)
        if d["status"] == "radius":
            rad.append(s)
        if any(not r["chol_ok"] for r in d["trace"]):
            chol.append(s)
    return rad, chol


# ----------------------------------------------------------------------------
# the 64 images of tests/test_gpu_pnp.py::test_full_pnp_matches_oracle
# ----------------------------------------------------------------------------
FULL_SEEDS = tuple(range(64))


@functools.lru_cache(maxsize=None)
def full_batch(mode):
    """-> (p2 f32 [64, 9, 2], cov f32 [64, 9, 2, 2], p3 [9, 3], [(Rt, diag)] of the oracle):
    noisy_case(seed) for FULL_SEEDS with one gated and one NaN covariance."""
    cases = [noisy_case(s) for s in FULL_SEEDS]
    p2 = np.stack([c[0] for c in cases])
    cov = np.stack([c[1] for c in cases])
    p3 = box_keypoints()
    cov[3, 2] = np.float32(1e-7) * np.eye(2, dtype=np.float32)     # gated -> zero weight
    cov[5, 4, 1, 0] = np.nan                                          # NaN -> zero weight (mode cov)
    if mode == "cov_v2":
        cov[5, 4, 1, 0] = 0.0
    refs = []
    for i in range(len(cases)):
        d = {}
        if mode == "cov":
            ref = P.uncertainty_pnp(p2[i], P.weights_from_cov(cov[i]), p3, K, diag=d)
        else:
            ref = P.uncertainty_pnp_v2(p2[i], cov[i], p3, K, diag=d)
        refs.append((ref, d))
    return p2, cov, p3, refs
