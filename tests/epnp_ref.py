"""EPnP in numpy -- the checker of libpvpose.so's pv_epnp (include/pvpose.h), TEST INFRASTRUCTURE ONLY.

OpenCV's ``modules/calib3d/src/epnp.cpp`` (Lepetit, Moreno-Noguer, Fua: "EPnP: An Accurate
O(n) Solution to the PnP Problem", IJCV 2009) restated step by step in float64 with LAPACK
(``eigh``, ``lstsq``, ``svd``).  The symmetric eigen solver is injectable so that the tests can
run the same steps through a solver of another family (tests/test_epnp_ref.py).

This project's conventions on top of cv2's steps (include/pvpose.h states them):

* each PCA axis of the control points is signed so that its largest-magnitude component is
  positive, ties to the lowest index (``sign=+1``; ``-1`` flips the convention, ``0`` keeps
  whatever the eigen solver returned);
* a candidate whose camera-frame points are coplanar or collinear (smallest singular value of
  the Arun/Horn matrix <= 1e-10 of the largest) has no rotation: its error is +inf;
* degenerate inputs give status DEGENERATE, Rt = [I | 0] and rt6 = 0: a model whose smallest
  PCA eigenvalue is <= 1e-12 of its largest, a chosen candidate whose error is not finite,
  or a final pose with a non-finite value.
"""
import numpy as np

from oracle.pnp import rodrigues_mat_to_vec

OK, DEGENERATE = 0, 1
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
PLANAR_RATIO = 1e-12
RANK_RATIO = 1e-10


def eigh_lapack(A):
    return np.linalg.eigh(A)


def control_points(p3, eigh=eigh_lapack, sign=+1):
    """Step 1 -> (cws [4, 3], PCA eigenvalues descending [3])."""
    pn = p3.shape[0]
    c0 = p3.sum(0) / pn
    d = p3 - c0
    w, U = eigh(d.T @ d)
    w, U = w[::-1], U[:, ::-1]
    cws = np.empty((4, 3))
    cws[0] = c0
    for i in range(3):
        u = U[:, i].copy()
        if sign != 0:
            k = int(np.argmax(np.abs(u)))
            if u[k] * sign < 0:
                u = -u
        cws[i + 1] = c0 + np.sqrt(max(w[i], 0.0) / pn) * u
    return cws, w


def barycentric(p3, cws):
    """Step 2 -> alphas [pn, 4]."""
    CC = (cws[1:] - cws[0]).T
    a = (np.linalg.inv(CC) @ (p3 - cws[0]).T).T
    return np.concatenate([1.0 - a.sum(1, keepdims=True), a], 1)


def build_M(alphas, p2, K):
    """Step 3 -> M [2 pn, 12]."""
    fu, fv, uc, vc = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    pn = alphas.shape[0]
    M = np.zeros((2 * pn, 12))
    for j in range(4):
        M[0::2, 3 * j] = alphas[:, j] * fu
        M[0::2, 3 * j + 2] = alphas[:, j] * (uc - p2[:, 0])
        M[1::2, 3 * j + 1] = alphas[:, j] * fv
        M[1::2, 3 * j + 2] = alphas[:, j] * (vc - p2[:, 1])
    return M


def build_L_rho(v, cws):
    """Step 4: v [4, 12] (v[0] the smallest eigenvalue's vector) -> L [6, 10], rho [6]."""
    L = np.empty((6, 10))
    rho = np.empty(6)
    for r, (a, b) in enumerate(PAIRS):
        dv = v[:, 3 * a:3 * a + 3] - v[:, 3 * b:3 * b + 3]
        g = dv @ dv.T
        L[r] = (g[0, 0], 2 * g[0, 1], g[1, 1], 2 * g[0, 2], 2 * g[1, 2], g[2, 2],
                2 * g[0, 3], 2 * g[1, 3], 2 * g[2, 3], g[3, 3])
        dc = cws[a] - cws[b]
        rho[r] = dc @ dc
    return L, rho


def _lstsq(A, b):
    return np.linalg.lstsq(A, b, rcond=None)[0]


def _trace_start(n, x):
    """The sign and zero rules of step 5 on the solution x of start n, and each rule's distance from its
    threshold (zero) relative to max |x|.  N = 1 has the sign of x[0] only."""
    with np.errstate(all="ignore"):
        sc = float(np.abs(x).max())
        rel = (lambda v: float(abs(v) / sc)) if sc > 0 and np.isfinite(sc) else (lambda v: 0.0)
        t = dict(x0_neg=bool(x[0] < 0), x0_margin=rel(x[0]), x2_zero=None, x2_margin=None, x1_neg=None, x1_margin=None)
        if n > 1:
            t.update(x2_zero=not bool(x[2] < 0 if x[0] < 0 else x[2] > 0), x2_margin=min(rel(x[0]), rel(x[2])),
                     x1_neg=bool(x[1] < 0), x1_margin=rel(x[1]))
    return t


def betas_approx(n, L, rho, trace=None):
    """Step 5: cv2's find_betas_approx_1/2/3.  `trace` (a dict) receives _trace_start's record."""
    with np.errstate(all="ignore"):
        be = np.zeros(4)
        if n == 1:
            x = _lstsq(L[:, [0, 1, 3, 6]], rho)
            if trace is not None:
                trace.update(_trace_start(n, x))
            be[0] = np.sqrt(abs(x[0]))
            s = -1.0 if x[0] < 0 else 1.0
            be[1:] = s * x[1:] / be[0]
            return be
        x = _lstsq(L[:, :3] if n == 2 else L[:, :5], rho)
        if trace is not None:
            trace.update(_trace_start(n, x))
        be[0] = np.sqrt(abs(x[0]))
        if x[0] < 0:
            be[1] = np.sqrt(-x[2]) if x[2] < 0 else 0.0
        else:
            be[1] = np.sqrt(x[2]) if x[2] > 0 else 0.0
        if x[1] < 0:
            be[0] = -be[0]
        if n == 3:
            be[2] = x[3] / be[0]
        return be


def gauss_newton(L, rho, be, iters=5):
    """Step 6: cv2's gauss_newton, five iterations on the 6x4 system."""
    be = be.copy()
    with np.errstate(all="ignore"):
        for _ in range(iters):
            b0, b1, b2, b3 = be
            A = np.stack([2 * L[:, 0] * b0 + L[:, 1] * b1 + L[:, 3] * b2 + L[:, 6] * b3,
                          L[:, 1] * b0 + 2 * L[:, 2] * b1 + L[:, 4] * b2 + L[:, 7] * b3,
                          L[:, 3] * b0 + L[:, 4] * b1 + 2 * L[:, 5] * b2 + L[:, 8] * b3,
                          L[:, 6] * b0 + L[:, 7] * b1 + L[:, 8] * b2 + 2 * L[:, 9] * b3], 1)
            r = rho - (L[:, 0] * b0 * b0 + L[:, 1] * b0 * b1 + L[:, 2] * b1 * b1 + L[:, 3] * b0 * b2 +
                       L[:, 4] * b1 * b2 + L[:, 5] * b2 * b2 + L[:, 6] * b0 * b3 + L[:, 7] * b1 * b3 +
                       L[:, 8] * b2 * b3 + L[:, 9] * b3 * b3)
            if not (np.isfinite(A).all() and np.isfinite(r).all()):
                return np.full(4, np.nan)
            be = be + _lstsq(A, r)
    return be


def candidate_pose(be, v, alphas, p3, p2, K, trace=None):
    """Step 7 -> (R, t, mean reprojection error in px).  `trace` (a dict) receives the candidate's
    decisions, each with its distance from the threshold: `negated` (point 0 behind the camera;
    |z of point 0| over the largest |coordinate| of the cloud), `rank_reject` (|s2 - 1e-10 s0| over
    1e-10 s0) and `det_flip` (|det R|, which is 1 for any R that passed the rank gate)."""
    nanpose = (np.full((3, 3), np.nan), np.full(3, np.nan))
    if trace is not None:
        trace.update(negated=None, z0_margin=None, rank_reject=None, rank_margin=None, det_flip=None, det_margin=None)
    if not np.isfinite(be).all():
        return (*nanpose, np.nan)
    with np.errstate(all="ignore"):
        ccs = (be @ v).reshape(4, 3)
        pcs = alphas @ ccs
        if trace is not None:
            trace.update(negated=bool(pcs[0, 2] < 0), z0_margin=float(abs(pcs[0, 2]) / np.abs(pcs).max()))
        if pcs[0, 2] < 0:
            ccs, pcs = -ccs, -pcs
        pn = p3.shape[0]
        pc0, pw0 = pcs.sum(0) / pn, p3.sum(0) / pn
        ABt = (pcs - pc0).T @ (p3 - pw0)
        if not np.isfinite(ABt).all():
            return (*nanpose, np.nan)
        U, s, Vt = np.linalg.svd(ABt)
        if trace is not None:
            trace.update(rank_reject=not bool(s[2] > RANK_RATIO * s[0]),
                         rank_margin=float(abs(s[2] - RANK_RATIO * s[0]) / (RANK_RATIO * s[0])) if s[0] > 0 else 0.0)
        if not s[2] > RANK_RATIO * s[0]:
            return (*nanpose, np.inf)
        R = U @ Vt
        if trace is not None:
            trace.update(det_flip=bool(np.linalg.det(R) < 0), det_margin=float(abs(np.linalg.det(R))))
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        t = pc0 - R @ pw0
        X = p3 @ R.T + t
        ue = K[0, 2] + K[0, 0] * X[:, 0] / X[:, 2]
        ve = K[1, 2] + K[1, 1] * X[:, 1] / X[:, 2]
        err = np.sqrt((p2[:, 0] - ue) ** 2 + (p2[:, 1] - ve) ** 2).sum() / pn
    return R, t, err


def select(cand_err):
    """Step 8: cv2's strict rule -> N in {1, 2, 3}; a tie (or a NaN) keeps the lower N."""
    n = 1
    if cand_err[1] < cand_err[0]:
        n = 2
    if cand_err[2] < cand_err[n - 1]:
        n = 3
    return n


def _degenerate(n_used=1, cand_err=None):
    return dict(Rt=np.concatenate([np.eye(3), np.zeros((3, 1))], 1), rt6=np.zeros(6), status=DEGENERATE,
                n_used=n_used, cand_err=np.full(3, np.nan) if cand_err is None else cand_err)


def epnp(p3, p2, K, eigh=eigh_lapack, sign=+1, trace=None):
    """points_3d [pn, 3], points_2d [pn, 2], K [3, 3] -> dict(Rt [3, 4], rt6 [6], status, n_used, cand_err [3]).

    `trace`, a dict, is filled with this image's decisions (the results do not depend on it):
    "pca" (the eigenvalues, descending), "starts" and "cands" (one dict per N = 1, 2, 3, see
    _trace_start and candidate_pose; empty when the image is degenerate before step 5), "n_used",
    "cand_err" and "select_margin" (second-best minus best candidate error)."""
    p3 = np.asarray(p3, np.float64)
    p2 = np.asarray(p2, np.float64)
    K = np.asarray(K, np.float64)
    assert p3.shape[0] == p2.shape[0] >= 6
    cws, w = control_points(p3, eigh, sign)
    if trace is not None:
        trace.update(pca=w.copy(), starts=[], cands=[], n_used=1, cand_err=np.full(3, np.nan), select_margin=np.nan)
    if not w[2] > PLANAR_RATIO * w[0]:
        return _degenerate()
    alphas = barycentric(p3, cws)
    M = build_M(alphas, p2, K)
    with np.errstate(all="ignore"):
        MtM = M.T @ M
    if not np.isfinite(MtM).all():
        return _degenerate()
    _, V = eigh(MtM)
    v = V[:, :4].T.copy()
    L, rho = build_L_rho(v, cws)
    cands, errs = [], np.empty(3)
    for n in (1, 2, 3):
        ts, tc = (None, None) if trace is None else ({}, {})
        be = gauss_newton(L, rho, betas_approx(n, L, rho, ts))
        R, t, e = candidate_pose(be, v, alphas, p3, p2, K, tc)
        cands.append((R, t))
        errs[n - 1] = e
        if trace is not None:
            trace["starts"].append(ts)
            trace["cands"].append(tc)
    n = select(errs)
    if trace is not None:
        with np.errstate(all="ignore"):
            srt = np.sort(errs)
            trace.update(n_used=n, cand_err=errs.copy(), select_margin=float(srt[1] - srt[0]))
    R, t = cands[n - 1]
    if not (np.isfinite(errs[n - 1]) and np.isfinite(R).all() and np.isfinite(t).all()):
        return _degenerate(n, errs)
    rt6 = np.concatenate([rodrigues_mat_to_vec(R), t])
    if not np.isfinite(rt6).all():
        return _degenerate(n, errs)
    return dict(Rt=np.concatenate([R, t[:, None]], 1), rt6=rt6, status=OK, n_used=n, cand_err=errs)


# ---------------------------------------------------------------- synthetic cases (shared by the tests)
def cuboid_model(half=(0.06, 0.04, 0.025)):
    """8 corners + centre of a cuboid with distinct half-extents (a cube's PCA axes are arbitrary)."""
    h = np.asarray(half, np.float64)
    c = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h
    return np.concatenate([c, np.zeros((1, 3))])


def pca_gaps_ok(p3, ratio=0.1):
    """Adjacent PCA eigenvalues differ by more than `ratio` of the larger: the control axes are well defined."""
    d = p3 - p3.mean(0)
    w = np.linalg.eigvalsh(d.T @ d)[::-1]
    return bool(w[0] - w[1] > ratio * w[0] and w[1] - w[2] > ratio * w[1] and w[2] > ratio * 0.1 * w[0])


def random_model(rng, pn, half=(0.06, 0.04, 0.025)):
    """pn random points in an anisotropic box, redrawn until the PCA eigenvalues are well separated."""
    for _ in range(1000):
        p3 = rng.uniform(-1.0, 1.0, (pn, 3)) * np.asarray(half)
        if pca_gaps_ok(p3):
            return p3
    raise AssertionError("no model with separated PCA eigenvalues")


def random_pose(rng, max_angle=3.0):
    from oracle.pnp import rodrigues_vec_to_mat
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    R = rodrigues_vec_to_mat(ax * rng.uniform(0.0, max_angle))
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.5, 1.2)])
    return np.concatenate([R, t[:, None]], 1)


def project(Rt, p3, K):
    X = p3 @ Rt[:, :3].T + Rt[:, 3]
    return np.stack([K[0, 2] + K[0, 0] * X[:, 0] / X[:, 2], K[1, 2] + K[1, 1] * X[:, 1] / X[:, 2]], 1)
