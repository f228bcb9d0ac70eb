"""numpy float64 restatement of include/pvicp.h (the definition the device is held to): every sum and
product written out with the header's parentheses, rule by rule.  Nothing here is fast.

* :func:`pixel_terms`  rules 1-3 for one pose: the used mask, the 28 terms per pixel, and which rule
                       rejected every other pixel
* :func:`ordered_sums` rule 4: the 28 sums in the header's order
* :func:`solve_step`   rules 5-6: damping, the written-out Cholesky, the step limit
* :func:`cayley`       rule 7's matrix
* :func:`iterate`      one ``pv_icp_iterate`` call on a batch, in place like the device
* :func:`refine`       the render + iterate loop of ``pvnet_amd.icp.refine_depth`` over tests/render_ref.py
"""
import numpy as np

RUNNING, CONVERGED, FEW, NOT_PD, BAD_INPUT = 0, 1, 2, 3, 4
NSUM, RUN, LANES, BLOCK = 28, 4, 256, 1024
# why a pixel was not used, in the order the rules are listed (the first that applies)
REJECT = ("used", "border", "ze", "neighbour", "edge", "zt", "l2", "dist")


def _ok32(z):
    z = np.asarray(z, np.float32)
    return np.isfinite(z) & (z > 0)


def pixel_terms(ze_map, zt_map, K, dist_max, edge_max):
    """ze_map, zt_map f32 [H, W] -> dict(used bool [H, W], T f64 [H, W, 28] (+0 where unused), why i8
    [H, W]: an index into REJECT, n f64 [H, W, 3], P f64 [H, W, 3], e f64 [H, W])."""
    ze32 = np.asarray(ze_map, np.float32)
    zt32 = np.asarray(zt_map, np.float32)
    H, W = ze32.shape
    K = np.asarray(K, np.float64)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    why = np.zeros((H, W), np.int8)
    T = np.zeros((H, W, NSUM))
    nrm = np.zeros((H, W, 3))
    Pm = np.zeros((H, W, 3))
    em = np.zeros((H, W))
    why[:] = 1
    if H < 3 or W < 3:
        return dict(used=why == 0, T=T, why=why, n=nrm, P=Pm, e=em)
    ys, xs = np.mgrid[1:H - 1, 1:W - 1]
    c = (slice(1, H - 1), slice(1, W - 1))
    zef, zlf, zrf = ze32[c], ze32[1:H - 1, 0:W - 2], ze32[1:H - 1, 2:W]
    zuf, zdf, ztf = ze32[0:H - 2, 1:W - 1], ze32[2:H, 1:W - 1], zt32[c]
    with np.errstate(all="ignore"):
        ze, zl, zr, zu, zd, zt = (a.astype(np.float64) for a in (zef, zlf, zrf, zuf, zdf, ztf))
        x, y = xs.astype(np.float64), ys.astype(np.float64)
        xc, xl, xr = x - cx, (x - 1.0) - cx, (x + 1.0) - cx
        ay, ayu, ayd = (y - cy) / fy, ((y - 1.0) - cy) / fy, ((y + 1.0) - cy) / fy
        ax, axl, axr = (xc - s * ay) / fx, (xl - s * ay) / fx, (xr - s * ay) / fx
        axu, axd = (xc - s * ayu) / fx, (xc - s * ayd) / fx
        P0, P1, P2 = ze * ax, ze * ay, ze
        du0, du1, du2 = zr * axr - zl * axl, zr * ay - zl * ay, zr - zl
        dv0, dv1, dv2 = zd * axd - zu * axu, zd * ayd - zu * ayu, zd - zu
        m0, m1, m2 = du1 * dv2 - du2 * dv1, du2 * dv0 - du0 * dv2, du0 * dv1 - du1 * dv0
        l2 = (m0 * m0 + m1 * m1) + m2 * m2
        d0, d1, d2 = P0 - zt * ax, P1 - zt * ay, P2 - zt
        dd = (d0 * d0 + d1 * d1) + d2 * d2
        r = np.sqrt(l2)
        n0, n1, n2 = m0 / r, m1 / r, m2 / r
        e = (n0 * d0 + n1 * d1) + n2 * d2
        c0, c1, c2 = P1 * n2 - P2 * n1, P2 * n0 - P0 * n2, P0 * n1 - P1 * n0
        w = np.zeros(ze.shape, np.int8)
        conds = [_ok32(zef), _ok32(zlf) & _ok32(zrf) & _ok32(zuf) & _ok32(zdf),
                 (np.abs(zl - ze) <= edge_max) & (np.abs(zr - ze) <= edge_max) & (np.abs(zu - ze) <= edge_max) &
                 (np.abs(zd - ze) <= edge_max),
                 _ok32(ztf), np.isfinite(l2) & (l2 > 0), dd <= dist_max * dist_max]
        for code, ok in reversed(list(zip(range(2, 8), conds))):
            w[~ok] = code                                              # the first failing rule wins
        used = w == 0
        J = [c0, c1, c2, n0, n1, n2]
        terms = [J[k] * J[l] for k in range(6) for l in range(k, 6)] + [J[k] * e for k in range(6)] + [e * e]
    why[c] = w
    for q, t in enumerate(terms):
        T[c + (q,)] = np.where(used, t, 0.0)
    for k, (nk, Pk) in enumerate(zip((n0, n1, n2), (P0, P1, P2))):
        nrm[c + (k,)] = np.where(used, nk, 0.0)
        Pm[c + (k,)] = np.where(used, Pk, 0.0)
    em[c] = np.where(used, e, 0.0)
    return dict(used=why == 0, T=T, why=why, n=nrm, P=Pm, e=em)


def ordered_sums(T):
    """T f64 [H, W, 28] -> f64 [28] in rule 4's order."""
    T = np.asarray(T, np.float64)
    npix = T.shape[0] * T.shape[1]
    nblk = -(-npix // BLOCK)
    flat = np.zeros((nblk * BLOCK, NSUM))
    flat[:npix] = T.reshape(npix, NSUM)
    Lv = flat.reshape(nblk, 4, 64, RUN, NSUM)                           # block, wave, lane, run
    lane = np.zeros((nblk, 4, 64, NSUM))
    for j in range(RUN):
        lane = lane + Lv[:, :, :, j]
    for o in (32, 16, 8, 4, 2, 1):
        lane = lane.copy()
        lane[:, :, :o] = lane[:, :, :o] + lane[:, :, o:2 * o]
    S = lane[:, :, 0]
    B = ((S[:, 0] + S[:, 1]) + S[:, 2]) + S[:, 3]
    total = np.zeros(NSUM)
    for k in range(nblk):
        total = total + B[k]
    return total


def unpack(neq):
    """f64 [28] -> (A [6, 6] symmetric, g [6], E)."""
    A = np.zeros((6, 6))
    q = 0
    for k in range(6):
        for l in range(k, 6):
            A[k, l] = A[l, k] = neq[q]
            q += 1
    return A, np.array(neq[21:27], np.float64), float(neq[27])


def chol_solve(M, g):
    """Rule 5's factorisation and the two substitutions -> (y with M y = g, ok)."""
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i + 1):
                s = np.float64(M[i, j])
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                if i == j:
                    if not (np.isfinite(s) and s > 0):
                        return None, False
                    L[i, i] = np.sqrt(s)
                else:
                    L[i, j] = s / L[j, j]
        z = np.zeros(6)
        for i in range(6):
            s = np.float64(g[i])
            for k in range(i):
                s = s - L[i, k] * z[k]
            z[i] = s / L[i, i]
        y = np.zeros(6)
        for i in range(5, -1, -1):
            s = z[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * y[k]
            y[i] = s / L[i, i]
    return y, bool(np.isfinite(y).all())


def solve_step(neq, lam, max_rot, max_trans):
    """-> (ok, w, v, rn, tn, k)."""
    A, g, _ = unpack(neq)
    M = A.copy()
    for k in range(6):
        M[k, k] = A[k, k] + np.float64(lam) * A[k, k]
    y, ok = chol_solve(M, g)
    if not ok:
        return False, None, None, np.nan, np.nan, np.nan
    xi = -y
    w, v = xi[:3], xi[3:]
    rn = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    tn = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    k = np.float64(1.0)
    if rn > max_rot:
        k = np.float64(max_rot) / rn
    if tn > max_trans and np.float64(max_trans) / tn < k:
        k = np.float64(max_trans) / tn
    return True, w, v, rn, tn, k


def cayley(w, k=1.0):
    """Rule 7's C for the rotation step k w."""
    k = np.float64(k)
    a = [(k * np.float64(w[i])) * 0.5 for i in range(3)]
    q = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    den, om = 1.0 + q, 1.0 - q
    b = [2.0 * a[i] for i in range(3)]
    C = np.zeros((3, 3))
    C[0, 0] = (om + b[0] * a[0]) / den
    C[0, 1] = (b[0] * a[1] - b[2]) / den
    C[0, 2] = (b[0] * a[2] + b[1]) / den
    C[1, 0] = (b[1] * a[0] + b[2]) / den
    C[1, 1] = (om + b[1] * a[1]) / den
    C[1, 2] = (b[1] * a[2] - b[0]) / den
    C[2, 0] = (b[2] * a[0] - b[1]) / den
    C[2, 1] = (b[2] * a[1] + b[0]) / den
    C[2, 2] = (om + b[2] * a[2]) / den
    return C


def apply_step(pose, w, v, k):
    """Rule 7 -> the new [3, 4] pose."""
    C = cayley(w, k)
    P = np.asarray(pose, np.float64)
    out = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            out[r, c] = (C[r, 0] * P[0, c] + C[r, 1] * P[1, c]) + C[r, 2] * P[2, c]
        out[r, 3] = ((C[r, 0] * P[0, 3] + C[r, 1] * P[1, 3]) + C[r, 2] * P[2, 3]) + np.float64(k) * v[r]
    return out


def new_state(poses):
    """The state a first call starts from: (pose copy, status, iters, cnt, stats, neq)."""
    b = len(poses)
    return dict(pose=np.array(poses, np.float64).reshape(b, 3, 4).copy(), status=np.zeros(b, np.int32),
                iters=np.zeros(b, np.int32), cnt=np.zeros(b, np.int32), stats=np.zeros((b, 3)), neq=np.zeros((b, NSUM)))


def iterate(state, depth_est, depth_test, K, img_id=None, dist_max=0.02, edge_max=0.01, lam=1e-6, min_count=30,
            max_rot=0.2, max_trans=0.05, eps_rot=1e-5, eps_trans=1e-5, detail=None):
    """One ``pv_icp_iterate`` call, in place on `state` (:func:`new_state`).  depth_est f32 [b, H, W],
    depth_test f32 [n_img, H, W], K [3, 3] or [b, 3, 3].  detail: optional list that receives each
    evaluated pose's :func:`pixel_terms` dict (None for a skipped or bad one)."""
    K = np.asarray(K, np.float64)
    b = len(state["pose"])
    n_img = len(depth_test)
    for i in range(b):
        info = None
        try:
            if state["status"][i] == CONVERGED:
                continue
            Ki = K if K.ndim == 2 else K[i]
            cam = np.array([Ki[0, 0], Ki[0, 1], Ki[0, 2], Ki[1, 1], Ki[1, 2]])
            img = i if img_id is None else int(img_id[i])
            if not (0 <= img < n_img) or not np.isfinite(state["pose"][i]).all() or not np.isfinite(cam).all() or \
                    cam[0] == 0 or cam[3] == 0:
                state["status"][i], state["cnt"][i] = BAD_INPUT, 0
                state["stats"][i], state["neq"][i] = np.nan, np.nan
                continue
            info = pixel_terms(depth_est[i], depth_test[img], Ki, dist_max, edge_max)
            neq = ordered_sums(info["T"])
            cnt = int(info["used"].sum())
            state["neq"][i], state["cnt"][i] = neq, cnt
            with np.errstate(all="ignore"):
                rms = np.sqrt(neq[27] / np.float64(cnt)) if cnt > 0 else np.nan
            if cnt < min_count:
                state["status"][i], state["stats"][i] = FEW, (rms, np.nan, np.nan)
                continue
            ok, w, v, rn, tn, k = solve_step(neq, lam, max_rot, max_trans)
            if not ok:
                state["status"][i], state["stats"][i] = NOT_PD, (rms, np.nan, np.nan)
                continue
            state["pose"][i] = apply_step(state["pose"][i], w, v, k)
            state["iters"][i] += 1
            state["stats"][i] = (rms, rn, tn)
            state["status"][i] = CONVERGED if (rn <= eps_rot and tn <= eps_trans) else RUNNING
        finally:
            if detail is not None:
                detail.append(info)
    return state


def render_depth(models, model_id, poses, K, H, W, znear=1e-3):
    """Each pose alone in its own frame through tests/render_ref.py -> f32 [b, H, W]."""
    from tests import render_ref as RR
    K = np.asarray(K, np.float64)
    out = np.full((len(poses), H, W), np.inf, np.float32)
    for i, P in enumerate(poses):
        mid = 0 if model_id is None else int(model_id[i])
        out[i] = RR.render(models, [(mid, 1, P)], K if K.ndim == 2 else K[i], H, W, znear)["depth"]
    return out


def refine(models, poses, model_id, depth, K, img_id=None, iters=8, znear=1e-3, **kw):
    """The reference chain: render each pose, iterate, `iters` times -> the final state."""
    state = new_state(poses)
    H, W = depth.shape[1:]
    for _ in range(int(iters)):
        de = render_depth(models, model_id, state["pose"], K, H, W, znear)
        iterate(state, de, depth, K, img_id, **kw)
    return state
