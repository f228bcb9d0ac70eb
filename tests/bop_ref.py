"""numpy restatement of include/pvbop.h (the definition the device is held to): MSSD, MSPD and VSD
in float64, every sum and product written out in the header's order, no ``@``, ``einsum`` or BLAS
call, so every operation rounds once and the device can equal it bit for bit.  Also the symmetry
table of ``pvnet_amd.bop.SymmetryTable`` restated independently, and the small shapes the BOP tests
share.  Nothing here is fast.

* :func:`sym_pose`      one (pose, symmetry): G_s, A_s, c_s
* :func:`sym_errors`    err f64 [b, 2], best i32 [b, 2] over a table of models and symmetries
* :func:`vsd`           counts i64 [b, 2 + ntau], err f64 [b, ntau]
* :func:`symmetries`    BOP's get_symmetry_transformations for one models_info entry
* :func:`cube`, :func:`plate`, :func:`cup`, :func:`cube_rotations`, :func:`plate_rotations`
"""
import math

import numpy as np

BIG = 2.0 ** 300
NAN = float("nan")


def _mat3(M, x, y, z):
    """rows of M [3, 4] applied to the columns x, y, z: ((M0 x + M1 y) + M2 z) + M3"""
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]


def sym_pose(Pe, Pg, S):
    """-> (G [3, 4], A|c [3, 4]) of the header for the estimate Pe, the ground truth Pg and the symmetry S."""
    G = np.empty((3, 4))
    D = np.empty((3, 4))
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                G[r, c] = (Pg[r, 0] * S[0, c] + Pg[r, 1] * S[1, c]) + Pg[r, 2] * S[2, c]
                D[r, c] = Pe[r, c] - G[r, c]
            G[r, 3] = ((Pg[r, 0] * S[0, 3] + Pg[r, 1] * S[1, 3]) + Pg[r, 2] * S[2, 3]) + Pg[r, 3]
            D[r, 3] = Pe[r, 3] - G[r, 3]
    return G, D


def project(M, K, x, y, z):
    X, Y, Z = _mat3(M, x, y, z)
    u = (K[0, 0] * X + K[0, 1] * Y) / Z + K[0, 2]
    v = (K[1, 1] * Y) / Z + K[1, 2]
    return u, v, Z


def sym_errors(models, syms, pose_est, pose_gt, K, model_id=None, metrics=("mssd", "mspd"), max_pn=None, max_ns=None,
               err=None, best=None):
    """models: list of f32 [pn, 3]; syms: list of f64 [ns, 3, 4]; pose_est, pose_gt f64 [b, 3, 4];
    K [3, 3] or [b, 3, 3].  err / best: arrays to write into (an unrequested column stays)."""
    Pe = np.asarray(pose_est, np.float64)
    Pg = np.asarray(pose_gt, np.float64)
    K = np.asarray(K, np.float64)
    b = Pe.shape[0]
    err = np.full((b, 2), -7.0) if err is None else err
    best = np.full((b, 2), -7, np.int32) if best is None else best
    max_pn = max(len(m) for m in models) if max_pn is None else max_pn
    max_ns = max(len(s) for s in syms) if max_ns is None else max_ns
    want = [m in metrics for m in ("mssd", "mspd")]
    for i in range(b):
        Ki = K if K.ndim == 2 else K[i]
        mid = 0 if model_id is None else int(model_id[i])
        ok = np.isfinite(Pe[i]).all() and np.isfinite(Pg[i]).all() and 0 <= mid < len(models)
        if ok:
            P = np.asarray(models[mid], np.float32).astype(np.float64).reshape(-1, 3)
            S = np.asarray(syms[mid], np.float64).reshape(-1, 3, 4)
            ok = 1 <= len(P) <= max_pn and 1 <= len(S) <= max_ns and np.isfinite(S).all()
        kok = all(np.isfinite(Ki[r, c]) for r, c in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2)))
        col = [None, None]
        if ok:
            x, y, z = P[:, 0], P[:, 1], P[:, 2]
            Ds, Ps = [], []
            with np.errstate(all="ignore"):
                if want[1]:
                    ue, ve, Ze = project(Pe[i], Ki, x, y, z)
                for s in range(len(S)):
                    G, D = sym_pose(Pe[i], Pg[i], S[s])
                    if want[0]:
                        if not (np.abs(D) < BIG).all():
                            Ds.append(np.inf)
                        else:
                            e0, e1, e2 = _mat3(D, x, y, z)
                            Ds.append(np.max((e0 * e0 + e1 * e1) + e2 * e2))
                    if want[1]:
                        ug, vg, Zg = project(G, Ki, x, y, z)
                        du, dv = ue - ug, ve - vg
                        d2 = du * du + dv * dv
                        d2 = np.where((Ze > 0) & (Zg > 0) & np.isfinite(d2), d2, np.inf)
                        Ps.append(np.max(d2))
            for c, vals in enumerate((Ds, Ps)):
                if want[c]:
                    k = int(np.argmin(vals))                          # the first minimum
                    col[c] = (math.sqrt(vals[k]), k)
        for c in range(2):
            if want[c]:
                good = ok and (c == 0 or kok)
                err[i, c], best[i, c] = col[c] if good else (NAN, -1)
    return err, best


def valid_depth(z):
    return np.isfinite(z) & (z > 0)


def vsd(depth_test, depth_est, depth_gt, K, delta, taus, img_id=None, drop_gt_clause=False):
    """depth_test f32 [n_img, H, W], depth_est / depth_gt f32 [b, H, W], K [3, 3] or [b, 3, 3],
    taus f64 [b, ntau] -> (counts i64 [b, 2 + ntau], err f64 [b, ntau]).
    drop_gt_clause deletes the `or vis_gt` of vis_est: only for the test that shows it matters."""
    dT = np.asarray(depth_test, np.float32)
    dE = np.asarray(depth_est, np.float32)
    dG = np.asarray(depth_gt, np.float32)
    K = np.asarray(K, np.float64)
    taus = np.asarray(taus, np.float64)
    b, H, W = dE.shape
    ntau = taus.shape[1]
    counts = np.zeros((b, 2 + ntau), np.int64)
    err = np.zeros((b, ntau))
    xs = np.arange(W, dtype=np.float64)[None, :]
    ys = np.arange(H, dtype=np.float64)[:, None]
    for i in range(b):
        Ki = K if K.ndim == 2 else K[i]
        j = i if img_id is None else int(img_id[i])
        fx, fy, cx, cy = Ki[0, 0], Ki[1, 1], Ki[0, 2], Ki[1, 2]
        if not (0 <= j < dT.shape[0]) or not all(np.isfinite(v) for v in (fx, fy, cx, cy)):
            counts[i], err[i] = -1, NAN
            continue
        with np.errstate(all="ignore"):
            ax, ay = (xs - cx) / fx, (ys - cy) / fy
            r = np.sqrt((ax * ax + ay * ay) + 1.0)
            zt, ze, zg = dT[j].astype(np.float64), dE[i].astype(np.float64), dG[i].astype(np.float64)
            dt, de, dg = zt * r, ze * r, zg * r
            t_ok, e_ok, g_ok = valid_depth(zt), valid_depth(ze), valid_depth(zg)
            vis_gt = g_ok & (~t_ok | (dg - dt <= delta))
            vis_est = e_ok & (~t_ok | (de - dt <= delta) | (vis_gt & (not drop_gt_clause)))
            un, it = vis_gt | vis_est, vis_gt & vis_est
            diff = np.abs(dg - de)
            counts[i, 0], counts[i, 1] = un.sum(), it.sum()
            for k in range(ntau):
                counts[i, 2 + k] = (it & (diff >= taus[i, k])).sum()
        u = int(counts[i, 0])
        for k in range(ntau):
            err[i, k] = float(int(counts[i, 2 + k]) + (u - int(counts[i, 1]))) / float(u) if u > 0 else 1.0
    return counts, err


# ---- the symmetry table, restated --------------------------------------------------------------------
def axis_rotation(axis, angle):
    """Rodrigues' formula about the unit vector along `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    c, s = math.cos(angle), math.sin(angle)
    x, y, z = a
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def _mm(A, B):
    """A [3, 3] times B [3, n], written out."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return np.array([[(A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c] for c in range(B.shape[1])]
                     for r in range(3)])


def symmetries(info, max_sym_disc_step=0.01):
    """One models_info entry -> f64 [ns, 3, 4]: the identity, the discrete transformations, and each
    of those composed with every step of every continuous symmetry (BOP's get_symmetry_transformations)."""
    disc = [np.eye(4)[:3]]
    for m in info.get("symmetries_discrete", ()):
        disc.append(np.asarray(m, np.float64).reshape(4, 4)[:3])
    cont = []
    n = int(math.ceil(math.pi / max_sym_disc_step))
    for sym in info.get("symmetries_continuous", ()):
        off = np.asarray(sym["offset"], np.float64).reshape(3)
        for k in range(1, n):
            R = axis_rotation(sym["axis"], 2.0 * math.pi * k / n)
            cont.append(np.concatenate([R, off.reshape(3, 1) - _mm(R, off.reshape(3, 1))], 1))
    out = []
    for d in disc:
        out.append(d)
        for c in cont:
            out.append(np.concatenate([_mm(d[:, :3], c[:, :3]), _mm(d[:, :3], c[:, 3:]) + d[:, 3:]], 1))
    return np.stack(out)


# ---- shapes --------------------------------------------------------------------------------------------
def cube(h=0.04, n=3):
    """The n^3 lattice points on the surface of a cube of half-edge h: invariant under its 24 rotations."""
    g = np.linspace(-h, h, n)
    p = np.array([(x, y, z) for x in g for y in g for z in g if max(abs(x), abs(y), abs(z)) == h])
    return p.astype(np.float32)


def plate(h=0.05, t=0.01, n=5):
    """A square plate (thin along z): invariant under the 8 rotations of the dihedral group D4."""
    g = np.linspace(-h, h, n)
    return np.array([(x, y, z) for x in g for y in g for z in (-t, t)], np.float32)


def cup(n_ring=315, radii=(0.03, 0.04, 0.025), heights=(-0.04, 0.0, 0.05)):
    """Rings about the z axis with n_ring points each: with n_ring = 315 the cloud is invariant
    (up to f32 rounding of the vertices) under a turn by any multiple of 2 pi / 315, and by nothing finer."""
    a = 2.0 * np.pi * np.arange(n_ring) / n_ring
    return np.concatenate([np.stack([r * np.cos(a), r * np.sin(a), np.full_like(a, h)], 1)
                           for r, h in zip(radii, heights)]).astype(np.float32)


def _signed_perms(det=1):
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sg in ((a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)):
            R = np.zeros((3, 3))
            for r in range(3):
                R[r, perm[r]] = sg[r]
            if round(np.linalg.det(R)) == det:
                out.append(R)
    return out


def cube_rotations():
    """The 24 proper rotations of the cube, the identity first."""
    rs = _signed_perms()
    rs.sort(key=lambda R: not np.array_equal(R, np.eye(3)))
    return rs


def plate_rotations():
    """The 8 proper rotations that keep a square plate thin along z, the identity first."""
    return [R for R in cube_rotations() if abs(R[2, 2]) == 1]


def as_info(rotations):
    """models_info's symmetries_discrete for a list of rotations (the identity left out)."""
    out = []
    for R in rotations:
        if not np.array_equal(R, np.eye(3)):
            M = np.eye(4)
            M[:3, :3] = R
            out.append([float(v) for v in M.reshape(-1)])
    return {"symmetries_discrete": out}
