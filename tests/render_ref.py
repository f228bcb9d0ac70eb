"""numpy restatement of include/pvrender.h (the definition the device is held to), and the
procedural meshes the render tests share.  Nothing here is fast and nothing needs a file.

* :func:`project_snap`   fp64 projection and the 1/256 px snap, with the snap margin
* :func:`raster_instance` exact int64 coverage with the top-left rule and the fp64 depth
* :func:`render`         one frame: skip rules, z-buffer with the tie rule, margins, won counts
* :func:`vertex_field`   compute_vertex per class (``synth.gt_vertex_field``)
* :func:`box`, :func:`icosphere`, :func:`bumpy_ellipsoid`, :func:`spread_keypoints`, :func:`random_rotation`
"""
import numpy as np

from pvnet_amd import synth

SUB = 256
MAX_SNAP = 1 << 29
INVALID = -(1 << 31)


def project_snap(verts, Rt, K, znear):
    """verts f32 [n, 3], Rt [3, 4], K [3, 3] -> dict(sxy i32 [n, 2] (INVALID rows drop their
    triangles), Z f64 [n], ok bool [n], margin: the smallest distance of any 256 u, 256 v of an ok
    vertex from a half-integer)."""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    P = np.asarray(Rt, np.float64)
    K = np.asarray(K, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        X = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
        Y = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
        Z = ((P[2, 0] * x + P[2, 1] * y) + P[2, 2] * z) + P[2, 3]
        u = (K[0, 0] * X + K[0, 1] * Y) / Z + K[0, 2]
        v = (K[1, 1] * Y) / Z + K[1, 2]
        tu, tv = u * 256.0, v * 256.0
        su, sv = np.rint(tu), np.rint(tv)
        ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z >= znear) & (np.abs(su) <= MAX_SNAP) & \
            (np.abs(sv) <= MAX_SNAP)
    sxy = np.full((p.shape[0], 2), INVALID, np.int64)
    sxy[ok, 0] = su[ok]
    sxy[ok, 1] = sv[ok]
    margin = np.inf
    if ok.any():
        t = np.concatenate([tu[ok], tv[ok]])
        margin = float(np.min(np.abs((t - np.floor(t)) - 0.5)))
    return dict(sxy=sxy.astype(np.int32), Z=Z, ok=ok, margin=margin)


def _edge(a, b, X, Y):
    dx, dy = int(b[0]) - int(a[0]), int(b[1]) - int(a[1])
    E = dx * (Y - int(a[1])) - dy * (X - int(a[0]))
    top_left = dy < 0 or (dy == 0 and dx > 0)
    return E, (E > 0) | ((E == 0) & top_left)


def raster_instance(sxy, Z, faces, H, W):
    """One instance from its snapped vertices -> dict(depth f32 [H, W] (+inf where nothing covers),
    depth64 (the same winner before rounding), count i32 [H, W]: triangles covering each sample)."""
    sxy = np.asarray(sxy, np.int64)
    Z = np.asarray(Z, np.float64)
    nv = sxy.shape[0]
    depth = np.full((H, W), np.inf, np.float32)
    depth64 = np.full((H, W), np.inf, np.float64)
    count = np.zeros((H, W), np.int32)
    for f in np.asarray(faces, np.int64).reshape(-1, 3):
        if f.min() < 0 or f.max() >= nv:
            continue
        i0, i1, i2 = (int(i) for i in f)
        if INVALID in (sxy[i0, 0], sxy[i1, 0], sxy[i2, 0]):
            continue
        p0, p1, p2 = sxy[i0], sxy[i1], sxy[i2]
        area = int(p1[0] - p0[0]) * int(p2[1] - p0[1]) - int(p2[0] - p0[0]) * int(p1[1] - p0[1])
        if area == 0:
            continue
        if area < 0:
            p1, p2, i1, i2 = p2, p1, i2, i1
        xs, ys = (p0[0], p1[0], p2[0]), (p0[1], p1[1], p2[1])
        bx0, bx1 = max(0, -(-int(min(xs)) // SUB)), min(W - 1, int(max(xs)) // SUB)
        by0, by1 = max(0, -(-int(min(ys)) // SUB)), min(H - 1, int(max(ys)) // SUB)
        if bx0 > bx1 or by0 > by1:
            continue
        Y, X = np.meshgrid(np.arange(by0, by1 + 1, dtype=np.int64) * SUB, np.arange(bx0, bx1 + 1, dtype=np.int64) * SUB,
                           indexing="ij")
        w2, c2 = _edge(p0, p1, X, Y)
        w0, c0 = _edge(p1, p2, X, Y)
        w1, c1 = _edge(p2, p0, X, Y)
        cov = c0 & c1 & c2
        if not cov.any():
            continue
        q0, q1, q2 = 1.0 / Z[i0], 1.0 / Z[i1], 1.0 / Z[i2]
        with np.errstate(all="ignore"):
            num = (w0.astype(np.float64) * q0 + w1.astype(np.float64) * q1) + w2.astype(np.float64) * q2
            Zp = 1.0 / (num / (w0 + w1 + w2).astype(np.float64))
            z32 = Zp.astype(np.float32)
        sub, sub64, cnt = depth[by0:by1 + 1, bx0:bx1 + 1], depth64[by0:by1 + 1, bx0:bx1 + 1], count[by0:by1 + 1, bx0:bx1 + 1]
        cnt += cov
        # f32 bit order, with the fp64 value to break the restatement's own ties the same way every time
        better = cov & ((z32 < sub) | ((z32 == sub) & (Zp < sub64)))
        sub[better] = z32[better]
        sub64[better] = Zp[better]
    return dict(depth=depth, depth64=depth64, count=count)


def render(models, insts, K, H, W, znear=1e-3, snapped=None):
    """One frame.  models: list of (verts, faces); insts: list of (model_id, label, Rt [3, 4]);
    snapped: optional list, per instance None or (sxy, Z) to rasterise instead of this file's own
    projection (the device's snapped vertices: coverage is then exact given them).

    -> dict(label i32 [H, W], inst i32 [H, W], depth f32 [H, W], won i64 [n], snap: per instance
    project_snap's dict or None for a skipped one, snap_margin, depth_margin_map f64 [H, W]: the
    relative gap between the two nearest depths of *different* instances (inf where fewer than two
    cover), depth_margin: its minimum, count: per instance the covering-triangle count map)."""
    label = np.zeros((H, W), np.int32)
    inst = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), np.inf, np.float32)
    snaps, counts, d64 = [], [], []
    snap_margin = np.inf
    for j, (mid, lab, Rt) in enumerate(insts):
        Rt = np.asarray(Rt, np.float64)
        if not (0 <= int(mid) < len(models)) or not np.isfinite(Rt).all() or not (1 <= int(lab) <= 255):
            snaps.append(None)
            counts.append(np.zeros((H, W), np.int32))
            continue
        verts, faces = models[int(mid)]
        s = project_snap(verts, Rt, K, znear)
        snap_margin = min(snap_margin, s["margin"])
        snaps.append(s)
        sxy, Z = (s["sxy"], s["Z"]) if snapped is None or snapped[j] is None else snapped[j]
        r = raster_instance(sxy, Z, faces, H, W)
        counts.append(r["count"])
        d64.append(r["depth64"])
        win = r["depth"] < depth            # strict: equal depths stay with the lower instance index
        label[win], inst[win], depth[win] = int(lab), j, r["depth"][win]
    margin_map = np.full((H, W), np.inf)
    if len(d64) >= 2:
        s = np.sort(np.stack(d64), 0)
        both = np.isfinite(s[1])
        margin_map[both] = (s[1][both] - s[0][both]) / s[0][both]
    won = np.array([int(np.count_nonzero(inst == j)) for j in range(len(insts))], np.int64)
    return dict(label=label, inst=inst, depth=depth, won=won, snap=snaps, snap_margin=float(snap_margin),
                depth_margin_map=margin_map, depth_margin=float(margin_map.min()), count=counts)


def vertex_field(label, keypoints):
    """label int [H, W], keypoints f64 [ncls, vn, 2] -> f32 [H, W, ncls * vn, 2]: compute_vertex
    (``synth.gt_vertex_field``) on ``label == c + 1`` for each class, zero elsewhere."""
    label = np.asarray(label)
    kp = np.asarray(keypoints, np.float64)
    ncls, vn = kp.shape[:2]
    H, W = label.shape
    out = np.zeros((H, W, ncls * vn, 2), np.float32)
    for c in range(ncls):
        out[:, :, c * vn:(c + 1) * vn] = synth.gt_vertex_field((label == c + 1).astype(np.uint8), kp[c]).reshape(H, W, vn, 2)
    return out


# ---- procedural meshes ----------------------------------------------------------------------------
def box(hx=0.05, hy=0.04, hz=0.03):
    """8 vertices, 12 triangles, outward winding."""
    v = np.array([[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float32)
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def icosphere(level=2, radius=0.05):
    """20 * 4^level triangles: level 2 -> 320, 3 -> 1,280, 5 -> 20,480."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def bumpy_ellipsoid(level=3, radii=(0.06, 0.045, 0.035)):
    """An icosphere stretched to an ellipsoid with three unequal bumps and a dent: no symmetry, so
    a silhouette with keypoints determines the pose."""
    v, f = icosphere(level, 1.0)
    d = v.astype(np.float64)
    s = np.ones(d.shape[0])
    for centre, amp, width in (((1, 0.3, 0.2), 0.35, 0.25), ((-0.4, 1, 0.5), 0.25, 0.15), ((0.2, -0.5, 1), 0.3, 0.2),
                               ((-1, -0.6, -0.7), -0.2, 0.3)):
        c = np.array(centre, np.float64)
        c /= np.linalg.norm(c)
        s += amp * np.exp(-np.sum((d - c) ** 2, 1) / width)
    return (d * s[:, None] * np.array(radii)).astype(np.float32), f


def spread_keypoints(verts, n=8):
    """n vertices by farthest-point sampling (from the one farthest from the centroid) and the
    centroid: [n + 1, 3] float64."""
    v = np.asarray(verts, np.float64)
    c = v.mean(0)
    pick = [int(np.argmax(np.sum((v - c) ** 2, 1)))]
    dist = np.sum((v - v[pick[0]]) ** 2, 1)
    while len(pick) < n:
        pick.append(int(np.argmax(dist)))
        dist = np.minimum(dist, np.sum((v - v[pick[-1]]) ** 2, 1))
    return np.concatenate([v[pick], c[None]])


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def pose(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1)
