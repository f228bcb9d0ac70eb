"""numpy restatement of include/pvshade.h in float64 (the definition the device is held to), on
tests/render_ref.py's projection, meshes and pose helpers.  Nothing here is fast.

* :func:`vertex_normals`  pv_shade_normals: area-weighted face sums in face order, normalised
* :func:`render`          one frame: the maps, the face map, the image, and how far each answer is
                          from a decision the device could take the other way: per pixel and channel
                          the *margin* (distance of the value before rounding from the nearest k + 0.5)
                          and per pixel the *contested* flag (another covering face whose f64 depth
                          rounds to the same or an adjacent f32 as the winner's)
* :func:`colored`, :func:`reverse_winding`, :func:`scenes`  what the CPU and the GPU tests share
"""
import numpy as np

from tests import render_ref as R

SUB = R.SUB
INVALID = R.INVALID
HEADLIGHT = np.array([0.0, 0.0, -1.0, 0.3, 0.3, 0.3, 0.7, 0.7, 0.7])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vertex_normals(verts, faces):
    """verts f32 [nv, 3], faces int [nf, 3] -> f64 [nv, 3]; zero where no valid face names the vertex."""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    nv = p.shape[0]
    N = np.zeros((nv, 3))
    for f in np.asarray(faces, np.int64).reshape(-1, 3):
        if f.min() < 0 or f.max() >= nv:
            continue
        c = _cross(p[f[1]] - p[f[0]], p[f[2]] - p[f[0]])
        for v in sorted(set(int(i) for i in f)):                       # a face naming v twice counts once
            N[v] = N[v] + c
    with np.errstate(all="ignore"):
        L = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        out = N / L[:, None]
    out[~((L > 0) & np.isfinite(L))] = 0.0
    return out


def _camera_points(verts, Rt):
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    P = np.asarray(Rt, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)], 1)


def _edge(a, b, X, Y):
    dx, dy = int(b[0]) - int(a[0]), int(b[1]) - int(a[1])
    E = dx * (Y - int(a[1])) - dy * (X - int(a[0]))
    top_left = dy < 0 or (dy == 0 and dx > 0)
    return E, (E > 0) | ((E == 0) & top_left)


def _oriented(sxy, f):
    """The face's indices after the winding swap, or None for a dropped face."""
    nv = sxy.shape[0]
    if f.min() < 0 or f.max() >= nv:
        return None
    i0, i1, i2 = (int(i) for i in f)
    if INVALID in (sxy[i0, 0], sxy[i1, 0], sxy[i2, 0]):
        return None
    p0, p1, p2 = sxy[i0], sxy[i1], sxy[i2]
    area = int(p1[0] - p0[0]) * int(p2[1] - p0[1]) - int(p2[0] - p0[0]) * int(p1[1] - p0[1])
    if area == 0:
        return None
    return (i0, i2, i1) if area < 0 else (i0, i1, i2)


def _ulps(a, b):
    ai, bi = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ai - bi)


def render(models, insts, K, H, W, light=HEADLIGHT, background=(0, 0, 0), znear=1e-3, snapped=None):
    """One frame.  models: list of (verts, faces, colors[, normals or None]); insts: list of
    (model_id, label, Rt [3, 4]); light f64 [9]; background: three integers or u8 [H, W, 3]; snapped:
    optional list, per instance None or (sxy, Z) to rasterise instead of this file's own projection.

    -> dict(label, inst, face i32 [H, W], depth f32 [H, W], won i64 [n], image u8 [H, W, 3],
    margin f64 [H, W, 3] (inf on the background and where the value is clamped whichever way it
    rounds), contested bool [H, W], covered bool [H, W])."""
    light = np.asarray(light, np.float64)
    max_faces = max(len(np.asarray(m[1]).reshape(-1, 3)) for m in models)
    depth = np.full((H, W), np.inf, np.float32)
    slot = np.full((H, W), -1, np.int64)
    cover = []                                                         # (slot, by0, bx0, cov, z32) of every face that covers
    cam = {}
    for j, (mid, lab, Rt) in enumerate(insts):
        Rt = np.asarray(Rt, np.float64)
        if not (0 <= int(mid) < len(models)) or not np.isfinite(Rt).all() or not (1 <= int(lab) <= 255):
            continue
        verts, faces = models[int(mid)][:2]
        if snapped is None or snapped[j] is None:
            s = R.project_snap(verts, Rt, K, znear)
            sxy, Z = s["sxy"], s["Z"]
        else:
            sxy, Z = snapped[j]
        sxy, Z = np.asarray(sxy, np.int64), np.asarray(Z, np.float64)
        P = _camera_points(verts, Rt)
        P[:, 2] = Z
        cam[j] = (sxy, P)
        for fi, f in enumerate(np.asarray(faces, np.int64).reshape(-1, 3)):
            idx = _oriented(sxy, f)
            if idx is None:
                continue
            p0, p1, p2 = sxy[idx[0]], sxy[idx[1]], sxy[idx[2]]
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
            q0, q1, q2 = 1.0 / Z[idx[0]], 1.0 / Z[idx[1]], 1.0 / Z[idx[2]]
            with np.errstate(all="ignore"):
                num = (w0.astype(np.float64) * q0 + w1.astype(np.float64) * q1) + w2.astype(np.float64) * q2
                z32 = (1.0 / (num / (w0 + w1 + w2).astype(np.float64))).astype(np.float32)
            sl = j * max_faces + fi
            cover.append((sl, by0, bx0, cov, z32))
            d, s_ = depth[by0:by1 + 1, bx0:bx1 + 1], slot[by0:by1 + 1, bx0:bx1 + 1]
            better = cov & ((z32 < d) | ((z32 == d) & (sl < s_)))      # the integer minimum over (depth bits, slot)
            d[better] = z32[better]
            s_[better] = sl
    covered = slot >= 0
    contested = np.zeros((H, W), bool)
    for sl, by0, bx0, cov, z32 in cover:
        h, w = cov.shape
        d, s_ = depth[by0:by0 + h, bx0:bx0 + w], slot[by0:by0 + h, bx0:bx0 + w]
        contested[by0:by0 + h, bx0:bx0 + w] |= cov & (s_ != sl) & (_ulps(z32, d) <= 1)
    inst = np.where(covered, slot // max_faces, -1).astype(np.int32)
    face = np.where(covered, slot % max_faces, -1).astype(np.int32)
    label = np.zeros((H, W), np.int32)
    for j, (_, lab, _) in enumerate(insts):
        label[inst == j] = int(lab)
    won = np.array([int(np.count_nonzero(inst == j)) for j in range(len(insts))], np.int64)

    bg = np.asarray(background, np.uint8)
    image = np.broadcast_to(bg, (H, W, 3)).copy()
    margin = np.full((H, W, 3), np.inf)
    l = light[:3]
    for sl in np.unique(slot[covered]):
        j, fi = int(sl // max_faces), int(sl % max_faces)
        mid, _, Rt = insts[j]
        model = models[int(mid)]
        Rt = np.asarray(Rt, np.float64)
        sxy, P = cam[j]
        i0, i1, i2 = _oriented(sxy, np.asarray(model[1], np.int64).reshape(-1, 3)[fi])
        ys, xs = np.nonzero(slot == sl)
        X, Y = xs.astype(np.int64) * SUB, ys.astype(np.int64) * SUB
        w2, _ = _edge(sxy[i0], sxy[i1], X, Y)
        w0, _ = _edge(sxy[i1], sxy[i2], X, Y)
        w1, _ = _edge(sxy[i2], sxy[i0], X, Y)
        with np.errstate(all="ignore"):
            a0, a1, a2 = (w.astype(np.float64) * (1.0 / P[i, 2]) for w, i in ((w0, i0), (w1, i1), (w2, i2)))
            s = (a0 + a1) + a2
            b0, b1, b2 = a0 / s, a1 / s, a2 / s
            nf = _cross(P[i1] - P[i0], P[i2] - P[i0])
            if _dot(nf, P[i0]) > 0:
                nf = -nf
            n = np.broadcast_to(nf, (len(xs), 3)).copy()
            normals = model[3] if len(model) > 3 else None
            if normals is not None:
                nn = np.asarray(normals, np.float64).reshape(-1, 3)
                nm = (b0[:, None] * nn[i0] + b1[:, None] * nn[i1]) + b2[:, None] * nn[i2]
                rot = np.stack([(Rt[r, 0] * nm[:, 0] + Rt[r, 1] * nm[:, 1]) + Rt[r, 2] * nm[:, 2] for r in range(3)], 1)
                rot[_dot(rot, nf) < 0] *= -1.0
                use = ~((nm[:, 0] == 0) & (nm[:, 1] == 0) & (nm[:, 2] == 0))
                n[use] = rot[use]
            ln, ll = np.sqrt(_dot(n, n)), np.sqrt(_dot(l, l))
            cos = _dot(n, l) / (ln * ll)
            d = np.where(cos > 0, cos, 0.0)
            d[~((ln > 0) & np.isfinite(ln))] = 0.0
            if not (ll > 0 and np.isfinite(ll)):
                d[:] = 0.0
            col = np.asarray(model[2], np.uint8).reshape(-1, 3).astype(np.float64)
            for k in range(3):
                c = (b0 * col[i0, k] + b1 * col[i1, k]) + b2 * col[i2, k]
                v = c * (light[3 + k] + light[6 + k] * d)
                r = np.rint(v)
                image[ys, xs, k] = np.where(np.isnan(r) | (r < 0), 0, np.minimum(r, 255)).astype(np.uint8)
                m = np.abs((v - np.floor(v)) - 0.5)
                m[np.isnan(v) | (v > 256) | (v < -1)] = np.inf
                margin[ys, xs, k] = m
    return dict(label=label, inst=inst, face=face, depth=depth, won=won, image=image, margin=margin, contested=contested,
                covered=covered)


# ---- what the CPU and the GPU tests share ----------------------------------------------------------
K_SMALL = np.array([[70.0, 0.0, 31.5], [0.0, 71.5, 23.5], [0.0, 0.0, 1.0]])
K_SKEW = np.array([[40.0, 0.7, 26.1], [0.0, 41.0, 18.2], [0.0, 0.0, 1.0]])
LIGHT_A = np.array([0.3, -0.5, -0.8, 0.37, 0.33, 0.41, 0.58, 0.61, 0.53])
LIGHT_B = np.array([-0.6, 0.2, -0.7, 0.29, 0.37, 0.31, 0.66, 0.58, 0.62])


def colored(mesh, seed, smooth=False):
    """(verts, faces) -> (verts, faces, random u8 colours in 16..239, normals or None)."""
    v, f = mesh
    c = np.random.default_rng(seed).integers(16, 240, size=(len(v), 3)).astype(np.uint8)
    return v, f, c, vertex_normals(v, f) if smooth else None


def reverse_winding(model):
    return (model[0], np.ascontiguousarray(np.asarray(model[1])[:, ::-1]), *model[2:])


def seeded_poses(seed, n, spread=0.03, near=0.3, far=0.5):
    rng = np.random.default_rng(seed)
    return [R.pose(R.random_rotation(rng), [rng.uniform(-spread, spread), rng.uniform(-spread, spread),
                                            rng.uniform(near, far)]) for _ in range(n)]


def base_meshes():
    return [R.box(), R.icosphere(2, 0.05), R.bumpy_ellipsoid(2), R.icosphere(3, 0.05)]


def models(smooth):
    return [colored(m, 40 + i, smooth) for i, m in enumerate(base_meshes())]


def occlusion_frames():
    """Two and three instances per frame with real occlusion (tests/test_gpu_render.py's)."""
    I = np.eye(3)
    rot = seeded_poses(21, 3)
    two = [[(1, 1, R.pose(I, [-0.01, 0.0, 0.40])), (0, 2, R.pose(rot[0][:, :3], [0.02, 0.01, 0.33]))],
           [(1, 3, R.pose(I, [-0.015, 0.0, 0.40])), (3, 4, R.pose(rot[1][:, :3], [0.02, 0.01, 0.42]))]]
    three = [[(1, 1, R.pose(I, [-0.03, 0.0, 0.40])), (3, 2, R.pose(rot[2][:, :3], [0.03, 0.0, 0.43])),
              (2, 3, R.pose(rot[0][:, :3], [0.0, 0.01, 0.36]))],
             [(2, 7, R.pose(rot[1][:, :3], [0.0, -0.035, 0.45])), (0, 8, R.pose(rot[2][:, :3], [0.04, 0.0, 0.38])),
              (1, 9, R.pose(I, [-0.035, 0.01, 0.41]))]]
    return two, three


def scenes():
    """name -> dict(smooth, frames, K, H, W, lights [b, 9] or [9], background): every scene whose image
    the GPU tests compare with :func:`render`.  tests/test_shade_ref.py asserts on each that every
    margin is at least 1e-9 and that at most 1 % of the covered pixels are contested."""
    two, three = occlusion_frames()
    single = [[(3, 1, p)] for p in seeded_poses(7, 2, near=0.18, far=0.3)] + [[(2, 2, p)] for p in seeded_poses(8, 2)]
    rng = np.random.default_rng(5)
    bg = rng.integers(0, 256, size=(2, 37, 53, 3)).astype(np.uint8)
    behind = np.array([0.0, 0.0, 1.0, 0.37, 0.33, 0.41, 0.58, 0.61, 0.53])       # from behind every visible surface
    dark = np.array([0.0, 0.0, 0.0, 0.37, 0.33, 0.41, 0.58, 0.61, 0.53])         # no direction at all
    bright = np.array([0.3, -0.5, -0.8, 1.37, 0.33, 2.41, 0.58, 0.61, 0.53])     # ambient above 1: clamps
    out = {}
    for smooth in (False, True):
        tag = "smooth" if smooth else "flat"
        out[f"occlusion2_{tag}"] = dict(smooth=smooth, frames=two, K=K_SMALL, H=48, W=64, lights=LIGHT_A, background=(0, 0, 0))
        out[f"occlusion3_{tag}"] = dict(smooth=smooth, frames=three, K=K_SKEW, H=37, W=53, lights=np.stack([LIGHT_A, LIGHT_B]),
                                        background=bg)
    out["small_triangles_smooth"] = dict(smooth=True, frames=single, K=K_SMALL, H=48, W=64,
                                         lights=np.stack([LIGHT_A, LIGHT_B, behind, dark]), background=(9, 120, 255))
    out["clamp_flat"] = dict(smooth=False, frames=two, K=K_SKEW, H=37, W=53, lights=np.stack([bright, behind]),
                             background=bg[:1])
    return out


def scene_reference(sc, snapped=None):
    """:func:`render` on every frame of a scene -> list of its dicts."""
    ms = models(sc["smooth"])
    refs = []
    for i, f in enumerate(sc["frames"]):
        lights, bg = np.asarray(sc["lights"]), sc["background"]
        light = lights if lights.ndim == 1 else lights[i]
        if isinstance(bg, np.ndarray):
            bg = bg[i if bg.shape[0] > 1 else 0]
        refs.append(render(ms, f, sc["K"], sc["H"], sc["W"], light, bg, snapped=None if snapped is None else snapped[i]))
    return refs
