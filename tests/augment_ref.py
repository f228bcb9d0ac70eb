"""include/pvaugment.h restated in numpy: the yardstick of tests/test_gpu_augment.py, itself pinned to
independent yardsticks by tests/test_augment_ref.py.  Geometry and draws are exact restatements (fp64,
uint64); the colour chain is evaluated in f64 from the same f32 inputs (weights, factors, constants),
so the device's f32 result differs from it by its own rounding alone."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
DRAWS = 8
BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 4, 8
ALL = 15
F = np.float32
INV255 = float(F(1.0) / F(255.0))
GREY = tuple(float(F(v)) for v in (0.299, 0.587, 0.114))


# ---- the draws -------------------------------------------------------------------------------------------
def mix(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draws(seed, first, b):
    """-> f64 [b][DRAWS] in [0, 1)."""
    with np.errstate(over="ignore"):
        n = np.uint64(first) + np.arange(b, dtype=np.uint64)
        base = mix(mix(np.uint64(seed) + G) + (n + np.uint64(1)) * G)
        k = np.arange(1, DRAWS + 1, dtype=np.uint64)
        z = mix(base[:, None] + k[None, :] * G)
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def draw_int(seed, n, k):
    """One draw in pure Python integers: the second statement of the generator."""
    M = (1 << 64) - 1

    def m(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    g = 0x9E3779B97F4A7C15
    z = m((m((m((seed + g) & M) + (n + 1) * g) & M) + (k + 1) * g) & M)
    return (z >> 11) * 2.0 ** -53


# ---- statistics and parameters ---------------------------------------------------------------------------
def label_stats(label, ncls):
    label = np.asarray(label)
    b, H, W = label.shape
    out = np.zeros((b, 8), np.int64)
    for i in range(b):
        ys, xs = np.nonzero((label[i] >= 1) & (label[i] <= ncls))
        if len(xs):
            out[i] = (len(xs), xs.sum(), ys.sum(), xs.min(), ys.min(), xs.max(), ys.max(), 0)
        else:
            out[i] = (0, 0, 0, W, H, -1, -1, 0)
    return out


def params(stats, seed, first, H, W, Ho, Wo, rot_deg=(-30.0, 30.0), scale=(0.8, 1.2), margin=0.25,
           jitter=(0.1, 0.1, 0.05, 0.05)):
    """-> fwd f64 [b][2][3], inv f64 [b][2][3], color f32 [b][4], (theta, s, t, c) for the tests."""
    b = stats.shape[0]
    u = draws(seed, first, b)
    theta = (rot_deg[0] + u[:, 0] * (rot_deg[1] - rot_deg[0])) * (3.141592653589793 / 180.0)
    s = scale[0] + u[:, 1] * (scale[1] - scale[0])
    span = 1.0 - 2.0 * margin
    tx = (margin + u[:, 2] * span) * float(Wo - 1)
    ty = (margin + u[:, 3] * span) * float(Ho - 1)
    cnt = stats[:, 0].astype(np.float64)
    has = stats[:, 0] > 0
    safe = np.where(has, cnt, 1.0)
    cx = np.where(has, stats[:, 1].astype(np.float64) / safe, float(W - 1) / 2.0)
    cy = np.where(has, stats[:, 2].astype(np.float64) / safe, float(H - 1) / 2.0)
    a, q = s * np.cos(theta), s * np.sin(theta)
    f02 = tx - (a * cx - q * cy)
    f12 = ty - (q * cx + a * cy)
    fwd = np.stack([np.stack([a, -q, f02], 1), np.stack([q, a, f12], 1)], 1)
    d = a * a + q * q
    ia, iq = a / d, q / d
    inv = np.stack([np.stack([ia, iq, -(ia * f02 + iq * f12)], 1), np.stack([-iq, ia, iq * f02 - ia * f12], 1)], 1)
    j = jitter
    color = np.stack([1.0 + j[0] * (2.0 * u[:, 4] - 1.0), 1.0 + j[1] * (2.0 * u[:, 5] - 1.0),
                      1.0 + j[2] * (2.0 * u[:, 6] - 1.0), j[3] * (2.0 * u[:, 7] - 1.0)], 1).astype(np.float32)
    return fwd, inv, color, dict(theta=theta, s=s, t=np.stack([tx, ty], 1), c=np.stack([cx, cy], 1), u=u)


# ---- the warp --------------------------------------------------------------------------------------------
def source_coords(M, Ho, Wo):
    """M f64 [2][3] -> sx, sy f64 [Ho][Wo], each operation rounded as the header orders them."""
    x = np.arange(Wo, dtype=np.float64)[None, :]
    y = np.arange(Ho, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        sx = (M[0, 0] * x + M[0, 1] * y) + M[0, 2]
        sy = (M[1, 0] * x + M[1, 1] * y) + M[1, 2]
    return sx, sy


def warp_label(label, M, Ho, Wo):
    """label [H][W] -> [Ho][Wo], nearest (ties to even), 0 outside or not finite."""
    H, W = label.shape
    sx, sy = source_coords(M, Ho, Wo)
    with np.errstate(all="ignore"):
        rx, ry = np.rint(sx), np.rint(sy)
        ok = (rx >= 0.0) & (rx <= W - 1) & (ry >= 0.0) & (ry <= H - 1)
    ix = np.where(ok, rx, 0.0).astype(np.int64)
    iy = np.where(ok, ry, 0.0).astype(np.int64)
    return np.where(ok, label[iy, ix], 0).astype(label.dtype)


def warp_image(image, M, Ho, Wo, fill=(0.0, 0.0, 0.0), weights=np.float32):
    """image u8 [H][W][3] -> f64 [Ho][Wo][3] on the 0..255 scale: bilinear, `fill` outside.  The
    weights are the fp64 fractions rounded to `weights`: float32 is the header's; float64 leaves them
    as they are, which is what an f64 yardstick computes (tests/test_augment_ref.py)."""
    H, W = image.shape[:2]
    sx, sy = source_coords(M, Ho, Wo)
    fillv = np.array([float(F(f)) for f in fill])
    with np.errstate(all="ignore"):
        fx, fy = np.floor(sx), np.floor(sy)
        any_in = (fx >= -1.0) & (fx <= W - 1) & (fy >= -1.0) & (fy <= H - 1)
        wx = np.where(any_in, sx - fx, 0.0).astype(weights).astype(np.float64)[..., None]
        wy = np.where(any_in, sy - fy, 0.0).astype(weights).astype(np.float64)[..., None]
    ix = np.where(any_in, fx, 0.0).astype(np.int64)
    iy = np.where(any_in, fy, 0.0).astype(np.int64)

    def tap(dy, dx):
        yy, xx = iy + dy, ix + dx
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        v = image[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64)
        return np.where(ok[..., None], v, fillv)

    v00, v01, v10, v11 = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    top = v00 + wx * (v01 - v00)
    bot = v10 + wx * (v11 - v10)
    c = top + wy * (bot - top)
    return np.where(any_in[..., None], c, fillv)


# ---- the colour chain (f64) ------------------------------------------------------------------------------
def grey(c):
    return (GREY[0] * c[..., 0] + GREY[1] * c[..., 1]) + GREY[2] * c[..., 2]


def clamp(c):
    return np.minimum(np.maximum(c, 0.0), 1.0)


def rgb_to_hsv(c):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = c.max(-1), c.min(-1)
    rng = maxc - minc
    flat = rng == 0
    safe = np.where(flat, 1.0, rng)
    s = np.where(flat, 0.0, rng / np.where(maxc == 0, 1.0, maxc))
    rc, gc, bc = (maxc - r) / safe, (maxc - g) / safe, (maxc - b) / safe
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, (2.0 + rc) - bc, (4.0 + gc) - rc))
    h = h / 6.0
    h = h - np.floor(h)
    return np.where(flat, 0.0, h), s, maxc


def hsv_to_rgb(h, s, v):
    h6 = h * 6.0
    fi = np.floor(h6)
    f = h6 - fi
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    sec = fi.astype(np.int64) % 6
    r = np.choose(sec, [v, q, p, p, t, v])
    g = np.choose(sec, [t, v, v, q, p, p])
    b = np.choose(sec, [p, p, t, v, v, q])
    out = np.stack([r, g, b], -1)
    return np.where((s == 0)[..., None], np.stack([v, v, v], -1), out)


def hue_shift(c, eta):
    h, s, v = rgb_to_hsv(c)
    h = h + eta
    h = h - np.floor(h)
    return hsv_to_rgb(h, s, v)


def photometric(c, color, flags):
    """c f64 [Ho][Wo][3] on [0, 1]; color f32 [4] -> f64 [Ho][Wo][3]."""
    beta, kappa, sigma, eta = (float(v) for v in np.asarray(color, np.float32))
    if flags & BRIGHTNESS:
        c = clamp(beta * c)
    if flags & CONTRAST:
        m = grey(c).mean()
        c = clamp(kappa * c + (1.0 - kappa) * m)
    if flags & SATURATION:
        c = clamp(sigma * c + ((1.0 - sigma) * grey(c))[..., None])
    if flags & HUE:
        c = hue_shift(c, eta)
    return c


def apply(image, label, inv, color, Ho, Wo, background=None, fill=(0.0, 0.0, 0.0), mean=(0.485, 0.456, 0.406),
          std=(0.229, 0.224, 0.225), flags=ALL):
    """image u8 [b][H][W][3], label [b][H][W], inv f64 [b][2][3], color f32 [b][4] ->
    (f64 [b][3][Ho][Wo], label [b][Ho][Wo])."""
    b = image.shape[0]
    mean_v = np.array([float(F(v)) for v in mean])
    rstd_v = np.array([float(F(1.0) / F(v)) for v in std])
    out = np.zeros((b, 3, Ho, Wo))
    lab = np.zeros((b, Ho, Wo), label.dtype)
    for i in range(b):
        lab[i] = warp_label(label[i], inv[i], Ho, Wo)
        c = warp_image(image[i], inv[i], Ho, Wo, fill)
        if background is not None:
            bg = background[i if background.shape[0] == b else 0].astype(np.float64)
            c = np.where((lab[i] == 0)[..., None], bg, c)
        c = photometric(c * INV255, color[i], flags)
        out[i] = ((c - mean_v) * rstd_v).transpose(2, 0, 1)
    return out, lab
