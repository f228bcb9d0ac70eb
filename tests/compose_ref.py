"""include/pvcompose.h restated in numpy: the yardstick of tests/test_gpu_compose.py, itself pinned to
independent yardsticks by tests/test_compose_ref.py.  Everything is an exact restatement: integers,
uint64, fp64 with every operation rounded, and f32 arrays whose every operation rounds to f32, in the
header's order.  The device's outputs equal these bit for bit."""
import math

import numpy as np

from tests.augment_ref import G, mix

F = np.float32
MAX_SLOTS, MAX_ERASE, MAX_DIM, TILE, DRAW0 = 16, 8, 2 ** 15, 32, 64
U64 = np.uint64


# ---- the draws -------------------------------------------------------------------------------------------
def base_key(seed, n):
    """mix(mix(seed + G) + (n + 1) G) for sample indices n (uint64, wrapping)."""
    with np.errstate(over="ignore"):
        n = np.asarray(n, U64)
        return mix(mix(U64(seed) + G) + (n + U64(1)) * G)


def u(seed, n, k):
    """The draw u(seed, n, k) of pvaugment.h, vectorised over n and k -> f64 in [0, 1)."""
    with np.errstate(over="ignore"):
        z = mix(base_key(seed, n) + (np.asarray(k, U64) + U64(1)) * G)
    return (z >> U64(11)).astype(np.float64) * 2.0 ** -53


# ---- pv_compose_apply ------------------------------------------------------------------------------------
def clipped_box(p, H, W):
    return max(int(p[3]), 0), max(int(p[4]), 0), min(int(p[5]), W - 1), min(int(p[6]), H - 1)


def live(p, N, ncls):
    return 0 <= int(p[0]) < N and 1 <= int(p[2]) <= ncls


def compose(bank_image, bank_label, pick, shift, ncls, Ho, Wo, background=None, fill=(0, 0, 0), erase=None):
    """bank_image u8 [N][H][W][3], bank_label [N][H][W], pick [b][S][8], shift [b][S][2], erase [b][E][4] or
    None -> (image u8 [b][Ho][Wo][3], label [b][Ho][Wo], instance [b][Ho][Wo], visible i32 [b][S]).
    Slots are painted in increasing s, so the highest belonging slot shows.  Python integers throughout:
    nothing overflows."""
    N, H, W = bank_label.shape
    b, S = pick.shape[:2]
    image = np.zeros((b, Ho, Wo, 3), np.uint8)
    label = np.zeros((b, Ho, Wo), bank_label.dtype)
    inst = np.zeros((b, Ho, Wo), bank_label.dtype)
    visible = np.zeros((b, S), np.int32)
    for f in range(b):
        if background is not None:
            image[f] = background[f if background.shape[0] == b else 0]
        else:
            image[f] = np.asarray(fill, np.uint8)
        for s in range(S):
            p = pick[f, s]
            if not live(p, N, ncls):
                continue
            x0, y0, x1, y1 = clipped_box(p, H, W)
            dx, dy = int(shift[f, s, 0]), int(shift[f, s, 1])
            ox0, ox1, oy0, oy1 = max(x0 + dx, 0), min(x1 + dx, Wo - 1), max(y0 + dy, 0), min(y1 + dy, Ho - 1)
            if x0 > x1 or y0 > y1 or ox0 > ox1 or oy0 > oy1:
                continue
            src = int(p[0])
            sl = bank_label[src, oy0 - dy:oy1 - dy + 1, ox0 - dx:ox1 - dx + 1]
            hit = sl.astype(np.int64) == int(p[1])
            image[f, oy0:oy1 + 1, ox0:ox1 + 1][hit] = bank_image[src, oy0 - dy:oy1 - dy + 1, ox0 - dx:ox1 - dx + 1][hit]
            label[f, oy0:oy1 + 1, ox0:ox1 + 1][hit] = int(p[2])
            inst[f, oy0:oy1 + 1, ox0:ox1 + 1][hit] = s + 1
        for e in range(0 if erase is None else erase.shape[1]):
            x0, y0, x1, y1 = (int(v) for v in erase[f, e])
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, Wo - 1), min(y1, Ho - 1)
            if x0 > x1 or y0 > y1:
                continue
            image[f, y0:y1 + 1, x0:x1 + 1] = np.asarray(fill, np.uint8)
            label[f, y0:y1 + 1, x0:x1 + 1] = 0
            inst[f, y0:y1 + 1, x0:x1 + 1] = 0
        for s in range(S):
            visible[f, s] = np.count_nonzero(inst[f] == s + 1)
    return image, label, inst, visible


# ---- pv_compose_params -----------------------------------------------------------------------------------
def params(pick, seed, first, N, H, W, Ho, Wo, ncls, E=0, margin=0.25, erase_frac=(0.1, 0.4), p_blur=0.5, noise=(0.0, 8.0)):
    """-> shift i32 [b][S][2], erase i32 [b][E][4], ksel i32 [b], amp f32 [b]."""
    b, S = pick.shape[:2]
    shift = np.zeros((b, S, 2), np.int32)
    erase = np.zeros((b, E, 4), np.int32)
    ksel = np.zeros(b, np.int32)
    amp = np.zeros(b, np.float32)
    span = 1.0 - 2.0 * margin
    with np.errstate(over="ignore"):
        ns = U64(first) + np.arange(b, dtype=U64)
    for f in range(b):
        n = ns[f]
        boxes = [None] * S
        for s in range(S):
            p = pick[f, s]
            x0, y0, x1, y1 = clipped_box(p, H, W)
            if not live(p, N, ncls) or x0 > x1 or y0 > y1:
                continue
            u0, u1 = (float(u(seed, n, DRAW0 + 8 * s + j)) for j in range(2))
            tx = (margin + u0 * span) * float(Wo - 1)
            ty = (margin + u1 * span) * float(Ho - 1)
            dx = int(np.rint(tx - (float(x0) + float(x1)) / 2.0))
            dy = int(np.rint(ty - (float(y0) + float(y1)) / 2.0))
            shift[f, s] = (dx, dy)
            boxes[s] = (x0, y0, x1, y1, dx, dy)
        for e in range(E):
            box = boxes[e % S]
            if box is None:
                erase[f, e] = (0, 0, -1, -1)
                continue
            x0, y0, x1, y1, dx, dy = box
            bw, bh = x1 - x0 + 1, y1 - y0 + 1
            u0, u1, u2, u3 = (float(u(seed, n, 192 + 8 * e + j)) for j in range(4))
            fw = erase_frac[0] + u0 * (erase_frac[1] - erase_frac[0])
            fh = erase_frac[0] + u1 * (erase_frac[1] - erase_frac[0])
            w = max(1, int(np.rint(fw * float(bw))))
            h = max(1, int(np.rint(fh * float(bh))))
            left = x0 + dx + int(math.floor(u2 * float(bw - w + 1)))
            top = y0 + dy + int(math.floor(u3 * float(bh - h + 1)))
            erase[f, e] = (left, top, left + w - 1, top + h - 1)
        u0, u1, u2 = (float(u(seed, n, 256 + j)) for j in range(3))
        ksel[f] = 1 + min(3, int(math.floor(4.0 * u1))) if u0 < p_blur else 0
        amp[f] = np.float32(noise[0] + u2 * (noise[1] - noise[0]))
    return shift, erase, ksel, amp


# ---- pv_compose_finish -----------------------------------------------------------------------------------
def kernels():
    """f32 [5][5]: w[j][t], the half-kernel of the (2 j + 1)-tap Gaussian with sigma = 0.3 (j - 1) + 0.8,
    normalised in f64, cast to f32."""
    w = np.zeros((5, 5), np.float64)
    for j in range(5):
        sigma = 0.3 * (j - 1) + 0.8
        g = [math.exp(-(t * t) / (2.0 * sigma * sigma)) for t in range(-j, j + 1)]
        total = math.fsum(g)
        for t in range(j + 1):
            w[j, t] = g[j + t] / total
    return w.astype(np.float32)


def reflect(i, n):
    """reflect-101 of the integer array i into 0..n - 1."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def noise_field(seed, n, H, W):
    """-> f32 [H][W][3]: t of the header for sample index n."""
    with np.errstate(over="ignore"):
        key = base_key(seed, n)
        p = np.arange(H * W, dtype=U64).reshape(H, W, 1)
        ch = np.arange(3, dtype=U64).reshape(1, 1, 3)
        z = mix(key + (U64(1 << 40) + U64(3) * p + ch + U64(1)) * G)
    m = U64(0xFFFF)
    s = (z & m) + ((z >> U64(16)) & m) + ((z >> U64(32)) & m) + (z >> U64(48))
    return (s.astype(np.int64) - 131070).astype(F) * F(2.0 ** -16)


def blur_pass(v, w, j, axis):
    """One separable pass in f32 along `axis` of v f32 [H][W][3]."""
    if j == 0:
        return v
    n = v.shape[axis]
    idx = np.arange(n)
    a = w[j, 0] * v
    for t in range(1, j + 1):
        a = a + w[j, t] * (np.take(v, reflect(idx - t, n), axis) + np.take(v, reflect(idx + t, n), axis))
    assert a.dtype == F
    return a


def blurred(image, j, w=None):
    """image u8 [H][W][3] -> f32 [H][W][3]: both passes."""
    w = kernels() if w is None else w
    return blur_pass(blur_pass(image.astype(F), w, j, 1), w, j, 0)


def finish(image, ksel, amp, seed, first, w=None):
    """image u8 [b][H][W][3], ksel i32 [b], amp f32 [b] -> u8 [b][H][W][3]."""
    b, H, W = image.shape[:3]
    out = np.zeros_like(image)
    with np.errstate(over="ignore"):
        ns = U64(first) + np.arange(b, dtype=U64)
    for f in range(b):
        j = int(ksel[f]) if 0 <= int(ksel[f]) <= 4 else 0
        a = blurred(image[f], j, w)
        with np.errstate(invalid="ignore"):
            c = a + F(amp[f]) * noise_field(seed, ns[f], H, W)
            assert c.dtype == F
            out[f] = np.rint(np.fmin(np.fmax(c, F(0)), F(255))).astype(np.uint8)
    return out
