"""The voting front half's counter RNG (pvnet_amd/csrc/pv_rng.h) and what front_half
(pvpipeline.hip) makes of a call's seed, restated in numpy: uint64 / uint32 arithmetic that
wraps, one float32 step.  tests/test_front_ref.py requires the four functions to equal
pv_rng.h compiled for the host bit for bit; tests/test_gpu_front_half.py then injects
``pairs`` and ``keep_mask`` into a call and requires what the seeded call gives.

Layout (read from front_half, compact_chunk, compact_hyp and item_hyp):
  * hypothesis seed ``mix64(seed)``, keep seed ``mix64(seed ^ 0xd1b54a32d192ed03)``;
  * the pair of (image b, hypothesis h, keypoint v) is ``rand_index(hyp seed, 2 gid, tn[b])``,
    ``rand_index(hyp seed, 2 gid + 1, tn[b])`` with ``gid = (b nh + h) vn + v``;
  * pixel p (row-major) of image b is kept when ``rand_unit(keep seed, b P + p) <
    float32(max_num) / float32(fg[b])``, a float32 comparison; an image with
    ``fg <= max_num`` keeps everything;
  * b is the pipeline's image index: the virtual image ``bi * ncls + c`` of a multi-object call.
"""
import numpy as np

U64 = np.uint64
U32 = np.uint32
F32 = np.float32
KEEP_XOR = 0xd1b54a32d192ed03


def _u64(x):
    if isinstance(x, (int, np.integer)):
        return np.array(int(x) & (2 ** 64 - 1), dtype=U64)
    x = np.asarray(x)
    assert x.dtype == U64, x.dtype
    return x


def mix64(z):
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = z + U64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> U64(30))) * U64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> U64(27))) * U64(0x94d049bb133111eb)
        return z ^ (z >> U64(31))


def hash32(x):
    x = np.asarray(x)
    assert x.dtype == U32, x.dtype
    with np.errstate(over="ignore"):
        x = x ^ (x >> U32(16))
        x = x * U32(0x7feb352d)
        x = x ^ (x >> U32(15))
        x = x * U32(0x846ca68b)
        return x ^ (x >> U32(16))


def _lo(x):
    return (x & U64(0xffffffff)).astype(U32)


def _hi(x):
    return (x >> U64(32)).astype(U32)


def rand_index(seed, key, n):
    """int32 in [0, n): seed, key uint64 (scalars or arrays), n int32 >= 1."""
    seed, key = _u64(seed), _u64(key)
    n = np.asarray(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        r = hash32(hash32(_lo(key) ^ _lo(seed)) + _hi(key) + _hi(seed))
    return ((r.astype(U64) * (n & 0xffffffff).astype(U64)) >> U64(32)).astype(np.int32)


def rand_unit(seed, key):
    """float32 in [0, 1): 24 bits, exact."""
    seed, key = _u64(seed), _u64(key)
    m = mix64(seed ^ mix64(key ^ U64(0x5bd1e995))) >> U64(40)
    return m.astype(F32) * F32(1.0 / 16777216.0)


def seeds(seed):
    """(hypothesis seed, keep seed) of a call with ``_seed=seed``, as Python ints."""
    s = int(seed) & (2 ** 64 - 1)
    return int(mix64(s)), int(mix64(s ^ KEEP_XOR))


def pairs(seed, n_per_image, nh, vn):
    """int32 [b, nh, vn, 2]: the pixel pairs a call with ``_seed=seed`` draws; ``n_per_image[b]``
    is image b's compacted count tn (an image with tn <= 0 draws nothing: zeros)."""
    hs, _ = seeds(seed)
    n = np.asarray(n_per_image, dtype=np.int64).reshape(-1)
    b = n.shape[0]
    gid = np.arange(b * nh * vn, dtype=U64).reshape(b, nh, vn)
    key = np.stack([gid * U64(2), gid * U64(2) + U64(1)], -1)
    out = rand_index(hs, key, np.maximum(n, 1).reshape(b, 1, 1, 1))
    out[n <= 0] = 0
    return out


def keep_mask(seed, fg_mask, max_num):
    """uint8 [b, H, W]: the keep decision of every pixel (the pipeline reads it at the
    foreground only) for a call with ``_seed=seed``; all ones for an image with fg <= max_num."""
    _, ks = seeds(seed)
    fg_mask = np.asarray(fg_mask).astype(bool)
    b, H, W = fg_mask.shape
    P = H * W
    out = np.ones((b, H, W), np.uint8)
    for i in range(b):
        fg = int(fg_mask[i].sum())
        if fg <= max_num:
            continue
        key = np.arange(i * P, (i + 1) * P, dtype=U64)
        pk = F32(max_num) / F32(fg)
        assert pk.dtype == F32
        out[i] = (rand_unit(ks, key) < pk).reshape(H, W)
    return out
