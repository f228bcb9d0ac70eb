"""References and scenes for the stages after the vote (k_refine_solve,
k_point_conf, k_evd_with_mean, k_evd_topk, k_motion_vote) at their edge shapes.

* The CPU oracle (``oracle/oracle.py``) stays the reference for everything
  discrete: tn, hypotheses, counts, winners, v5 confidence counts, the top-k
  set.  For the two EVD reductions this module restates the arithmetic after
  the oracle's own fp32 inputs in float64 (``evd_with_mean_f64``,
  ``evd_topk_f64``) and returns, with each value, the sum of the absolute
  terms that a rounding-error bound scales with.
* The scenes are small frames built from ``synth.synthetic_field``; each one
  exists to put a kernel on one of its edges (``tests/test_tail_refs.py``
  asserts that it does, on the CPU).  Everything here is cached: treat what
  these functions return as read-only.

``tests/test_tail_refs.py`` pins the references against the reference's golden
vectors and the oracle; ``tests/test_gpu_tail_stages.py`` uses them.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from pvnet_amd import synth

F32 = np.float32
U32 = 2.0 ** -24          # unit roundoff of float32
COV_RTOL = 1e-4           # the project's covariance tolerance (tests/test_oracle_golden.py)
KP_TOL = 1e-2

# derived bounds, in units of U32 times the sum of absolute terms (see the
# docstrings of the GPU tests and DESIGN.md "Edge-shape tests of the stages after the vote")
EVD_COV_UNITS = 8
EVD_MEAN_UNITS = 4


# ----------------------------------------------------------------------------
# float64 references of the EVD reductions
# ----------------------------------------------------------------------------
def evd_with_mean_f64(hyp, ratio, mean):
    """RV:394-401 on the oracle's fp32 ``hyp`` [b,vn,hn,2] / ``ratio`` [b,vn,hn]
    (``O._evd_collect``) and ``mean`` [b,vn,2]: the ``ratio < max - 0.1f`` rule
    and ``diff = fl32(hyp - mean)`` in float32 as the reference computes them,
    everything after that in float64.

    Returns (cov f64 [b,vn,2,2], S_abs f64 [b,vn,2,2], kept int [b,vn]) with
    ``S_abs[i,j] = sum_h |d_i d_j| w_h / den`` and ``kept`` the number of
    hypotheses the threshold rule leaves a weight."""
    hyp, ratio, mean = np.asarray(hyp, F32), np.asarray(ratio, F32), np.asarray(mean, F32)
    thresh = (ratio.max(2) - F32(0.1)).astype(F32)                     # RV:394, fp32
    w32 = np.where(ratio < thresh[:, :, None], F32(0), ratio)          # RV:395, fp32 compare
    diff = (hyp - mean[:, :, None]).astype(F32)                        # RV:398, fp32
    d, w = diff.astype(np.float64), w32.astype(np.float64)
    den = w.sum(2) + np.float64(F32(1e-3))                             # RV:401 (the constant is the fp32 one)
    prod = d[..., :, None] * d[..., None, :]                           # [b,vn,hn,2,2]
    cov = (prod * w[..., None, None]).sum(2) / den[..., None, None]
    s_abs = (np.abs(prod) * w[..., None, None]).sum(2) / den[..., None, None]
    return cov, s_abs, (w32 > 0).sum(2)


def topk_weights(ratio, topk, ties="first"):
    """RV:320-321's scatter of the top-k ratios into zeros.  ``ties="first"``
    is ``O.topk_scatter`` (among hypotheses equal to the k-th ratio the lowest
    indices are taken: the library's rule); ``"last"`` takes the highest
    indices instead -- the wrong rule, for tests that show they would notice."""
    ratio = np.asarray(ratio, F32)
    if ties == "first":
        return O.topk_scatter(ratio, topk)
    assert ties == "last"
    return O.topk_scatter(ratio[..., ::-1], topk)[..., ::-1]


def evd_topk_f64(hyp, ratio, topk, mean_used=None, ties="first", weights=None):
    """RV:320-329 in float64 on the oracle's fp32 ``hyp`` / ``ratio``, the
    selection by ``O.topk_scatter`` (or ``weights`` [b,vn,hn], an explicit
    scatter of the selected ratios, for another admissible choice among ties).

    Returns (mean f64 [b,vn,2], M_abs f64 [b,vn,2], cov f64 [b,vn,2,2],
    S_abs f64 [b,vn,2,2]): ``M_abs = sum_h |w q| / wsum``; the covariance is
    taken about ``mean_used`` (fp32 [b,vn,2], the mean the kernel returned, so
    that a bound on the covariance does not carry the mean's own rounding;
    default: the float64 mean rounded to fp32) with ``diff = fl32(hyp -
    mean_used)``, and ``S_abs[i,j] = sum_h |d_i d_j| w_h / wsum``."""
    hyp = np.asarray(hyp, F32)
    w = (topk_weights(ratio, topk, ties) if weights is None else np.asarray(weights, F32)).astype(np.float64)
    q = hyp.astype(np.float64)
    wsum = w.sum(2)
    mean = (w[..., None] * q).sum(2) / wsum[..., None]
    m_abs = np.abs(w[..., None] * q).sum(2) / wsum[..., None]
    mu = mean.astype(F32) if mean_used is None else np.asarray(mean_used, F32)
    d = (hyp - mu[:, :, None]).astype(F32).astype(np.float64)
    prod = d[..., :, None] * d[..., None, :]
    cov = (prod * w[..., None, None]).sum(2) / wsum[..., None, None]
    s_abs = (np.abs(prod) * w[..., None, None]).sum(2) / wsum[..., None, None]
    return mean, m_abs, cov, s_abs


def worst_ratio(err, bound):
    """max over the entries of err / bound (0 / 0 counts as 0, x / 0 as inf)."""
    err, bound = np.abs(np.asarray(err, np.float64)), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def tie_info(ratio_row, topk):
    """What k_evd_topk's tie rule has to do for one keypoint's ratios [hn]:
    the hypotheses equal to the k-th largest ratio (``ties``, ascending), how
    many of them the selection needs (``need``), and the ones taken / dropped
    under the lowest-index-first rule."""
    r = np.asarray(ratio_row)
    k = min(int(topk), r.shape[0])
    kth = np.sort(r)[::-1][k - 1]
    ties = np.nonzero(r == kth)[0]
    need = k - int((r > kth).sum())
    return dict(k=k, ties=ties, need=need, taken=ties[:need], dropped=ties[need:])


# ----------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False


def _scene(f, H, W, vn):
    mask = np.argmax(f["seg"], 1).astype(np.int64)
    vertex = np.ascontiguousarray(f["vertex"].transpose(0, 2, 3, 1).reshape(1, H, W, vn, 2))
    kps = np.asarray(f["keypoints"], np.float64)
    _frozen(mask, vertex, kps, f["seg"], f["vertex"])
    return dict(f=f, mask=mask, vertex=vertex, kps=kps, tn=int(f["tn"]), H=H, W=W, vn=vn)


@functools.lru_cache(maxsize=None)
def scene_large():
    """Scene 1: 208x208, vn = 2, a disk of 38,647 pixels -- more than the
    32,768 records per keypoint that k_refine_solve preloads, so its tail loop
    and k_point_conf's second stride run."""
    H = W = 208
    f = synth.synthetic_field(4, H=H, W=W, vn=2, radius=115., center=(104., 104.),
                              keypoints=[[60.3, 70.7], [150.1, 120.9]])
    return _scene(f, H, W, 2)


LARGE_KEEP_MAX_NUM = 36000
LARGE_KEEP_SEED = 1


@functools.lru_cache(maxsize=None)
def large_keep():
    """Scene 1's downsampling keep-mask at max_num = 36,000 (``synth.keep_mask``,
    injected on both sides): u8 [1,H,W]."""
    s = scene_large()
    keep = synth.keep_mask(s["mask"][0] != 0, LARGE_KEEP_MAX_NUM, np.random.default_rng(LARGE_KEEP_SEED))[None]
    _frozen(keep)
    return keep


def pairs(seed, tn, nh, vn):
    """Injected pixel pairs [1,nh,vn,2] (int32) in [0, tn)."""
    return np.random.default_rng(seed).integers(0, tn, (1, nh, vn, 2)).astype(np.int32)


LARGE_NH = 128


@functools.lru_cache(maxsize=None)
def oracle_large(downsampled=False, half=False):
    """The oracle's v5 run of scene 1 (v5 is v3 plus the confidence: one run
    serves both) at nh = 128, inlier_thresh 0.99: all pixels (max_num 100,000),
    or the kept ones at max_num 36,000; ``half``: on the fp16-rounded field.
    Returns dict(idxs, kp, conf, diag, max_num, keep)."""
    s = scene_large()
    keep = large_keep() if downsampled else None
    tn = int(((s["mask"][0] != 0) & (keep[0] != 0)).sum()) if downsampled else s["tn"]
    max_num = LARGE_KEEP_MAX_NUM if downsampled else 100000
    idxs = pairs(40 + downsampled, tn, LARGE_NH, 2)
    vertex = s["vertex"].astype(np.float16).astype(F32) if half else s["vertex"]
    dg = []
    kp, conf = O.ransac_voting_layer_v5(s["mask"], vertex, LARGE_NH, inlier_thresh=0.99, max_num=max_num,
                                        idxs=[idxs[0]], keep=keep, diag=dg)
    _frozen(idxs, kp, conf)
    return dict(idxs=idxs, kp=kp, conf=conf, diag=dg[0], max_num=max_num, keep=keep)


@functools.lru_cache(maxsize=None)
def scene_wide(vn=64):
    """Scene 2: 40x56, 64 keypoints (the ABI's upper bound), tn = 613;
    ``vn`` < 64 keeps the first keypoints' channels only."""
    H, W = 40, 56
    kps = np.random.default_rng(2).uniform([5, 5], [50, 35], (64, 2))
    f = synth.synthetic_field(5, H=H, W=W, vn=64, radius=14., center=(28., 20.), keypoints=kps)
    s = _scene(f, H, W, 64)
    if vn != 64:
        vertex = np.ascontiguousarray(s["vertex"][:, :, :, :vn])
        kp = s["kps"][:vn].copy()
        _frozen(vertex, kp)
        s = dict(s, vertex=vertex, kps=kp, vn=vn, f=None)
    return s


TIE_IDXS_SEED = 1
TIE_ROUND, TIE_MIN_HYP = 200, 600      # nh = 600 = 2 * 256 + 88


@functools.lru_cache(maxsize=None)
def scene_tie():
    """Scene 3: 48x64, vn = 2, 97 noisy pixels and 600 hypotheses: few pixels
    make many equal counts, so the top-k cut falls inside a run of ties that
    spreads over k_evd_topk's waves and 256-slabs.  ``idxs`` [3,200,2,2] are
    the EVD rounds' pixel pairs; ``hyp`` / ``ratio`` what the oracle collects."""
    H, W = 48, 64
    f = synth.synthetic_field(3, H=H, W=W, vn=2, radius=5.5, center=(30., 24.),
                              keypoints=[[20.3, 15.7], [45.1, 30.9]], noise=0.15, outlier=0.3)
    s = _scene(f, H, W, 2)
    idxs = np.random.default_rng(TIE_IDXS_SEED).integers(0, s["tn"], (3, TIE_ROUND, 2, 2)).astype(np.int32)
    hyp, ratio = evd_collect(s["mask"], s["vertex"], TIE_ROUND, TIE_MIN_HYP, idxs=[list(idxs)], min_num=5)
    _frozen(idxs, hyp, ratio)
    return dict(s, idxs=idxs, hyp=hyp, ratio=ratio)


def evd_collect(mask, vertex, round_hyp_num, min_hyp_num, idxs, min_num=5, max_num=30000, keep=None,
                inlier_thresh=0.99, guard=None):
    """``O._evd_collect``: the hypotheses [b,vn,hn,2] and ratios [b,vn,hn] both
    EVD layers reduce (bit-exact on the device)."""
    return O._evd_collect(mask, vertex, round_hyp_num, min_hyp_num, inlier_thresh, min_num, max_num, idxs, keep, 0,
                          guard_hyp_num=min_hyp_num if guard is None else guard)


# ---- k_refine_solve's nh switches ------------------------------------------
NH_SWITCHES = (1, 100, 1024, 1025, 1536)


@functools.lru_cache(maxsize=None)
def nh_switch_mask():
    """The first 20x20 block (blocks scanned row-major on a 20-pixel grid) that
    lies wholly inside scene 1's disk, as the mask: int64 [1,H,W], tn = 400."""
    s = scene_large()
    fg = s["mask"][0] != 0
    for r in range(0, s["H"] - 19, 20):
        for c in range(0, s["W"] - 19, 20):
            if fg[r:r + 20, c:c + 20].all():
                m = np.zeros_like(s["mask"])
                m[0, r:r + 20, c:c + 20] = 1
                _frozen(m)
                return m
    raise AssertionError("no 20x20 block inside the disk")


@functools.lru_cache(maxsize=None)
def nh_switch_runs(nh):
    """The three pixel-pair sets [1,nh,2,2] of test_refine_nh_switches:
    ``random``; ``last``, in which each keypoint's best pair of ``random``
    stands at h = nh - 1 only (every hypothesis that reached its count is
    replaced by the keypoint's worst pair); ``tie``, ``last`` with that pair
    also at h = min(5, nh - 1).  With each set the oracle's diag of it."""
    s, mask = scene_large(), nh_switch_mask()
    tn = int(mask.sum())
    rnd = np.random.default_rng(1000 + nh).integers(0, tn, (1, nh, 2, 2)).astype(np.int32)

    def run(ix):
        dg = []
        kp = O.ransac_voting_layer_v3(mask, s["vertex"], nh, idxs=[ix[0]], diag=dg)
        return dict(idxs=ix, kp=kp, diag=dg[0])

    first = run(rnd)
    cnt, win = first["diag"]["counts"], first["diag"]["win_idx"]
    last = rnd.copy()
    for v in range(2):
        pair = rnd[0, win[v], v].copy()
        last[0, cnt[:, v] == cnt[win[v], v], v] = rnd[0, int(np.argmin(cnt[:, v])), v]
        last[0, nh - 1, v] = pair
    tie = last.copy()
    for v in range(2):
        tie[0, min(5, nh - 1), v] = last[0, nh - 1, v]
    out = dict(random=first, last=run(last), tie=run(tie))
    _frozen(rnd, last, tie)
    return out


# ---- b_inv's identity fallback, per image ----------------------------------
SINGULAR_NH = 128


@functools.lru_cache(maxsize=None)
def scene_singular():
    """b = 2, vn = 3, 40x56.  Image 0 is a strip of 40 pixels on row 0 whose
    keypoint 0 has the constant direction (-1, 0): every pixel pair is
    parallel (hypothesis (0, 0), KU:75), every pixel votes for (0, 0), and
    the inliers' normals are all (0, 1), so ATA = [[0, 0], [0, 40]] has a
    zero pivot.  Its keypoints 1, 2 point at planted keypoints.  Image 1 is a
    regular field."""
    H, W, vn = 40, 56, 3
    f1 = synth.synthetic_field(7, H=H, W=W, vn=vn, radius=14., center=(28., 20.),
                               keypoints=[[12.3, 9.7], [40.1, 30.9], [30.6, 12.2]])
    s1 = _scene(f1, H, W, vn)
    mask = np.zeros((2, H, W), np.int64)
    vertex = np.zeros((2, H, W, vn, 2), F32)
    mask[1], vertex[1] = s1["mask"][0], s1["vertex"][0]
    cols = np.arange(5, 45)
    mask[0, 0, cols] = 1
    vertex[0, 0, cols, 0] = (-1.0, 0.0)
    for v, kp in ((1, (30.2, 15.6)), (2, (20.4, 25.3))):
        d = np.stack([kp[0] - cols, np.full(cols.shape, kp[1] - 0.0)], 1)
        vertex[0, 0, cols, v] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    rng = np.random.default_rng(17)
    idxs = np.stack([rng.integers(0, 40, (SINGULAR_NH, vn, 2)),
                     rng.integers(0, s1["tn"], (SINGULAR_NH, vn, 2))]).astype(np.int32)
    _frozen(mask, vertex, idxs)
    return dict(mask=mask, vertex=vertex, idxs=idxs, tn=(40, s1["tn"]), vn=vn)


# ---- the two foreground predicates -----------------------------------------
LABEL_VALUES = {np.int64: (1, 2, 255, 256, 257, -1), np.int32: (1, 2, 255, 256, 257, -1), np.uint8: (1, 2, 255)}


def label_map(dtype):
    """Scene 2's disk cut into bands of rows (equal pixel counts, row-major),
    band k holding ``LABEL_VALUES[dtype][k]``; background 0: [1,40,56]."""
    s = scene_wide()
    vals = LABEL_VALUES[dtype]
    rows, cols = np.nonzero(s["mask"][0])
    lab = np.zeros(s["mask"].shape, dtype)
    band = np.arange(rows.size) * len(vals) // rows.size
    lab[0, rows, cols] = np.array(vals, np.int64).astype(dtype)[band]
    return lab
