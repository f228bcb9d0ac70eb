"""k_vote_mfma's band phase after its per-wave work was cut: the re-check
of a flagged MFMA takes whether a column is a fast hypothesis from a wave mask, tests
pix < np with wave-uniform masks per pair slot, combines both with the candidate
compare's ballot in scalar registers and packs a queue entry from precomputed parts;
its constants come from the host (tests/test_band_consts.py).  Every case compares
the pipeline's vote counts (hn = 512) with the CPU oracle's, bit for bit, the way
tests/test_gpu_vote_issue.py does, and with pv_vote_counts' on the same hypotheses
handed in by the caller.

The cases put pixels on the cone's edge of chosen hypotheses: the pixel's direction is
(h - c) turned by exactly acos(thr) (float64, rounded to float32), so z = X - |Y| of
that pair is zero up to rounding -- inside every band, a candidate of the re-check and
a pair only the reference's sequence decides.

Frames are 480 x 640 so that the vote grid is the full persistent one: with vn = 3 and
whole rows from row 40 as foreground, 256 k pixels give block u the pixels
[k (u % 256), + k) of keypoint u / 256, one sub-chunk of k <= 352 pixels."""
import numpy as np
import pytest

from oracle import oracle as O
from pvnet_amd import synth
from tests.test_gpu_vote_issue import HN, H, W, _api_counts, cu

pytestmark = pytest.mark.gpu

TINY = (1e-7, 0.0)      # |n| below 1e-6: the pixel never votes (KU's norm1 guard)


def _rows_mask(tn):
    mask = np.zeros((H, W), bool)
    mask.reshape(-1)[40 * W:40 * W + tn] = True
    return mask


def _field(seed, vn, mask=None, radius=97.5):
    f = synth.synthetic_field(seed, H=H, W=W, vn=vn, radius=radius, mask=mask)
    m64 = f["mask"][None].astype(np.int64)
    vv = np.ascontiguousarray(f["vertex"].transpose(0, 2, 3, 1).reshape(1, H, W, vn, 2))
    return m64, vv


def _good_pair(rng, coords, direct, free, avoid):
    """A pixel pair out of `free` whose hypotheses (every keypoint) are ordinary points at
    least 3 px from every pixel of `avoid`: inside the frame, off the integer lattice."""
    for _ in range(1000):
        pair = rng.choice(free, 2, replace=False).astype(np.int32)
        h = O.generate_hypothesis(direct, coords, np.broadcast_to(pair, (1, direct.shape[1], 2)).copy())[0]
        ok = np.all(np.isfinite(h)) and np.all(np.abs(h - [320, 240]) < [300, 220])
        ok = ok and np.all(np.abs(h - np.rint(h)) > 1e-3)
        if ok and all(np.hypot(*(coords[avoid].astype(np.float64) - hv).T).min() > 3.0 for hv in h):
            return pair
    raise AssertionError("no ordinary hypothesis found")


def _aim(vv, coords, direct, hyp, px, hs, thr):
    """Pixel px[i]'s direction for every keypoint v becomes (hyp[hs[i], v] - c) turned by
    +-acos(thr), alternating; written to the field `vv` and to `direct`."""
    th = np.arccos(np.float64(thr))
    for i, (t, h) in enumerate(zip(px, hs)):
        x, y = int(coords[t, 0]), int(coords[t, 1])
        for v in range(direct.shape[1]):
            d = hyp[h, v].astype(np.float64) - coords[t].astype(np.float64)
            assert np.hypot(*d) > 3.0
            a = th if (i + v) % 2 else -th
            e = np.array([np.cos(a) * d[0] - np.sin(a) * d[1], np.sin(a) * d[0] + np.cos(a) * d[1]]) / np.hypot(*d)
            vv[0, y, x, v] = e.astype(np.float32)
            direct[t, v] = e.astype(np.float32)


def _set_dir(vv, coords, direct, t, d):
    x, y = int(coords[t, 0]), int(coords[t, 1])
    vv[0, y, x, :] = np.float32(d)
    direct[t, :] = np.float32(d)


def _edge_votes(coords, direct, hyp, pairs, thr):
    """Does the oracle decide the (pixel, hypothesis) pairs both ways?  (Then the
    construction is on the cone's edge, not beside it.)"""
    votes = [O.vote_test(*(float(x) for x in (*direct[t, 0], *coords[t], *hyp[h, 0])), thr) for t, h in pairs]
    return 0 < sum(votes) < len(votes)


def _counts(device, m64, vv, idxs, thr):
    """Counts [b][hn, vn] of the pipeline (k_vote_mfma on the compacted records), checked
    against the oracle's; no downsampling."""
    from pvnet_amd import ransac_voting_gpu as rvg
    big = H * W + 1
    dg = []
    O.ransac_voting_layer_v3(m64, vv, HN, inlier_thresh=thr, min_num=1, max_num=big, idxs=list(idxs), diag=dg)
    diag = {}
    rvg.ransac_voting_layer_v3(cu(m64, device), cu(vv, device), HN, inlier_thresh=thr, min_num=1, max_num=big,
                               _idxs=idxs, _diag=diag)
    got = diag["counts"].cpu().numpy()
    for b in range(m64.shape[0]):
        np.testing.assert_array_equal(got[b].T, dg[b]["counts"])
    return got


def _check(device, m64, vv, coords, direct, idxs, thr, edge_pairs):
    """Pipeline == oracle == pv_vote_counts on the caller's hypotheses."""
    c2, d2 = O.compact(O.fg_mask_v3(m64[0]), vv[0])
    np.testing.assert_array_equal(c2, coords)
    np.testing.assert_array_equal(d2, direct)
    hyp = O.generate_hypothesis(direct, coords, idxs[0])
    got = _counts(device, m64, vv, idxs, thr)[0].T
    np.testing.assert_array_equal(_api_counts(device, coords, direct, hyp, thr), got)
    assert _edge_votes(coords, direct, hyp, edge_pairs[:400], thr)
    return hyp


def _edge_case(device, seed, k, thr, block, n_edge, groups, first=0):
    """vn = 3, k pixels per block; n_edge pixels of sub-chunk `block` (from its pixel
    `first`) sit on the edge of one point that is hypothesis 128 g + 32 (g % 4) + 5 g of
    each group g in `groups` (the same pixel pair: every such wave finds every edge pixel)."""
    vn, tn = 3, 256 * k
    m64, vv = _field(seed, vn, mask=_rows_mask(tn))
    coords, direct = O.compact(O.fg_mask_v3(m64[0]), vv[0])
    assert coords.shape[0] == tn
    rng = np.random.default_rng(seed)
    px = np.arange(block * k + first, block * k + first + n_edge)
    free = np.setdiff1d(np.arange(tn), px)
    idxs = rng.choice(free, (1, HN, vn, 2)).astype(np.int32)
    pair = _good_pair(rng, coords, direct, free, px)
    hs = [128 * g + 32 * (g % 4) + 5 * g for g in groups]
    for h in hs:
        idxs[0, h] = pair
    hyp = O.generate_hypothesis(direct, coords, idxs[0])
    _aim(vv, coords, direct, hyp, px, [hs[0]] * n_edge, thr)
    _check(device, m64, vv, coords, direct, idxs, thr, [(t, hs[0]) for t in px])


@pytest.mark.parametrize("thr", [0.99, 0.999999])
def test_many_candidates_every_wave(thr, device):
    """224 of one sub-chunk's 352 pixels on the edge of a point that is one hypothesis of
    each 128-hypothesis group: every wave of the block queues 224 pairs of one column,
    more than its 128-entry queue holds, so reference passes run mid-phase.  thr
    0.999999 is where K is largest."""
    _edge_case(device, 101, 352, thr, block=37, n_edge=224, groups=(0, 1, 2, 3), first=64)


def test_uneven_waves(device):
    """The same with the point a hypothesis of group 2 only: one wave's queue overflows,
    the block's other three find next to nothing."""
    _edge_case(device, 102, 352, 0.99, block=200, n_edge=224, groups=(2,), first=100)


@pytest.mark.parametrize("k", [1, 17, 351])
def test_last_batch_edge(k, device):
    """k pixels per (block, keypoint): the last batch is partial (1, 1 and 15 pixels).  In
    blocks of kind A the last batch's pixels are on the edge and a pixel that never
    votes sits inside the range; in blocks of kind B the final pixel never votes and the
    ones before it are on the edge: candidates are found beside the padding rows, whose
    slots must not be queued (pix < np)."""
    vn, tn, thr = 3, 256 * k, 0.99
    m64, vv = _field(110 + k, vn, mask=_rows_mask(tn))
    coords, direct = O.compact(O.fg_mask_v3(m64[0]), vv[0])
    rng = np.random.default_rng(k)
    last0 = (k - 1) // 16 * 16                      # first pixel of the last batch
    edge, tiny = [], []
    for blk in range(3, 256, 5):
        b0 = blk * k
        if k == 1:
            (edge if blk % 2 else tiny).append(b0)
        elif blk % 2:                                # A: the last batch on the edge, a silent pixel inside
            edge += list(range(b0 + last0, b0 + k))
            tiny.append(b0 + (k - 1) // 2 - 1)
        else:                                        # B: the final pixel silent, the ones before it on the edge
            tiny.append(b0 + k - 1)
            edge += list(range(b0 + max(last0 - 2, 0), b0 + k - 1))
    px = np.array(sorted(set(edge) - set(tiny)))
    special = np.union1d(px, tiny)
    free = np.setdiff1d(np.arange(tn), special)
    idxs = rng.choice(free, (1, HN, vn, 2)).astype(np.int32)
    pair = _good_pair(rng, coords, direct, free, special)
    hs = [5, 128 + 37, 256 + 74, 384 + 127]
    for h in hs:
        idxs[0, h] = pair
    hyp = O.generate_hypothesis(direct, coords, idxs[0])
    _aim(vv, coords, direct, hyp, px, [hs[0]] * len(px), thr)
    for t in tiny:
        _set_dir(vv, coords, direct, t, TINY)
    _check(device, m64, vv, coords, direct, idxs, thr, [(t, hs[0]) for t in px])


def test_every_set(device):
    """Edge pairs whose hypotheses sit at columns 0 and 31 of each of the four sets of one
    wave (eight different points): a wrong fragment, G or fast-hypothesis mask for one
    of the four sets shows."""
    vn, k, thr = 3, 352, 0.99
    tn = 256 * k
    m64, vv = _field(120, vn, mask=_rows_mask(tn))
    coords, direct = O.compact(O.fg_mask_v3(m64[0]), vv[0])
    rng = np.random.default_rng(120)
    px = np.arange(91 * k + 7, 91 * k + 7 + 128)
    free = np.setdiff1d(np.arange(tn), px)
    idxs = rng.choice(free, (1, HN, vn, 2)).astype(np.int32)
    hs = [128 * 1 + 32 * j + c for j in range(4) for c in (0, 31)]
    for h in hs:
        idxs[0, h] = _good_pair(rng, coords, direct, free, px)
    hyp = O.generate_hypothesis(direct, coords, idxs[0])
    tg = [hs[i % 8] for i in range(len(px))]
    _aim(vv, coords, direct, hyp, px, tg, thr)
    _check(device, m64, vv, coords, direct, idxs, thr, list(zip(px, tg)))


def test_slow_and_fast_sub_chunks_two_frames(device):
    """Two frames of different tn in one batch (~60k and ~5k pixels, vn = 9: ~760 pixels
    per block, so blocks hold two or three sub-chunks and one per keypoint straddles the
    image boundary).  One pixel of frame 0 with |n| above 1e18 sends its sub-chunk down the
    slow path; pixels 352 before and after it -- the same block's neighbouring
    sub-chunk on one side or the other -- are on the edge of a hypothesis of every
    group, and so are the first pixels of frame 1."""
    vn, thr = 9, 0.99
    ma, va = _field(21, vn, radius=138.0)
    mb, vb = _field(22, vn, radius=40.5)
    idxs, frames = [], []
    for f, (m64, vv) in enumerate(((ma, va), (mb, vb))):
        coords, direct = O.compact(O.fg_mask_v3(m64[0]), vv[0])
        tn = coords.shape[0]
        rng = np.random.default_rng(130 + f)
        if f == 0:
            assert 55000 < tn < 65000
            big = 30000
            px = np.concatenate([np.arange(big - 352 - 60, big - 352 + 60), np.arange(big + 352 - 60, big + 352 + 60)])
            special = np.append(px, big)
        else:
            assert 4000 < tn < 6500
            px = np.arange(0, 96)
            special = px
        free = np.setdiff1d(np.arange(tn), special)
        ix = rng.choice(free, (HN, vn, 2)).astype(np.int32)
        pair = _good_pair(rng, coords, direct, free, special)
        hs = [3, 128 + 40, 256 + 95, 384 + 100]
        for h in hs:
            ix[h] = pair
        hyp = O.generate_hypothesis(direct, coords, ix)
        _aim(vv, coords, direct, hyp, px, [hs[0]] * len(px), thr)
        if f == 0:
            _set_dir(vv, coords, direct, big, (3e18, 4e18))
        idxs.append(ix)
        frames.append((coords, direct, hyp, px, hs[0]))
    m64 = np.concatenate([ma, mb])
    vv = np.concatenate([va, vb])
    got = _counts(device, m64, vv, np.stack(idxs), thr)
    for b, (coords, direct, hyp, px, h0) in enumerate(frames):
        np.testing.assert_array_equal(_api_counts(device, coords, direct, hyp, thr), got[b].T)
        assert _edge_votes(coords, direct, hyp, [(t, h0) for t in px], thr)
