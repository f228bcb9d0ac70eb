"""k_vote_mfma after its issue-slot cuts: the per-wave work that
was moved or replaced by an exact equivalent -- the hypothesis classes made by
the lane that makes the hypothesis, the B fragments and bands made by lane
half and exchanged, the pixel validity tested on the squared norm, the
exact-only pass behind one wave-uniform test -- and the hot loop's batch
edges.  Every case compares the pipeline's vote counts (hn = 512) with the
CPU oracle's, bit for bit, the way test_gpu_vote_mfma.py does.

Frames are 480 x 640 so that the vote grid is the full persistent one (the
bench's): with vn = 3 a frame of 256 k foreground pixels gives every block k
pixels of one keypoint."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O
from pvnet_amd import synth

pytestmark = pytest.mark.gpu

H, W, HN = 480, 640, 512
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pvnet_amd", "csrc", "pv_common.h")


def cu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _frame(seed, vn, mask=None, radius=97.5, specials=()):
    """A synthetic field plus `specials`: pixels (x, y, dx, dy) added to the mask with
    the given direction for every keypoint.  Returns (mask [1,H,W] i64, vertex
    [1,H,W,vn,2], coords, direct, {(x, y): compacted index})."""
    f = synth.synthetic_field(seed, H=H, W=W, vn=vn, radius=radius, mask=mask)
    m = f["mask"].copy()
    vv = np.ascontiguousarray(f["vertex"].transpose(0, 2, 3, 1).reshape(1, H, W, vn, 2))
    for x, y, dx, dy in specials:
        assert not m[y, x]
        m[y, x] = True
        vv[0, y, x, :, 0] = np.float32(dx)
        vv[0, y, x, :, 1] = np.float32(dy)
    m64 = m[None].astype(np.int64)
    coords, direct = O.compact(O.fg_mask_v3(m64[0]), vv[0])
    index = {(int(c[0]), int(c[1])): i for i, c in enumerate(coords)}
    return m64, vv, coords, direct, index


def _pipeline_vs_oracle(device, m64, vv, idxs, thr=0.99):
    """Counts [hn, vn] of the pipeline (k_vote_mfma on the compacted records), checked
    against the oracle's; no downsampling (max_num above the frame's foreground)."""
    from pvnet_amd import ransac_voting_gpu as rvg
    big = H * W + 1
    dg = []
    O.ransac_voting_layer_v3(m64, vv, HN, inlier_thresh=thr, min_num=1, max_num=big, idxs=[idxs[0]], diag=dg)
    diag = {}
    rvg.ransac_voting_layer_v3(cu(m64, device), cu(vv, device), HN, inlier_thresh=thr, min_num=1, max_num=big,
                               _idxs=idxs, _diag=diag)
    got = diag["counts"].cpu().numpy()[0].T
    np.testing.assert_array_equal(got, dg[0]["counts"])
    return got


def _api_counts(device, coords, direct, hyp, thr=0.99):
    """The same vote through pv_vote_counts: the caller's hypotheses, raw pixel operands."""
    from pvnet_amd import ransac_voting as rv
    return rv.vote_counts(cu(direct, device), cu(coords, device), cu(hyp, device), thr).cpu().numpy()


@pytest.mark.parametrize("k", [1, 15, 16, 17, 351, 352])
def test_batch_edges(k, device):
    """k pixels per (block, keypoint): one pixel, one short of / exactly / one past a
    16-pixel MFMA batch, and the bench's 22-batch sub-chunk one short and full (the last
    batch's read-ahead is the slab's last).  vn = 3 and 256 k foreground pixels (whole
    rows from row 40) over the 768 blocks of the full grid."""
    vn, tn = 3, 256 * k
    mask = np.zeros((H, W), bool)
    mask.reshape(-1)[40 * W:40 * W + tn] = True
    m64, vv, coords, direct, _ = _frame(10 + k, vn, mask=mask)
    assert coords.shape[0] == tn
    idxs = np.random.default_rng(k).integers(0, tn, (1, HN, vn, 2)).astype(np.int32)
    _pipeline_vs_oracle(device, m64, vv, idxs)


def test_blocks_span_sub_chunks(device):
    """~60k foreground pixels, vn = 9, max_num raised: ~700 pixels per block, two or
    three sub-chunks each with a partial last one."""
    m64, vv, coords, direct, _ = _frame(21, 9, radius=138.0)
    tn = coords.shape[0]
    assert 55000 < tn < 65000
    idxs = np.random.default_rng(21).integers(0, tn, (1, HN, 9, 2)).astype(np.int32)
    _pipeline_vs_oracle(device, m64, vv, idxs)


def test_hypothesis_classes_in_every_set(device):
    """Pixel pairs whose hypotheses are degenerate (parallel directions -> (0, 0)), an
    exact lattice point (exact-only), beyond kMHypMax = 8e6 (exact-only in k_vote_mfma)
    and non-finite (never an inlier), at columns 0..3 of every 32-hypothesis set of
    every wave, between ordinary ones.  The classes are made by the lane that makes
    the hypothesis and exchanged across the lane halves, and a wave with no exact-only
    hypothesis skips that pass on one wave-uniform test; here every wave has some in
    every set.  Counts equal the oracle's, and equal pv_vote_counts' on the same
    hypotheses handed in by the caller."""
    vn = 3
    sp = [(600, 456, 1.0, 0.0), (610, 458, 1.0, 0.0),            # parallel
          (600, 462, 1.0, 0.0), (620, 464, 0.0, 1.0),            # (620, 462) exactly
          (600, 466, 4.0, 0.0), (600, 476, 4.0, 4e-6),           # x = 600 - 1e7
          (600, 470, 9e17, 0.0), (605, 472, 0.0, 9e17)]          # overflow: inf / inf
    m64, vv, coords, direct, ix = _frame(31, vn, specials=sp)
    tn = coords.shape[0]
    idxs = np.random.default_rng(31).integers(0, tn - len(sp), (1, HN, vn, 2)).astype(np.int32)
    t = [ix[(x, y)] for x, y, _, _ in sp]
    for kind in range(4):
        idxs[0, kind::32, :, 0] = t[2 * kind]
        idxs[0, kind::32, :, 1] = t[2 * kind + 1]
    hyp = O.generate_hypothesis(direct, coords, idxs[0])
    assert np.all(hyp[0::32] == 0)
    assert np.all(hyp[1::32] == np.float32([620, 462]))
    assert np.all(np.abs(hyp[2::32, :, 0]) > 8e6) and np.all(np.isfinite(hyp[2::32]))
    assert not np.any(np.isfinite(hyp[3::32]))
    got = _pipeline_vs_oracle(device, m64, vv, idxs)
    np.testing.assert_array_equal(_api_counts(device, coords, direct, hyp), got)


def test_four_sets_at_four_distances(device):
    """Sets 0..3 of every wave hold hypotheses about 1e1, 1e3, 1e5 and 5e6 px from the
    mask (scales s = 1 .. 2^-9, bands four orders of magnitude apart): each lane half
    makes two sets' fragments and bands and receives the other two's."""
    vn = 3
    eps = [1.0, 1e-2, 1e-4, 2e-6]
    sp = [(600, 460, 1.0, 0.0)] + [(580 + 2 * j, 470, 1.0, eps[j]) for j in range(4)]   # x = xb - 10 / eps
    m64, vv, coords, direct, ix = _frame(41, vn, specials=sp)
    tn = coords.shape[0]
    idxs = np.random.default_rng(41).integers(0, tn - len(sp), (1, HN, vn, 2)).astype(np.int32)
    for j in range(4):
        for c in range(8):
            idxs[0, 32 * j + c::128, :, 0] = ix[(600, 460)]
            idxs[0, 32 * j + c::128, :, 1] = ix[(580 + 2 * j, 470)]
    hyp = O.generate_hypothesis(direct, coords, idxs[0])
    for j, d in enumerate([1e1, 1e3, 1e5, 5e6]):
        x = hyp[32 * j::128, :, 0]
        assert np.all(np.abs(x - (580 + 2 * j)) > 0.9 * d) and np.all(np.abs(x - (580 + 2 * j)) < 1.1 * d), (j, x)
    got = _pipeline_vs_oracle(device, m64, vv, idxs)
    np.testing.assert_array_equal(_api_counts(device, coords, direct, hyp), got)


def _const(name):
    m = re.search(r"constexpr float " + name + r" = (0x[0-9a-fA-F.]+p[+-]?\d+)f;", open(HDR).read())
    return np.float32(float.fromhex(m.group(1)))


def _dir_with_sq(S):
    """(nx, ny), about (0.8, 0.6) sqrt(S), with fl(fl(nx nx) + fl(ny ny)) == S in float32."""
    S = np.float32(S)
    r = np.sqrt(np.float64(S))
    off = np.arange(-48, 48, dtype=np.int32)
    nx = (np.float32(0.8 * r).view(np.int32) + off).view(np.float32)
    ny = (np.float32(0.6 * r).view(np.int32) + off).view(np.float32)
    s = (nx * nx)[:, None] + (ny * ny)[None, :]
    assert s.dtype == np.float32
    i, j = np.argwhere(s == S)[0]
    return float(nx[i]), float(ny[j])


@pytest.mark.parametrize("which", ["low", "max", "nonfinite"])
def test_norm_boundary(which, device):
    """Pixels whose squared norm is the validity constant T, its successor and its
    predecessor (kN1SqLow: the pixel votes or never does; kN1SqMax: inside or outside
    the fast domain), and pixels with a NaN or an infinite component: votes equal the
    oracle's, whose norm1 is the reference's sqrtf."""
    vn = 3
    # the pixels sit below the disk and point (0.6, -0.8) (mirrored if need be) at keypoint 0,
    # where the hypotheses gather: whether such a pixel votes shows in the counts
    kx, ky = synth.field_keypoints(51, vn)[0]
    sx = 1.0 if kx > 320 else -1.0
    if which == "nonfinite":
        dirs = [(np.nan, 1.0), (1.0, np.inf)]
    else:
        T = _const("kN1SqLow" if which == "low" else "kN1SqMax")
        dirs = []
        for s in (T, np.nextafter(T, np.float32(np.inf)), np.nextafter(T, np.float32(0))):
            a, b = _dir_with_sq(s)
            dirs.append((sx * b, -a))
    sp = []
    for i, (dx, dy) in enumerate(dirs):
        y = 456 + 2 * i
        sp.append((int(round(kx - sx * 0.6 * (y - ky) / 0.8)), y, dx, dy))
    m64, vv, coords, direct, ix = _frame(51, vn, specials=sp)
    tn = coords.shape[0]
    idxs = np.random.default_rng(51).integers(0, tn - len(sp), (1, HN, vn, 2)).astype(np.int32)
    if which == "low":
        # (the oracle's counts change when the boundary pixels are taken out: they do decide votes)
        hyp = O.generate_hypothesis(direct, coords, idxs[0])
        d0 = direct.copy()
        d0[[ix[(x, y)] for x, y, _, _ in sp]] = 0
        assert np.any(O.vote_counts(direct, coords, hyp, 0.99) != O.vote_counts(d0, coords, hyp, 0.99))
    _pipeline_vs_oracle(device, m64, vv, idxs)
