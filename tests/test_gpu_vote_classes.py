"""The hypotheses' classes made by their producer: compact_hyp and k_hyp_gen
store, beside each keypoint's hypotheses, the ballots of the fast ones and of the exact-only
ones per 32 (hyp_class, pvnet_amd/csrc/pv_hypclass.h; the workspace's first bytes,
[b][vn][4 ceil(nh / 128)][2] words), and the pipeline's k_vote_mfma -- which no longer makes
or classifies hypotheses -- reads its four sets' words.  Every case compares the vote counts
with the CPU oracle's vote_counts, bit for bit, and the stored words with hyp_class of the
stored hypotheses (tests/test_hyp_class.py's numpy restatement).

Frames are tiny (24 x 32; the first tn pixels are the foreground, so a pixel's compacted
index is its pixel index): with vn = 2 and hn = 512 the vote's work index has 8 tn pixel
steps, cut over at most 6 blocks of ~470 steps -- tn = 14 is one partial MFMA batch per
(keypoint, group), tn = 352 one full sub-chunk in the first block and tn = 353 a second
sub-chunk of one pixel.  Chosen pixel pairs make hypotheses that are degenerate ((0, 0)),
on the lattice, beyond kMHypMax and non-finite.  On a frame this small a non-finite
hypothesis needs directions above kN1Max (1e19: the intersection overflows), and such a
pixel sends its sub-chunk through the reference's sequence; so every size runs twice, without
that pair (the matrix-core path in every sub-chunk) and with it at the foreground's end."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.test_hyp_class import EXACT, FAST, restated

pytestmark = pytest.mark.gpu

H, W, HN, VN = 24, 32, 512, 2
F32 = np.float32
NSP = 6


def special(tn, nonfinite):
    """Pixel pairs (compacted indices, directions for every keypoint) and the class of their hypothesis."""
    sp = {"degenerate": ((0, (1.0, 0.0)), (1, (1.0, 0.0)), EXACT),     # parallel -> (0, 0), a lattice point
          "lattice": ((2, (1.0, 0.0)), (3, (0.0, 1.0)), EXACT),        # (3, 0) exactly
          "far": ((4, (0.0, 4.0)), (5, (4e-7, 4.0)), EXACT)}           # y = -1e7: finite, beyond kMHypMax
    if nonfinite:                                                      # 1e38 x overflows for a column x >= 4
        t1 = max(t for t in range(tn) if t % W >= 4)
        sp["nonfinite"] = ((t1 - 1, (1e19, 0.0)), (t1, (0.0, 1e19)), 0)
    return sp


def cu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _frame(tn, seed, H=H, W=W, vn=VN, fg=1, nonfinite=False):
    """mask [H,W] i64 (`fg` on the first tn pixels), vertex [H,W,vn,2]: unit directions towards
    keypoint targets off the lattice (with noise), the SPECIAL pixels' directions on top."""
    rng = np.random.default_rng(seed)
    mask = np.zeros(H * W, np.int64)
    mask[:tn] = fg
    kp = np.stack([rng.uniform(0.2, 0.8, vn) * W + 0.37, rng.uniform(0.2, 0.8, vn) * H + 0.41], 1)
    rows, cols = np.divmod(np.arange(H * W), W)
    d = kp[None] - np.stack([cols, rows], 1)[:, None]
    ang = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0, 0.05, d.shape[:2])
    ver = np.stack([np.cos(ang), np.sin(ang)], -1).astype(F32).reshape(H, W, vn, 2)
    for (t0, d0), (t1, d1), _ in special(tn, nonfinite).values():
        ver.reshape(H * W, vn, 2)[t0] = F32(d0)
        ver.reshape(H * W, vn, 2)[t1] = F32(d1)
    return mask.reshape(H, W), ver


def _ordinary_pairs(rng, coords, direct, n, free):
    """n pixel pairs [n, vn, 2] out of the ordinary pixels whose hypotheses are fast for every keypoint."""
    out = np.zeros((n, direct.shape[1], 2), np.int32)
    k = 0
    while k < n:
        cand = rng.choice(free, (4 * n, direct.shape[1], 2)).astype(np.int32)
        hyp = O.generate_hypothesis(direct, coords, cand)
        ok = np.all(restated(hyp[..., 0], hyp[..., 1]) == FAST, axis=1)
        take = cand[ok][:n - k]
        out[k:k + len(take)] = take
        k += len(take)
    return out


def _idxs(rng, coords, direct, nh, sp):
    """[nh, vn, 2]: set 0 all fast, set 1 all exact-only (lattice: no fast column), set 2 all
    non-finite where `sp` has that pair (neither word has a bit; else degenerate), set 3 all
    beyond kMHypMax, then each kind at columns 0.. and 31.. of every later set between ordinary ones."""
    vn, tn = direct.shape[1], coords.shape[0]
    used = {p[0] for p0, p1, _ in sp.values() for p in (p0, p1)}
    idxs = _ordinary_pairs(rng, coords, direct, nh, np.array(sorted(set(range(tn)) - used)))
    pair = {k: np.broadcast_to(np.int32([p0[0], p1[0]]), (vn, 2)) for k, (p0, p1, _) in sp.items()}
    idxs[32:64] = pair["lattice"]
    idxs[64:96] = pair.get("nonfinite", pair["degenerate"])
    idxs[96:128] = pair["far"]
    for c, k in enumerate(sp):
        idxs[128 + c::32] = pair[k]
        idxs[128 + 31 - c::32] = pair[k]
    return idxs


def _expected_words(hyp, nh):
    """hyp [nh, vn, 2] -> uint32 [vn, nset, 2]: the fast and the exact-only ballots per 32 hypotheses."""
    cls = restated(hyp[..., 0], hyp[..., 1])                       # [nh, vn]
    nset = 4 * (-(-nh // 128))
    out = np.zeros((hyp.shape[1], nset, 2), np.uint32)
    for h in range(nh):
        for v in range(hyp.shape[1]):
            for k, bit in ((0, FAST), (1, EXACT)):
                if cls[h, v] & bit:
                    out[v, h >> 5, k] |= np.uint32(1 << (h & 31))
    return out


def _workspace_words(ws, b, vn, nh):
    """(hypcls [b, vn, nset, 2], counts [b, vn, nh]) from the workspace's first bytes."""
    nset = 4 * (-(-nh // 128))
    ncls = -(-(2 * b * vn * nset) // 4) * 4
    buf = next(iter(ws._buf.values()))
    w = buf[:4 * (ncls + b * vn * nh)].cpu().numpy().view(np.uint32)
    return w[:2 * b * vn * nset].reshape(b, vn, nset, 2), w[ncls:].view(np.int32).reshape(b, vn, nh)


def _case(tn, seed, nonfinite):
    mask, ver = _frame(tn, seed, nonfinite=nonfinite)
    coords, direct = O.compact(O.fg_mask_v3(mask), ver)
    assert coords.shape[0] == tn and np.all(coords[:, 0] + W * coords[:, 1] == np.arange(tn))
    sp = special(tn, nonfinite)
    idxs = _idxs(np.random.default_rng(seed), coords, direct, HN, sp)
    hyp = O.generate_hypothesis(direct, coords, idxs)
    cls = restated(hyp[..., 0], hyp[..., 1])
    for c, (_, _, want) in enumerate(sp.values()):
        assert np.all(cls[128 + c::32] == want) and np.all(cls[128 + 31 - c::32] == want)
    assert np.all(cls[:32] == FAST) and np.all(cls[32:64] == EXACT) and np.all(cls[96:128] == EXACT)
    assert np.all(cls[64:96] == (0 if nonfinite else EXACT)) and np.all(np.isfinite(hyp[64:96])) != nonfinite
    assert np.all(np.isfinite(hyp[96:128])) and np.all(np.abs(hyp[96:128]).max(-1) > 8e6)
    return mask, ver, coords, direct, idxs, hyp


@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("tn", [14, 352, 353])
def test_tiny_frame_classes_and_counts(tn, nonfinite, device):
    from pvnet_amd import ransac_voting as rv
    from pvnet_amd import ransac_voting_gpu as rvg
    mask, ver, coords, direct, idxs, hyp = _case(tn, 100 + tn, nonfinite)
    want = O.vote_counts(direct, coords, hyp, 0.99)                # [hn, vn]
    ws, diag = rvg.VotingWorkspace(), {}
    rvg.ransac_voting_layer_v3(cu(mask[None], device), cu(ver[None], device), HN, min_num=1, _idxs=idxs[None],
                               _diag=diag, _workspace=ws)
    assert int(diag["tn"][0]) == tn
    ghyp = diag["hyp"].cpu().numpy()[0]
    np.testing.assert_array_equal(ghyp.view(np.uint32), hyp.view(np.uint32))
    np.testing.assert_array_equal(diag["counts"].cpu().numpy()[0].T, want)
    words, _ = _workspace_words(ws, 1, VN, HN)
    np.testing.assert_array_equal(words[0], _expected_words(ghyp, HN))
    assert np.all(words[0, :, 0] == [0xffffffff, 0]) and np.all(words[0, :, 1] == [0, 0xffffffff])
    assert np.all(words[0, :, 2] == [0, 0 if nonfinite else 0xffffffff]) and np.all(words[0, :, 3] == [0, 0xffffffff])
    # pv_vote_counts classifies the caller's hypotheses itself, through the same hyp_class
    got = rv.vote_counts(cu(direct, device), cu(coords, device), cu(hyp, device), 0.99).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def test_two_images_second_empty(device):
    from pvnet_amd import ransac_voting_gpu as rvg
    mask, ver, coords, direct, idxs, hyp = _case(353, 7, True)
    m2 = np.stack([mask, np.zeros_like(mask)])
    v2 = np.stack([ver, ver])
    ws, diag = rvg.VotingWorkspace(), {}
    kp = rvg.ransac_voting_layer_v3(cu(m2, device), cu(v2, device), HN, min_num=1, _idxs=np.stack([idxs, idxs]),
                                    _diag=diag, _workspace=ws)
    assert diag["tn"].cpu().numpy().tolist() == [353, 0] and np.all(kp[1].cpu().numpy() == 0)
    np.testing.assert_array_equal(diag["counts"].cpu().numpy()[0].T, O.vote_counts(direct, coords, hyp, 0.99))
    words, counts = _workspace_words(ws, 2, VN, HN)
    np.testing.assert_array_equal(words[0], _expected_words(hyp, HN))
    assert not words[1].any() and not counts[1].any()              # no hypotheses, no classes, no votes


def test_evd_with_mean_16_rounds(device):
    """estimate_voting_distribution_with_mean at 16 x 256 = 4,096 hypotheses (128 sets per
    keypoint; the foreground is mask == 1)."""
    from pvnet_amd import ransac_voting_gpu as rvg
    nh, tn = 4096, 200
    mask, ver = _frame(tn, 11, nonfinite=True)
    mask.reshape(-1)[tn:tn + 40] = 2                               # not foreground for EVD
    coords, direct = O.compact(O.fg_mask_evd(mask), ver)
    assert coords.shape[0] == tn
    idxs = _idxs(np.random.default_rng(11), coords, direct, nh, special(tn, True))
    hyp = O.generate_hypothesis(direct, coords, idxs)
    ws = rvg.VotingWorkspace()
    mean = np.tile(F32([[16.0, 12.0]]), (1, VN, 1))
    rvg.estimate_voting_distribution_with_mean(cu(mask[None], device), cu(ver[None], device), cu(mean, device), 256, nh,
                                               min_num=5, _idxs=idxs[None], _workspace=ws)
    words, counts = _workspace_words(ws, 1, VN, nh)
    np.testing.assert_array_equal(words[0], _expected_words(hyp, nh))
    np.testing.assert_array_equal(counts[0].T, O.vote_counts(direct, coords, hyp, 0.99))


def test_hyp_gen_route(device):
    """A frame above the fused hypotheses' 1,536 chunks (607 x 648: 1,537): k_hyp_gen makes the
    hypotheses and their classes."""
    from pvnet_amd import ransac_voting_gpu as rvg
    Hb, Wb, tn = 607, 648, 353
    mask, ver = _frame(tn, 13, H=Hb, W=Wb, nonfinite=True)
    coords, direct = O.compact(O.fg_mask_v3(mask), ver)
    idxs = _idxs(np.random.default_rng(13), coords, direct, HN, special(tn, True))
    hyp = O.generate_hypothesis(direct, coords, idxs)
    ws, diag = rvg.VotingWorkspace(), {}
    rvg.ransac_voting_layer_v3(cu(mask[None], device), cu(ver[None], device), HN, min_num=1, _idxs=idxs[None],
                               _diag=diag, _workspace=ws)
    np.testing.assert_array_equal(diag["hyp"].cpu().numpy()[0].view(np.uint32), hyp.view(np.uint32))
    np.testing.assert_array_equal(diag["counts"].cpu().numpy()[0].T, O.vote_counts(direct, coords, hyp, 0.99))
    words, _ = _workspace_words(ws, 1, VN, HN)
    np.testing.assert_array_equal(words[0], _expected_words(hyp, HN))


def test_vote_counts_null_hypotheses_is_einval(device):
    from pvnet_amd import _lib
    L = _lib.load()
    x = torch.zeros(64, dtype=torch.float32, device=device)
    c = torch.zeros(64, dtype=torch.int32, device=device)
    assert L.pv_vote_counts(x.data_ptr(), x.data_ptr(), None, c.data_ptr(), 4, 2, 4, 0.99, None) == -1   # PV_EINVAL
    torch.cuda.synchronize()
    assert not c.any()
