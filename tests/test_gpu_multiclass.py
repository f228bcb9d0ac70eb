"""Multi-object voting on the GPU: one label map and the keypoints of every
class in one pipeline (``ransac_voting_layer_v3_multi`` and friends), against
the oracle run per class on ``label == c + 1`` and against the existing
single-object layer on the stacked batch of binary masks.

The scene (90 x 150: 52.7 compaction chunks, a partial last one; 3 classes of
4 keypoints):
  * a disk of 1,517 px labelled 1;
  * a disk of 2,784 px labelled 2, clipped by the bottom border and reaching
    into the last chunk; with max_num = 2000 it is downsampled, the injected
    keep-mask leaves 1,983 px;
  * 29 px labelled 3: below min_num = 100 for v3 (exact zeros), voted by the
    EVD test (min_num = 20);
  * stray labels 4 and 257 (255 in a uint8 map), which belong to no class;
  * every class's vertex channels hold noise on the pixels that are not its
    own, so a wrong class offset shows.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

KP_TOL = 1e-2      # as tests/test_gpu_parity.py
COV_RTOL = 1e-4

H, W, C, VN = 90, 150, 3, 4
MIN_NUM, MAX_NUM = 100, 2000
FG = (1517, 2784, 29)
TN = (1517, 1983, 0)
KEYPOINTS = np.array([[[30., 20.], [55., 25.], [38., 48.], [44.5, 31.25]],
                      [[95., 60.], [130., 66.], [108., 85.], [118.5, 70.75]],
                      [[18., 73.], [23., 74.], [19., 78.], [21.5, 76.25]]], np.float32)


@pytest.fixture(scope="module")
def rvg():
    from pvnet_amd import ransac_voting_gpu
    return ransac_voting_gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cu(x, dev, dtype=None):
    t = torch.from_numpy(np.array(x, order="C"))               # a copy: the shared scene stays read-only
    return t.to(dev) if dtype is None else t.to(device=dev, dtype=dtype)


@functools.lru_cache(maxsize=None)
def scene():
    """label int64 [H,W] (with the 257 strays), vertex f32 [H,W,C*VN,2], keep u8 [C,H,W]."""
    rng = np.random.default_rng(20240611)
    yy, xx = np.mgrid[0:H, 0:W]
    label = np.zeros((H, W), np.int64)
    label[(xx - 40) ** 2 + (yy - 30) ** 2 <= 484] = 1
    label[(xx - 110) ** 2 + (yy - 70) ** 2 <= 1025] = 2
    label[(xx - 20) ** 2 + (yy - 75) ** 2 <= 9] = 3
    label[5, 100:104] = 4
    label[60, 10:13] = 257
    label[89, 0] = 257
    assert tuple(int((label == c + 1).sum()) for c in range(C)) == FG
    assert (label.reshape(-1)[52 * 256:] == 2).any()          # class 2 reaches the partial last chunk
    vertex = rng.standard_normal((H, W, C * VN, 2)).astype(np.float32)   # noise everywhere ...
    for c in range(C):                                         # ... but on the class's own pixels
        own = label == c + 1
        for v in range(VN):
            d = KEYPOINTS[c, v][None, None, :] - np.stack([xx, yy], -1).astype(np.float32)
            d = d + 0.02 * rng.standard_normal(d.shape).astype(np.float32) * np.linalg.norm(d, axis=-1, keepdims=True)
            n = np.linalg.norm(d, axis=-1, keepdims=True)
            d = np.where(n > 0, d / np.maximum(n, 1e-12), 0).astype(np.float32)
            vertex[own, c * VN + v] = d[own]
    keep = np.ones((C, H, W), np.uint8)
    pix = np.flatnonzero(label.reshape(-1) == 2)
    drop = rng.choice(pix, size=FG[1] - TN[1], replace=False)
    keep[1].reshape(-1)[drop] = 0
    label.setflags(write=False)
    vertex.setflags(write=False)
    keep.setflags(write=False)
    return label, vertex, keep


def label_as(dtype):
    label = scene()[0]
    if dtype == np.uint8:                                      # 257 does not fit: another label of no class
        return np.where(label == 257, 255, label).astype(np.uint8)
    return label.astype(dtype)


@functools.lru_cache(maxsize=None)
def v3_reference(nh):
    """The oracle per class on label == c + 1 with injected idxs / keep (computed once per nh)."""
    label, vertex, keep = scene()
    rng = np.random.default_rng(1000 + nh)
    idxs = np.zeros((C, nh, VN, 2), np.int32)
    kps, diags = [], []
    for c in range(C):
        if TN[c]:
            idxs[c] = rng.integers(0, TN[c], size=(nh, VN, 2), dtype=np.int32)
        dg = []
        kp = O.ransac_voting_layer_v3((label == c + 1)[None].astype(np.int64), vertex[None, :, :, c * VN:(c + 1) * VN],
                                      nh, min_num=MIN_NUM, max_num=MAX_NUM, idxs=idxs[c][None], keep=keep[c][None],
                                      diag=dg)
        kps.append(kp[0])
        diags.append(dg[0])
    return idxs, np.stack(kps), diags


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.uint8], ids=["int64", "int32", "uint8"])
@pytest.mark.parametrize("nh", [128, 40])
def test_oracle_parity(nh, dtype, device, rvg):
    """nh = 128: hypotheses by k_compact's first blocks, matrix-core vote; nh = 40: made in the vote kernel."""
    _, vertex, keep = scene()
    idxs, kp_ref, dref = v3_reference(nh)
    diag = {}
    kp = rvg.ransac_voting_layer_v3_multi(cu(label_as(dtype), device)[None], cu(vertex, device)[None], C, nh,
                                          min_num=MIN_NUM, max_num=MAX_NUM, _idxs=idxs[None], _keep=keep[None].copy(),
                                          _diag=diag).cpu().numpy()
    diag = {k: v.cpu().numpy() for k, v in diag.items()}
    assert kp.shape == (1, C, VN, 2)
    np.testing.assert_array_equal(diag["tn"][0], TN)
    for c in range(C):
        if dref[c].get("skipped"):
            assert np.all(bits(kp[0, c]) == 0)                 # exact zeros
            continue
        assert dref[c]["tn"] == TN[c]
        np.testing.assert_array_equal(bits(diag["hyp"][0, c]), bits(dref[c]["hyp"]))
        np.testing.assert_array_equal(diag["counts"][0, c].T, dref[c]["counts"])
        np.testing.assert_array_equal(diag["win_idx"][0, c], dref[c]["win_idx"])
        np.testing.assert_allclose(kp[0, c], kp_ref[c], atol=KP_TOL, rtol=0)
    assert dref[2].get("skipped") and not dref[0].get("skipped") and not dref[1].get("skipped")
    # the scene is a sane one: the voted keypoints are the planted ones
    assert np.abs(kp[0, :2] - KEYPOINTS[:2]).max() < 0.5


def stacked(rvg, label, vertex, ncls, nh, device, **kw):
    """The existing single-object layer on the [b*C] uint8 masks label == c + 1 and contiguous vertex slices."""
    b, h, w = label.shape
    vn = vertex.shape[3] // ncls
    cls = torch.arange(1, ncls + 1, device=device, dtype=label.dtype).view(1, ncls, 1, 1)
    masks = (label[:, None] == cls).to(torch.uint8).reshape(b * ncls, h, w)
    vs = vertex.reshape(b, h, w, ncls, vn, 2).permute(0, 3, 1, 2, 4, 5).reshape(b * ncls, h, w, vn, 2).contiguous()
    diag = {}
    out = rvg.ransac_voting_layer_v3(masks, vs, nh, _diag=diag, **kw)
    return out, diag


def assert_equal_to_stacked(out, diag, out_s, diag_s):
    b, ncls = out.shape[:2]
    np.testing.assert_array_equal(bits(out.cpu().numpy()).reshape(b * ncls, -1),
                                  bits(out_s.cpu().numpy()).reshape(b * ncls, -1))
    for k in ("tn", "counts", "win_idx"):
        a, s = diag[k].cpu().numpy(), diag_s[k].cpu().numpy()
        np.testing.assert_array_equal(a.reshape(s.shape), s, err_msg=k)
    a, s = diag["hyp"].cpu().numpy(), diag_s["hyp"].cpu().numpy()
    voted = diag_s["tn"].cpu().numpy() > 0                     # a skipped image's hypotheses are never written
    assert voted.any() and not voted.all()
    np.testing.assert_array_equal(bits(a).reshape(s.shape)[voted], bits(s)[voted], err_msg="hyp")


def test_stacked_equivalence(device, rvg):
    """b = 2, the RNG's idxs and downsampling (the keys of the virtual images, the look-back)."""
    label, vertex, _ = scene()
    lab = cu(np.stack([label, label[::-1]]), device)
    ver = cu(np.stack([vertex, vertex[::-1]]), device)
    kw = dict(min_num=MIN_NUM, max_num=MAX_NUM, _seed=77)
    diag = {}
    out = rvg.ransac_voting_layer_v3_multi(lab, ver, C, 128, _diag=diag, **kw)
    out_s, diag_s = stacked(rvg, lab, ver, C, 128, device, **kw)
    tn = diag["tn"].cpu().numpy()
    assert tn.shape == (2, C) and np.all(tn[:, 0] == FG[0]) and np.all(tn[:, 2] == 0)
    assert np.all((tn[:, 1] > 1800) & (tn[:, 1] < 2200))       # Bernoulli(2000 / 2784) of 2784: 2000 +- 8 sigma
    assert_equal_to_stacked(out, diag, out_s, diag_s)


def test_wide_form(device, rvg):
    """94 chunks x 6 images x 8 classes = 4512 > PVV_FG_WIDE_ABOVE (4096): the label counter's 8-chunk
    blocks and their group sums, k_compact's task form."""
    b, h, w, ncls, vn = 6, 120, 200, 8, 2
    assert -(-h * w // 256) * b * ncls > 4096 >= -(-h * w // 256) * (b - 1) * ncls
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    label = np.zeros((b, h, w), np.int32)
    for bi in range(b):
        for c in rng.permutation(ncls):
            cx, cy, r = rng.integers(0, w), rng.integers(0, h), rng.integers(8, 30)
            label[bi][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = c + 1
    label[:, -1, -5:] = 300                                    # no class, in the partial last chunk
    lab = cu(label, device)
    ver = cu(rng.standard_normal((b, h, w, ncls * vn, 2)).astype(np.float32), device)
    kw = dict(min_num=100, max_num=800, _seed=9)
    diag = {}
    out = rvg.ransac_voting_layer_v3_multi(lab, ver, ncls, 128, _diag=diag, **kw)
    out_s, diag_s = stacked(rvg, lab, ver, ncls, 128, device, **kw)
    tn = diag["tn"].cpu().numpy()
    fg = np.stack([(label == c + 1).sum((1, 2)) for c in range(ncls)], 1)
    assert (fg < 100).any() and (fg > 800).any() and ((fg >= 100) & (fg <= 800)).any()   # all three branches
    np.testing.assert_array_equal(tn[(fg >= 100) & (fg <= 800)], fg[(fg >= 100) & (fg <= 800)])
    assert np.all(tn[fg < 100] == 0)
    assert_equal_to_stacked(out, diag, out_s, diag_s)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_network_entry(dtype, device, rvg):
    """Logits [b,C+1,h,w] (channels-last memory) and an NCHW f16 vertex_pred, with ties and NaNs planted."""
    label, vertex, _ = scene()
    rng = np.random.default_rng(3)
    lab = np.where(label > C, 0, label)
    logits = rng.standard_normal((2, C + 1, H, W)).astype(np.float32)
    for bi, l in enumerate((lab, lab[::-1])):
        np.put_along_axis(logits[bi], l[None], 6.0, 0)
    logits[0, 1, 30, 30:50] = logits[0, 2, 30, 30:50] = 9.0    # ties of two maxima: the first wins
    logits[0, :, 31, 30:50] = 1.0                              # all equal: label 0
    logits[0, 2, 32, 30:50] = np.nan                           # NaN is the maximum
    logits[0, 1, 33, 30:50] = logits[0, 3, 33, 30:50] = np.nan   # the first NaN wins
    logits[0, 0, 34, 30:50] = np.nan                           # NaN in the background plane: label 0
    logits[1, 3, 60:70, 100:120] = np.inf
    logits[1, 1, 65, 100:120] = np.nan                         # NaN beats +inf
    seg = cu(logits, device, dtype).contiguous(memory_format=torch.channels_last)
    assert not seg.is_contiguous()
    vp = np.stack([vertex, vertex[::-1]]).reshape(2, H, W, C * VN * 2).transpose(0, 3, 1, 2)
    vertex_pred = cu(vp, device, torch.float16).contiguous()
    amax = torch.argmax(seg, 1)
    assert amax.dtype == torch.int64
    a = amax.cpu().numpy()
    assert np.all(a[0, 30, 30:50] == 1) and np.all(a[0, 31, 30:50] == 0) and np.all(a[0, 32, 30:50] == 2)
    assert np.all(a[0, 33, 30:50] == 1) and np.all(a[0, 34, 30:50] == 0) and np.all(a[1, 65, 100:120] == 1)
    kw = dict(min_num=MIN_NUM, max_num=MAX_NUM, _seed=21)
    diag = {}
    out = rvg.ransac_voting_layer_v3_multi_from_network(seg, vertex_pred, C, 128, _diag=diag, **kw)
    view = vertex_pred.permute(0, 2, 3, 1).unflatten(3, (C * VN, 2))
    diag_l = {}
    out_l = rvg.ransac_voting_layer_v3_multi(amax, view, C, 128, _diag=diag_l, **kw)
    assert out.shape == (2, C, VN, 2) and int(diag["tn"][0, 0]) > 1000
    assert_equal_to_stacked(out, diag, out_l, diag_l)


@functools.lru_cache(maxsize=None)
def evd_reference():
    label, vertex, keep = scene()
    rng = np.random.default_rng(4)
    nh, rhn = 256, 64
    tn = (TN[0], TN[1], FG[2])                                 # min_num = 20: class 3 votes too
    idxs = np.stack([rng.integers(0, tn[c], size=(nh, VN, 2), dtype=np.int32) for c in range(C)])
    covs = []
    for c in range(C):
        _, cov = O.estimate_voting_distribution_with_mean(
            (label == c + 1)[None].astype(np.int64), vertex[None, :, :, c * VN:(c + 1) * VN], KEYPOINTS[c][None],
            round_hyp_num=rhn, min_hyp_num=nh, min_num=20, max_num=MAX_NUM,
            idxs=[list(idxs[c].reshape(nh // rhn, rhn, VN, 2))], keep=keep[c][None])
        covs.append(cov[0])
    return idxs, np.stack(covs)


def test_evd_with_mean(device, rvg):
    label, vertex, keep = scene()
    idxs, cov_ref = evd_reference()
    assert np.isfinite(cov_ref).all() and np.linalg.cond(cov_ref.astype(np.float64)).max() < 100
    mean = cu(KEYPOINTS, device)[None]
    m, cov = rvg.estimate_voting_distribution_with_mean_multi(
        cu(label, device)[None], cu(vertex, device)[None], mean, C, round_hyp_num=64, min_hyp_num=256, min_num=20,
        max_num=MAX_NUM, _idxs=idxs[None], _keep=keep[None].copy())
    assert m is mean and cov.shape == (1, C, VN, 2, 2)
    cov = cov.cpu().numpy()
    for c in range(C):      # the tolerance of tests/test_gpu_parity.py's EVD tests, per class
        np.testing.assert_allclose(cov[0, c], cov_ref[c], rtol=COV_RTOL, atol=1e-4 * np.abs(cov_ref[c]).max())


def test_graph_capture(device, rvg):
    """One multi call captured after a warm-up with an explicit workspace; two replays equal the eager result."""
    label, vertex, _ = scene()
    lab, ver = cu(label, device)[None], cu(vertex, device)[None]
    ws = rvg.VotingWorkspace()
    kw = dict(min_num=MIN_NUM, max_num=MAX_NUM, _seed=5, _workspace=ws)
    ref = rvg.ransac_voting_layer_v3_multi(lab, ver, C, 128, **kw).clone()
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gph, stream=s):
            out = rvg.ransac_voting_layer_v3_multi(lab, ver, C, 128, **kw)
    assert np.abs(ref.cpu().numpy()[0, :2] - KEYPOINTS[:2]).max() < 0.5
    for _ in range(2):
        out.zero_()
        gph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(ref.cpu().numpy()))
