"""The stages after the vote on their edge shapes: k_refine_solve and
k_point_conf (pvrefine.hip), k_evd_with_mean, k_evd_topk and k_motion_vote
(pvevd.hip), through the Python layers.

Everything discrete (tn, hypotheses, counts, winners, v5 confidence) is
bit-equal to the CPU oracle; the EVD reductions are held to bounds derived
from the kernels' roundings against float64 restatements of the same
arithmetic (``tests/tail_refs.py``, pinned on the CPU by
``tests/test_tail_refs.py``, which also asserts that each scene reaches the
edge it is named for).  Every test prints its worst error / bound (``-s``).

Derived bounds (u = 2^-24, the fp32 unit roundoff):

* EVD covariance entries: ``|got - ref64| <= 8 u S_abs`` with ``S_abs = sum_h
  |d_i d_j| w_h / den``.  Both kernels round each term once in fp32 (``dx *
  w``; ``diff`` and ``w`` themselves are the reference's fp32 values), sum in
  fp64, then round the sum, the denominator (twice with mean: the weight sum
  and ``+ 1e-3f``; once for top-k) and the quotient to fp32: 5 units, 8 leaves
  room for the order of the fp64 sum.
* top-k mean: ``|got - ref64| <= 4 u sum|w q| / wsum``: one rounding per term
  (``w * q``), one of the sum, one of ``wsum``, one of the quotient.
* motion: within one fp32 ulp of the oracle's fp64 mean rounded to fp32 (the
  kernel adds the same fp32 terms in fp64 in another order, then rounds once).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import tail_refs as R

pytestmark = pytest.mark.gpu

F32 = np.float32
KP_TOL = R.KP_TOL
COV_RTOL = R.COV_RTOL


@pytest.fixture(scope="module")
def rvg():
    from pvnet_amd import ransac_voting_gpu
    return ransac_voting_gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def cu(x, dev, dtype=None):
    t = torch.from_numpy(np.array(x, order="C"))       # a copy: the cached scenes are read-only arrays
    return t.to(dev) if dtype is None else t.to(device=dev, dtype=dtype)


class Worst:
    """Prints each check's worst error / bound, asserts it is at most 1, and
    prints the test's worst at the end."""

    def __init__(self, test):
        self.test, self.worst = test, 0.0

    def add(self, what, got, ref, bound):
        r = R.worst_ratio(np.asarray(got, np.float64) - np.asarray(ref, np.float64), bound)
        print(f"  {self.test}: {what}: err / bound = {r:.3g}")
        self.worst = max(self.worst, r)
        assert r <= 1.0, (self.test, what, r)

    def close(self, what, got, ref, rtol, atol):
        """numpy's allclose criterion as a bound."""
        self.add(what, got, ref, atol + rtol * np.abs(np.asarray(ref, np.float64)))

    def done(self):
        print(f"{self.test}: worst err / bound = {self.worst:.3g}")


def conf_at(od, pts, thr=0.999):
    """RV:856-858 by the oracle's vote on the pixels of its diag ``od``: the
    inlier ratio of ``pts`` [vn,2] at ``thr``."""
    vn, tn = pts.shape[0], od["tn"]
    inl = np.zeros((1, vn, tn), np.uint8)
    O.voting_for_hypothesis(od["direct"], od["coords"], np.ascontiguousarray(pts, F32)[None], inl, thr)
    return inl.sum(2)[0].astype(F32) / F32(tn)


def check_pipeline(w, what, diag, i, od, kp=None, ko=None):
    """Image ``i`` of a device ``_diag`` against the oracle's diag ``od``."""
    vn = od["hyp"].shape[1]
    assert int(diag["tn"][i]) == od["tn"], what
    np.testing.assert_array_equal(bits(diag["hyp"][i]), bits(od["hyp"]), err_msg=what)
    np.testing.assert_array_equal(diag["counts"][i].T, od["counts"], err_msg=what)
    np.testing.assert_array_equal(diag["win_idx"][i], od["win_idx"], err_msg=what)
    np.testing.assert_array_equal(bits(diag["win_ratio"][i]), bits(od["win_ratio"]), err_msg=what)
    assert int(diag["iters"][i]) == od["iters"], what
    w.close(what + " ata", diag["ata"][i].reshape(vn, 2, 2), od["ATA"], 1e-6, 1e-7 * np.abs(od["ATA"]).max())
    w.close(what + " atb", diag["atb"][i].reshape(vn, 2), od["ATb"], 1e-6, 1e-7 * np.abs(od["ATb"]).max())
    if kp is not None:
        w.close(what + " keypoints", kp, ko, 0, KP_TOL)


def run_v3_v5(rvg, device, w, what, mask, vertex, nh, idxs, od, ko, conf_o, **kw):
    """v3 and v5 on one single-image scene against the oracle's v5 run (v5's
    max_iter = 20 on both, for the iteration count)."""
    m, v, idxs = cu(mask, device), cu(vertex, device), np.array(idxs)
    diag = {}
    kp = rvg.ransac_voting_layer_v3(m, v, nh, max_iter=20, _idxs=idxs, _diag=diag, **kw).cpu().numpy()
    diag = {k: t.cpu().numpy() for k, t in diag.items()}
    check_pipeline(w, what + " v3", diag, 0, od, kp[0], ko[0])
    diag5 = {}
    kp5, conf = rvg.ransac_voting_layer_v5(m, v, nh, inlier_thresh=0.99, _idxs=idxs, _diag=diag5, **kw)
    kp5, conf = kp5.cpu().numpy(), conf.cpu().numpy()
    diag5 = {k: t.cpu().numpy() for k, t in diag5.items()}
    check_pipeline(w, what + " v5", diag5, 0, od, kp5[0], ko[0])
    np.testing.assert_array_equal(bits(kp5), bits(kp), err_msg=what)
    # k_point_conf on its own input (the device's points), then end to end
    np.testing.assert_array_equal(bits(conf[0]), bits(conf_at(od, kp5[0])), err_msg=what + " conf at device points")
    np.testing.assert_array_equal(bits(conf[0]), bits(conf_o[0]), err_msg=what + " conf")
    return kp, conf


def check_evd_with_mean(rvg, device, w, what, mask, vertex, mean, rnd, mn, idxs, hyp, ratio, **kw):
    _, cov = rvg.estimate_voting_distribution_with_mean(cu(mask, device), cu(vertex, device), cu(mean, device), rnd,
                                                        mn, min_num=5, _idxs=np.array(idxs), **kw)
    cov = cov.cpu().numpy()
    c64, s_abs, kept = R.evd_with_mean_f64(hyp, ratio, mean)
    print(f"  {what}: hypotheses kept by the max - 0.1 rule: {kept.min()}..{kept.max()} of {ratio.shape[2]}")
    w.add(what + " cov (with mean)", cov, c64, R.EVD_COV_UNITS * R.U32 * s_abs)
    np.testing.assert_array_equal(bits(cov[..., 0, 1]), bits(cov[..., 1, 0]))
    return cov


def check_evd_topk(rvg, device, w, what, mask, vertex, topk, rnd, mn, idxs, hyp, ratio, **kw):
    mu, cov = rvg.estimate_voting_distribution(cu(mask, device), cu(vertex, device), rnd, mn, topk, min_num=5,
                                               _idxs=np.array(idxs), **kw)
    mu, cov = mu.cpu().numpy(), cov.cpu().numpy()
    m64, m_abs, _, _ = R.evd_topk_f64(hyp, ratio, topk)
    _, _, c64, s_abs = R.evd_topk_f64(hyp, ratio, topk, mean_used=mu)
    w.add(what + f" mean (top {topk})", mu, m64, R.EVD_MEAN_UNITS * R.U32 * m_abs)
    w.add(what + f" cov (top {topk})", cov, c64, R.EVD_COV_UNITS * R.U32 * s_abs)
    np.testing.assert_array_equal(bits(cov[..., 0, 1]), bits(cov[..., 1, 0]))
    return mu, cov


# ---------------------------------------------------------------- refine and v5
def test_refine_tail_loop_large_tn(device, rvg):
    """tn = 38,647 (> the 32,768 records k_refine_solve preloads per keypoint:
    its tail loop, k_point_conf's second stride) for v3 and v5; the same frame
    downsampled by an injected keep-mask at max_num 36,000 (32,768 < tn <
    36,000: the compacted set still reaches the tail loop); and the fp16
    network layout through the fused entry."""
    w = Worst("refine_tail_loop_large_tn")
    s = R.scene_large()
    for ds in (False, True):
        o = R.oracle_large(downsampled=ds)
        assert o["diag"]["tn"] > 32768
        run_v3_v5(rvg, device, w, "downsampled" if ds else "all pixels", s["mask"], s["vertex"], R.LARGE_NH,
                  o["idxs"], o["diag"], o["kp"], o["conf"], max_num=o["max_num"],
                  _keep=np.array(o["keep"]) if ds else None)
    o = R.oracle_large(half=True)
    diag = {}
    kp = rvg.ransac_voting_layer_v3_from_network(cu(s["f"]["seg"], device, torch.float16),
                                                 cu(s["f"]["vertex"], device, torch.float16), R.LARGE_NH,
                                                 max_num=100000, _idxs=np.array(o["idxs"]), _diag=diag).cpu().numpy()
    diag = {k: t.cpu().numpy() for k, t in diag.items()}
    check_pipeline(w, "fp16 from_network", diag, 0, o["diag"], kp[0], o["kp"][0])
    w.done()


def _raises_for_65_keypoints(rvg, device):
    m = torch.ones((1, 40, 56), dtype=torch.int64, device=device)
    v = torch.zeros((1, 40, 56, 65, 2), device=device)
    mean = torch.zeros((1, 65, 2), device=device)
    for call in (lambda: rvg.ransac_voting_layer_v3(m, v, 128),
                 lambda: rvg.ransac_voting_layer_v5(m, v, 128),
                 lambda: rvg.ransac_motion_voting(m, v),
                 lambda: rvg.estimate_voting_distribution_with_mean(m, v, mean, 128, 128),
                 lambda: rvg.estimate_voting_distribution(m, v, 128, 128, 16)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            call()


@pytest.mark.parametrize("nh", [128, 40, 512])
@pytest.mark.parametrize("vn", [1, 64])
def test_vn_bounds(vn, nh, device, rvg):
    """vn = 1 and vn = 64 (the ABI's bound: the gather's sks[64] / srat[64],
    the one-wave solve) through v3, v5 and both EVD layers.  The pipeline
    votes on the matrix cores, with pre-generated keypoint-major hypotheses,
    when ceil(nh / 128) is a multiple of 4 (hyp_pregen_used): nh = 512 here;
    nh = 128 and 40 vote in k_vote_count and refine from the reference
    layout.  65 keypoints are refused by the host check of every entry."""
    w = Worst(f"vn_bounds[{vn}-{nh}]")
    s = R.scene_wide(vn)
    idxs = R.pairs(100 + vn + nh, s["tn"], nh, vn)
    dg = []
    ko, co = O.ransac_voting_layer_v5(s["mask"], s["vertex"], nh, inlier_thresh=0.99, max_num=30000,
                                      idxs=[idxs[0]], diag=dg)
    run_v3_v5(rvg, device, w, "scene 2", s["mask"], s["vertex"], nh, idxs, dg[0], ko, co, max_num=30000)
    hyp, ratio = R.evd_collect(s["mask"], s["vertex"], nh, nh, idxs=[[idxs[0]]])
    np.testing.assert_array_equal(bits(hyp[0].transpose(1, 0, 2)), bits(dg[0]["hyp"]))   # the same hypotheses
    mean = s["kps"][None].astype(F32)
    check_evd_with_mean(rvg, device, w, "scene 2", s["mask"], s["vertex"], mean, nh, nh, idxs, hyp, ratio)
    check_evd_topk(rvg, device, w, "scene 2", s["mask"], s["vertex"], 16, nh, nh, idxs, hyp, ratio)
    _raises_for_65_keypoints(rvg, device)
    w.done()


@pytest.mark.parametrize("nh", R.NH_SWITCHES)
def test_refine_nh_switches(nh, device, rvg):
    """k_refine_solve on both sides of its switches: nh = 1 and 100 (fewer
    hypotheses than the block's threads), 1024 (the last nh of the LDS
    instantiation), 1025 and 1536 (k_refine_solve<true>, whose loop reads the
    counts past 1024; 1024 and 1536 vote on the matrix cores and hand it the
    keypoint-major hypotheses, 1025 the reference layout), on 400 pixels; with random pairs, with the winner at
    the last index only, and with a first / last tie the first must win."""
    w = Worst(f"refine_nh_switches[{nh}]")
    s, mask = R.scene_large(), R.nh_switch_mask()
    assert int(mask.sum()) == 400
    runs = R.nh_switch_runs(nh)
    best = runs["random"]["diag"]["counts"].max(0)
    c = runs["last"]["diag"]["counts"]
    assert np.all(runs["last"]["diag"]["win_idx"] == nh - 1) and np.all(c[nh - 1] == best)
    assert nh == 1 or np.all(c[:nh - 1].max(0) < best)
    c, first = runs["tie"]["diag"]["counts"], min(5, nh - 1)
    assert np.all(runs["tie"]["diag"]["win_idx"] == first) and np.all(c[first] == best) and np.all(c[nh - 1] == best)
    m, v = cu(mask, device), cu(s["vertex"], device)
    for name, r in runs.items():
        diag = {}
        kp = rvg.ransac_voting_layer_v3(m, v, nh, _idxs=np.array(r["idxs"]), _diag=diag).cpu().numpy()
        diag = {k: t.cpu().numpy() for k, t in diag.items()}
        check_pipeline(w, name, diag, 0, r["diag"], kp[0], r["kp"][0])
    w.done()


def test_singular_fallback_is_per_image(device, rvg):
    """b_inv's identity fallback (RV:514-517) holds for the image that has a
    singular keypoint -- all three of its keypoints come out as ATb -- and
    for no other image of the batch."""
    w = Worst("singular_fallback_is_per_image")
    s = R.scene_singular()
    dg = []
    ko = O.ransac_voting_layer_v3(s["mask"], s["vertex"], R.SINGULAR_NH, min_num=5, idxs=list(s["idxs"]), diag=dg)
    assert O.lu2_solve_inv(dg[0]["ATA"][0]) is None and all(O.lu2_solve_inv(a) is not None for a in dg[1]["ATA"])
    np.testing.assert_array_equal(ko[0], dg[0]["ATb"])
    m, v = cu(s["mask"], device), cu(s["vertex"], device)
    diag = {}
    kp = rvg.ransac_voting_layer_v3(m, v, R.SINGULAR_NH, min_num=5, _idxs=np.array(s["idxs"]), _diag=diag).cpu().numpy()
    diag = {k: t.cpu().numpy() for k, t in diag.items()}
    check_pipeline(w, "image 0", diag, 0, dg[0])
    np.testing.assert_array_equal(diag["ata"][0, 0], [[0, 0], [0, 40]])
    np.testing.assert_array_equal(bits(kp[0]), bits(diag["atb"][0]))          # identity: the points are ATb
    w.close("image 0 keypoints (= ATb)", kp[0], ko[0], 1e-6, 0)
    check_pipeline(w, "image 1", diag, 1, dg[1], kp[1], ko[1])
    assert np.abs(kp[1] - diag["atb"][1]).max() > 1                          # ... and solved here
    k1 = rvg.ransac_voting_layer_v3(m[1:], v[1:], R.SINGULAR_NH, min_num=5, _idxs=np.array(s["idxs"][1:])).cpu().numpy()
    np.testing.assert_array_equal(bits(kp[1]), bits(k1[0]))
    w.done()


# ---------------------------------------------------------------- EVD
@pytest.mark.parametrize("topk", [128, 300, 600, 1000])
def test_evd_topk_ties(topk, device, rvg):
    """k_evd_topk's tie rule (the first ``need`` hypotheses equal to the k-th
    count, in index order: ballot prefix in a wave, wave offsets through LDS,
    a running base over the 256-slabs) where the ties straddle waves and
    slabs, nh = 600 = 2 * 256 + 88, and topk >= nh.  The wrong rule (highest
    index first) is more than 100 bounds away at topk 128 and 300, so a tie
    slip cannot pass."""
    w = Worst(f"evd_topk_ties[{topk}]")
    t = R.scene_tie()
    idxs = t["idxs"].reshape(1, R.TIE_MIN_HYP, 2, 2)
    if topk in (128, 300):
        m, m_abs, c, s_abs = R.evd_topk_f64(t["hyp"], t["ratio"], topk)
        mw, _, cw, _ = R.evd_topk_f64(t["hyp"], t["ratio"], topk, ties="last", mean_used=m.astype(F32))
        far_m = R.worst_ratio(mw - m, R.EVD_MEAN_UNITS * R.U32 * m_abs)
        far_c = R.worst_ratio(cw - c, R.EVD_COV_UNITS * R.U32 * s_abs)
        print(f"  wrong tie rule: mean {far_m:.3g} bounds away, covariance {far_c:.3g}")
        assert far_m > 100 and far_c > 100
    check_evd_topk(rvg, device, w, "scene 3", t["mask"], t["vertex"], topk, R.TIE_ROUND, R.TIE_MIN_HYP, idxs,
                   t["hyp"], t["ratio"])
    w.done()


def test_evd_with_mean_ragged_nh(device, rvg):
    """k_evd_with_mean at nh = 600 (a partial last stride) and nh = 64 (fewer
    hypotheses than threads); then a batch of [scene 3, an empty mask, 3
    pixels] through both EVD layers: the images below min_num give
    w d d^T / (w + 1e-3) with w = min_hyp_num, d = -mean (RV:343-348), and
    zeros from the top-k layer (RV:276-281)."""
    w = Worst("evd_with_mean_ragged_nh")
    t = R.scene_tie()
    mean = t["kps"][None].astype(F32)
    idxs = t["idxs"].reshape(1, R.TIE_MIN_HYP, 2, 2)
    cov0 = check_evd_with_mean(rvg, device, w, "nh 600", t["mask"], t["vertex"], mean, R.TIE_ROUND, R.TIE_MIN_HYP,
                               idxs, t["hyp"], t["ratio"])
    i64 = R.pairs(64, t["tn"], 64, 2)
    hyp, ratio = R.evd_collect(t["mask"], t["vertex"], 64, 64, idxs=[[i64[0]]])
    check_evd_with_mean(rvg, device, w, "nh 64", t["mask"], t["vertex"], mean, 64, 64, i64, hyp, ratio)
    # the batch
    mask = np.zeros((3,) + t["mask"].shape[1:], np.int64)
    mask[0] = t["mask"][0]
    mask[2, 10, 20:23] = 1
    vertex = np.repeat(t["vertex"], 3, 0)
    means = np.stack([mean[0], [[3.5, -2.25], [10.0, 7.0]], [[-1.5, 4.0], [0.25, 8.0]]]).astype(F32)
    bidx = np.zeros((3, R.TIE_MIN_HYP, 2, 2), np.int32)
    bidx[0] = idxs[0]
    _, cov = rvg.estimate_voting_distribution_with_mean(cu(mask, device), cu(vertex, device), cu(means, device),
                                                        R.TIE_ROUND, R.TIE_MIN_HYP, min_num=5, _idxs=bidx)
    cov = cov.cpu().numpy()
    np.testing.assert_array_equal(bits(cov[0]), bits(cov0[0]))
    _, co = O.estimate_voting_distribution_with_mean(mask, vertex, means, R.TIE_ROUND, R.TIE_MIN_HYP, min_num=5,
                                                     idxs=[list(t["idxs"]), None, None])
    d = -means[1:].astype(np.float64)
    closed = R.TIE_MIN_HYP * d[..., :, None] * d[..., None, :] / (R.TIE_MIN_HYP + np.float64(F32(1e-3)))
    for ref, name in ((co[1:], "oracle"), (closed, "closed form")):
        w.close(f"below min_num, with mean vs {name}", cov[1:], ref, COV_RTOL, 1e-4 * np.abs(ref).max())
    for topk in (128, 1000):
        mu, cv = rvg.estimate_voting_distribution(cu(mask, device), cu(vertex, device), R.TIE_ROUND, R.TIE_MIN_HYP,
                                                  topk, min_num=5, _idxs=bidx)
        mu, cv = mu.cpu().numpy(), cv.cpu().numpy()
        # (the oracle with one round of 600: its guard rows then have the voted image's length)
        mo, co = O.estimate_voting_distribution(mask, vertex, R.TIE_MIN_HYP, R.TIE_MIN_HYP, topk, min_num=5,
                                                idxs=[[idxs[0]], None, None])
        assert not mo[1:].any() and not co[1:].any()
        np.testing.assert_array_equal(mu[1:], 0)
        np.testing.assert_array_equal(cv[1:], 0)
        m64, m_abs, _, _ = R.evd_topk_f64(t["hyp"], t["ratio"], topk)
        _, _, c64, s_abs = R.evd_topk_f64(t["hyp"], t["ratio"], topk, mean_used=mu[:1])
        w.add(f"batch image 0 mean (top {topk})", mu[:1], m64, R.EVD_MEAN_UNITS * R.U32 * m_abs)
        w.add(f"batch image 0 cov (top {topk})", cv[:1], c64, R.EVD_COV_UNITS * R.U32 * s_abs)
        w.close(f"batch image 0 cov (top {topk}) vs oracle", cv[:1], co[:1], COV_RTOL, 1e-4 * np.abs(co[:1]).max())
    w.done()


def test_evd_large_tn(device, rvg):
    """Both EVD layers on tn = 38,647 (max_num 100,000), 256 hypotheses."""
    w = Worst("evd_large_tn")
    s = R.scene_large()
    idxs = R.pairs(50, s["tn"], 256, 2)
    hyp, ratio = R.evd_collect(s["mask"], s["vertex"], 256, 256, idxs=[[idxs[0]]], max_num=100000)
    mean = s["kps"][None].astype(F32)
    check_evd_with_mean(rvg, device, w, "scene 1", s["mask"], s["vertex"], mean, 256, 256, idxs, hyp, ratio,
                        max_num=100000)
    check_evd_topk(rvg, device, w, "scene 1", s["mask"], s["vertex"], 128, 256, 256, idxs, hyp, ratio, max_num=100000)
    w.done()


# ---------------------------------------------------------------- motion
def check_motion(rvg, device, w, what, mask, vertex, half=False):
    """mask [b,H,W] (any supported dtype), vertex f32 [b,H,W,vn,2] offsets;
    ``half``: the device gets the fp16 NCHW tensor's permuted view and the
    oracle the fp16-rounded values."""
    b, H, W, vn, _ = vertex.shape
    if half:
        nchw = np.ascontiguousarray(vertex.reshape(b, H, W, 2 * vn).transpose(0, 3, 1, 2)).astype(np.float16)
        vt = cu(nchw, device).permute(0, 2, 3, 1).view(b, H, W, vn, 2)
        assert not vt.is_contiguous()
        vertex = np.ascontiguousarray(nchw.astype(F32).transpose(0, 2, 3, 1).reshape(b, H, W, vn, 2))
    else:
        vt = cu(vertex, device)
    got = rvg.ransac_motion_voting(cu(mask, device), vt).cpu().numpy()
    ref = O.ransac_motion_voting(mask, vertex)
    equal = float((bits(got) == bits(ref)).mean())
    print(f"  {what}: bit-equal share {equal:.4f}")
    w.add(what, got, ref, np.spacing(np.abs(ref)))
    return got


def test_motion_edges(device, rvg):
    """k_motion_vote: a frame whose pixel count is no multiple of the block
    (37 x 51 = 1,887), tn > 32,768, vn at 1 / 9 / 64, every mask dtype, fp32
    and strided fp16 vertex, an empty image and one whose only foreground
    pixel is the frame's last."""
    w = Worst("motion_edges")
    rng = np.random.default_rng(77)
    H, W = 37, 51
    base = rng.random((2, H, W)) < 0.5
    kinds = ((np.int64, 3), (np.int32, 3), (np.uint8, 200), (np.bool_, True))
    for vn in (1, 9, 64):
        vertex = rng.normal(0, 3, (2, H, W, vn, 2)).astype(F32)
        for dt, val in kinds:
            mask = (base * val).astype(dt)
            for half in (False, True):
                check_motion(rvg, device, w, f"37x51 vn {vn} {np.dtype(dt).name} {'fp16 view' if half else 'fp32'}",
                             mask, vertex, half)
    s = R.scene_large()
    vertex = rng.normal(0, 3, (1, 208, 208, 2, 2)).astype(F32)
    for half in (False, True):
        check_motion(rvg, device, w, f"tn 38,647 {'fp16 view' if half else 'fp32'}", s["mask"], vertex, half)
    mask = np.zeros((3, H, W), np.int64)
    mask[0] = base[0]
    mask[2, H - 1, W - 1] = 1
    vertex = rng.normal(0, 3, (3, H, W, 9, 2)).astype(F32)
    got = check_motion(rvg, device, w, "b 3: random, empty, last pixel", mask, vertex)
    assert not got[1].any()
    np.testing.assert_array_equal(bits(got[2]), bits(vertex[2, H - 1, W - 1] + np.array([W - 1, H - 1], F32)))
    w.done()


# ---------------------------------------------------------------- predicates
@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.uint8], ids=["int64", "int32", "uint8"])
def test_mask_value_semantics(dtype, device, rvg):
    """The two foreground predicates side by side on label values where they
    differ (1, 2, 255, 256, 257, -1; uint8: 1, 2, 255): v3, v5 and motion
    count ``(m & 0xFF) != 0`` (RV:533 ``mask.byte()``), both EVD layers
    ``m == 1`` (RV:340, RV:273)."""
    w = Worst(f"mask_value_semantics[{np.dtype(dtype).name}]")
    s = R.scene_wide(4)
    lab = R.label_map(dtype)
    fg3 = O.fg_mask_v3(lab[0])[None].astype(np.int64)
    fge = O.fg_mask_evd(lab[0])[None].astype(np.int64)
    n3, ne = int(fg3.sum()), int(fge.sum())
    assert ne < n3 and ne == int((lab == 1).sum())
    nh = 128
    idxs = R.pairs(7, n3, nh, 4)
    dg = []
    ko, co = O.ransac_voting_layer_v5(fg3, s["vertex"], nh, inlier_thresh=0.99, max_num=30000, idxs=[idxs[0]],
                                      diag=dg)
    assert dg[0]["tn"] == n3
    run_v3_v5(rvg, device, w, "labels", lab, s["vertex"], nh, idxs, dg[0], ko, co, max_num=30000)
    got = rvg.ransac_motion_voting(cu(lab, device), cu(s["vertex"], device)).cpu().numpy()
    ref = O.ransac_motion_voting(fg3, s["vertex"])
    w.add("motion", got, ref, np.spacing(np.abs(ref)))
    iev = R.pairs(8, ne, 64, 4)
    hyp, ratio = R.evd_collect(fge, s["vertex"], 64, 64, idxs=[[iev[0]]])
    mean = s["kps"][None].astype(F32)
    check_evd_with_mean(rvg, device, w, "labels", lab, s["vertex"], mean, 64, 64, iev, hyp, ratio)
    check_evd_topk(rvg, device, w, "labels", lab, s["vertex"], 16, 64, 64, iev, hyp, ratio)
    w.done()
