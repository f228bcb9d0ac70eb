"""CPU pins of ``tests/tail_refs.py``: the float64 EVD references against the
reference's golden vectors and the oracle, and the property each scene exists
for (so that a scene that stops exercising its edge fails here, without a
GPU)."""
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from tests import golden_io as G
from tests import tail_refs as R

COV_RTOL = R.COV_RTOL


def assert_cov(got, ref):
    np.testing.assert_allclose(got, ref, rtol=COV_RTOL, atol=1e-4 * np.abs(ref).max())


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("case", ["cat_evdm", "synth_evdm"])
def test_evd_with_mean_f64_matches_golden(case):
    g = G.load(case)
    mask, vertex = (G.cat_inputs(g) if case.startswith("cat") else G.synth_inputs(g))[:2]
    hyp, ratio = R.evd_collect(mask, vertex, 256, 4096, idxs=[list(g["idxs"][0])], min_num=20)
    cov, s_abs, kept = R.evd_with_mean_f64(hyp, ratio, g["mean"])
    assert_cov(cov, g["cov"])
    assert np.all(np.abs(cov) <= s_abs * (1 + 1e-12)) and np.all(kept >= 1) and np.all(kept <= 4096)


@pytest.fixture(scope="module")
def synth_top_collect():
    """The hypotheses and ratios of one golden's EVD rounds, by golden name."""
    cache = {}

    def get(name):
        if name not in cache:
            g = G.load(name)
            mask, vertex = G.synth_inputs(g)[:2]
            cache[name] = (g, *R.evd_collect(mask, vertex, 256, 4096, idxs=[list(g["idxs"][0])], guard=256))
        return cache[name]
    return get


def test_evd_topk_f64_matches_golden_top4096(synth_top_collect):
    g, hyp, ratio = synth_top_collect("synth_evd_top4096")
    mean, m_abs, cov, s_abs = R.evd_topk_f64(hyp, ratio, 4096)
    np.testing.assert_allclose(mean, g["mean"], atol=1e-3, rtol=1e-5)
    assert_cov(cov, g["cov"])
    assert np.all(np.abs(mean) <= m_abs * (1 + 1e-12)) and np.all(np.abs(cov) <= s_abs * (1 + 1e-12))


def test_evd_topk_f64_matches_golden_top128(synth_top_collect):
    """torch's topk(sorted=False) leaves the choice among hypotheses tied at
    the k-th ratio open (RV:320), so the golden's mean and
    covariance belong to *some* admissible choice: per keypoint, one of the
    ways to take ``need`` of the tied hypotheses must reproduce the golden
    within COV_RTOL (at most 5 ways here); where there is no choice, the
    lowest-index-first reference itself must."""
    g, hyp, ratio = synth_top_collect("synth_evd_top128")
    amax = 1e-4 * np.abs(g["cov"]).max()
    choices = []
    for v in range(9):
        r = ratio[0, v]
        ti = R.tie_info(r, 128)
        ok = []
        for sub in itertools.combinations(ti["ties"], ti["need"]):
            w = np.where(r > r[ti["ties"][0]], r, np.float32(0))
            w[list(sub)] = r[list(sub)]
            mean, _, cov, _ = R.evd_topk_f64(hyp[:, v:v + 1], ratio[:, v:v + 1], 128, weights=w[None, None])
            ok.append(bool(np.allclose(cov[0, 0], g["cov"][0, v], rtol=COV_RTOL, atol=amax)
                           and np.allclose(mean[0, 0], g["mean"][0, v], atol=1e-3, rtol=1e-5)))
        assert any(ok), (v, ok)
        choices.append(len(ok))
    assert max(choices) > 1                     # the golden does hold real ties


def test_f64_references_match_oracle_small_scenes():
    """Against O.estimate_voting_distribution[_with_mean] (fp32 matmul) on the
    tie scene (nh = 600) and the 64-keypoint scene (nh = 128)."""
    t = R.scene_tie()
    mean = t["kps"][None].astype(np.float32)
    _, co = O.estimate_voting_distribution_with_mean(t["mask"], t["vertex"], mean, R.TIE_ROUND, R.TIE_MIN_HYP,
                                                     min_num=5, idxs=[list(t["idxs"])])
    assert_cov(R.evd_with_mean_f64(t["hyp"], t["ratio"], mean)[0], co)
    for topk in (128, 300, 600, 1000):
        mo, co = O.estimate_voting_distribution(t["mask"], t["vertex"], R.TIE_ROUND, R.TIE_MIN_HYP, topk,
                                                idxs=[list(t["idxs"])])
        m64, _, c64, _ = R.evd_topk_f64(t["hyp"], t["ratio"], topk, mean_used=mo)
        np.testing.assert_allclose(m64, mo, atol=1e-3, rtol=1e-5)
        assert_cov(c64, co)
    w = R.scene_wide()
    idxs = R.pairs(21, w["tn"], 128, 64)
    hyp, ratio = R.evd_collect(w["mask"], w["vertex"], 128, 128, idxs=[[idxs[0]]])
    mean = w["kps"][None].astype(np.float32)
    _, co = O.estimate_voting_distribution_with_mean(w["mask"], w["vertex"], mean, 128, 128, min_num=5,
                                                     idxs=[[idxs[0]]])
    assert_cov(R.evd_with_mean_f64(hyp, ratio, mean)[0], co)
    mo, co = O.estimate_voting_distribution(w["mask"], w["vertex"], 128, 128, 16, idxs=[[idxs[0]]])
    m64, _, c64, _ = R.evd_topk_f64(hyp, ratio, 16, mean_used=mo)
    np.testing.assert_allclose(m64, mo, atol=1e-3, rtol=1e-5)
    assert_cov(c64, co)


def test_wrong_tie_rule_is_far_outside_the_bounds():
    """Highest index first among ties moves the tie scene's mean and
    covariance by more than 100 x the derived bounds at topk 128 and 300 (a
    tie slip in k_evd_topk cannot hide inside them), and changes nothing
    where every hypothesis is selected."""
    t = R.scene_tie()
    for topk in (128, 300):
        m, m_abs, c, s_abs = R.evd_topk_f64(t["hyp"], t["ratio"], topk)
        mw, _, cw, _ = R.evd_topk_f64(t["hyp"], t["ratio"], topk, ties="last", mean_used=m.astype(np.float32))
        assert R.worst_ratio(mw - m, R.EVD_MEAN_UNITS * R.U32 * m_abs) > 100
        assert R.worst_ratio(cw - c, R.EVD_COV_UNITS * R.U32 * s_abs) > 100
    for topk in (600, 1000):
        np.testing.assert_array_equal(R.topk_weights(t["ratio"], topk, "last"), t["ratio"])
        np.testing.assert_array_equal(R.topk_weights(t["ratio"], topk), t["ratio"])


# ---------------------------------------------------------------- the scenes
def test_scene_large_reaches_the_tail_loop():
    s = R.scene_large()
    assert s["tn"] == 38647 > 32768 and s["H"] * s["W"] % 256 == 0
    o = R.oracle_large()
    assert o["diag"]["tn"] == 38647
    assert np.abs(o["kp"][0] - s["kps"]).max() < 0.3
    assert np.all(np.abs(o["conf"] - 0.5) < 0.02)
    # k_refine_solve's tail loop and k_point_conf's second stride must matter: inliers beyond record 32,768
    d = o["diag"]
    inl = np.zeros((1, 2, d["tn"]), np.uint8)
    O.voting_for_hypothesis(d["direct"], d["coords"], d["win_pts"][None], inl, 0.99)
    assert np.all(inl[0, :, 32768:].sum(1) > 1000)
    od = R.oracle_large(downsampled=True)
    assert 32768 < od["diag"]["tn"] < R.LARGE_KEEP_MAX_NUM < od["diag"]["foreground"] == 38647
    assert np.abs(od["kp"][0] - s["kps"]).max() < 0.3


def test_scene_wide_and_label_maps():
    w = R.scene_wide()
    assert w["tn"] == 613 and w["vertex"].shape == (1, 40, 56, 64, 2)
    kp = O.ransac_voting_layer_v3(w["mask"], w["vertex"], 128, idxs=[R.pairs(20, w["tn"], 128, 64)[0]])
    assert np.abs(kp[0] - w["kps"]).max() < 1.0     # 20 % outliers on 613 pixels: sub-pixel, not exact
    w1 = R.scene_wide(1)
    assert w1["vertex"].shape == (1, 40, 56, 1, 2)
    np.testing.assert_array_equal(w1["vertex"][..., 0, :], w["vertex"][..., 0, :])
    for dt, vals in R.LABEL_VALUES.items():
        lab = R.label_map(dt)
        assert lab.dtype == dt and set(np.unique(lab)) == set(vals) | {0}
        v3, evd = O.fg_mask_v3(lab[0]), O.fg_mask_evd(lab[0])
        # the predicates differ on every value but 0 and 1; 256 is background for both
        assert int(evd.sum()) == int((lab == 1).sum()) >= 100
        assert int(v3.sum()) == int(np.isin(lab, [v for v in vals if v % 256 != 0]).sum())
        assert evd.sum() < v3.sum() <= 613 and (v3.sum() < 613) == (256 in vals)


# (topk, keypoint) -> (hypotheses tied at the k-th count, needed, first dropped tie)
TIE_TABLE = {(300, 0): (18, 5, 219), (300, 1): (17, 5, 141), (128, 0): (14, 7, None), (128, 1): (9, 1, None)}


def test_scene_tie_properties():
    t = R.scene_tie()
    assert t["tn"] == 97 and t["ratio"].shape == (1, 2, 600) and R.TIE_IDXS_SEED == 1
    straddles = []
    for (topk, v), (nties, need, first_dropped) in TIE_TABLE.items():
        ti = R.tie_info(t["ratio"][0, v], topk)
        assert (len(ti["ties"]), ti["need"]) == (nties, need), (topk, v)
        if first_dropped is not None:
            assert ti["dropped"][0] == first_dropped
        slabs = set(ti["ties"] // 256)
        assert slabs == ({0, 1} if (topk, v) == (128, 1) else {0, 1, 2}), (topk, v)
        assert ti["need"] < len(ti["ties"])
        # a taken and a dropped tie in different 64-lane waves of one 256-slab
        straddles.append(any(a // 256 == b // 256 and a // 64 != b // 64 for a in ti["taken"] for b in ti["dropped"]))
    assert any(straddles)
    for topk in (600, 1000):
        for v in range(2):
            ti = R.tie_info(t["ratio"][0, v], topk)
            assert ti["k"] == 600 and ti["need"] == len(ti["ties"])


def test_nh_switch_runs_place_the_winner():
    m = R.nh_switch_mask()
    assert int(m.sum()) == 400
    np.testing.assert_array_equal(O.fg_mask_v3(m[0]) & ~O.fg_mask_v3(R.scene_large()["mask"][0]), False)
    assert R.NH_SWITCHES == (1, 100, 1024, 1025, 1536)
    for nh in R.NH_SWITCHES:
        runs = R.nh_switch_runs(nh)
        for name, r in runs.items():
            assert r["diag"]["tn"] == 400 and r["idxs"].shape == (1, nh, 2, 2)
        best = runs["random"]["diag"]["counts"].max(0)
        assert np.all(best > 0)
        c = runs["last"]["diag"]["counts"]
        np.testing.assert_array_equal(runs["last"]["diag"]["win_idx"], [nh - 1] * 2)
        np.testing.assert_array_equal(c[nh - 1], best)
        if nh > 1:
            assert np.all(c[:nh - 1].max(0) < best)             # the winner stands at the last index only
        c = runs["tie"]["diag"]["counts"]
        first = min(5, nh - 1)
        np.testing.assert_array_equal(runs["tie"]["diag"]["win_idx"], [first] * 2)
        np.testing.assert_array_equal(c[first], best)
        np.testing.assert_array_equal(c[nh - 1], best)
        assert np.all((c == best).sum(0) == (2 if nh > 1 else 1))


def test_scene_singular_has_a_zero_pivot_in_image_0_only():
    s = R.scene_singular()
    dg = []
    kp = O.ransac_voting_layer_v3(s["mask"], s["vertex"], R.SINGULAR_NH, min_num=5, idxs=list(s["idxs"]), diag=dg)
    assert (dg[0]["tn"], dg[1]["tn"]) == s["tn"] and s["tn"][0] == 40
    np.testing.assert_array_equal(dg[0]["ATA"][0], [[0, 0], [0, 40]])
    assert dg[0]["win_ratio"][0] == 1.0                          # every pixel is an inlier of (0, 0)
    assert [O.lu2_solve_inv(a) is None for a in dg[0]["ATA"]] == [True, False, False]
    assert all(O.lu2_solve_inv(a) is not None for a in dg[1]["ATA"])
    np.testing.assert_array_equal(kp[0], dg[0]["ATb"])           # the identity for the whole image (RV:514-517)
    assert np.abs(kp[0, 1:]).max() > 100                         # ... which is far from any keypoint
    assert np.abs(kp[1] - [[12.3, 9.7], [40.1, 30.9], [30.6, 12.2]]).max() < 1.0
