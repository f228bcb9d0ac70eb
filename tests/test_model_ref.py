"""tests/model_ref.py (the numpy restatement of include/pvmodel.h) against what the project's tests
used so far -- render_ref.spread_keypoints and the broadcast norm -- and its own rules: the tie
rule, the kept centroid, k above the point count, absent points, the lane order of the centroid."""
import numpy as np
import pytest

from tests import model_ref as M
from tests import render_ref as R

MESHES = {"ellipsoid3": lambda: R.bumpy_ellipsoid(3)[0], "box": lambda: R.box(0.05, 0.04, 0.03)[0],
          "icosphere5": lambda: R.icosphere(5)[0]}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_centroid_start_is_spread_keypoints(name):
    verts = MESHES[name]()
    want = R.spread_keypoints(verts, 8)
    r = M.farthest_points(M.widen(verts), 8, M.START_CENTROID)
    np.testing.assert_array_equal(r["picked"], want[:8])           # the same vertices, ties included
    np.testing.assert_array_equal(M.widen(verts)[r["idx"]], want[:8])
    e = M.extent(M.widen(verts))
    np.testing.assert_array_equal(e["centroid"], want[8])          # the lane order and numpy.mean agree here
    assert e["count"] == verts.shape[0]
    np.testing.assert_array_equal(e["bbox_min"], M.widen(verts).min(0))
    np.testing.assert_array_equal(e["bbox_max"], M.widen(verts).max(0))


@pytest.mark.parametrize("name", ["ellipsoid3", "box"])
def test_diameter_is_the_broadcast_norm(name):
    v = M.widen(MESHES[name]())
    want = float(np.max(np.linalg.norm(v[:, None] - v[None], axis=2)))
    got = M.diameter(v)
    assert abs(got - want) <= np.spacing(want)                     # 1 ulp: the norm sums in another order


def test_tie_goes_to_the_lowest_index():
    # a square: from corner 0 the far corner 2 wins, then 1 and 3 tie and 1 is taken
    v = M.widen([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    r = M.farthest_points(v, 4, M.START_INDEX, 0)
    assert r["idx"].tolist() == [0, 2, 1, 3] and r["pick_d2"].tolist() == [np.inf, 2.0, 1.0, 1.0]
    # centroid start: all four corners tie, so corner 0
    assert M.farthest_points(v, 2, M.START_CENTROID)["idx"].tolist() == [0, 2]
    # identical points: every pick is index 0, the diameter is 0
    same = M.widen(np.ones((7, 3)))
    r = M.farthest_points(same, 5, M.START_CENTROID)
    assert r["idx"].tolist() == [0] * 5 and r["pick_d2"].tolist() == [0.0] * 5 and M.diameter(same) == 0.0


def test_kept_centroid_changes_the_picks():
    # three points on a line, centroid at 1: plain goes to the far end, kept prefers the point away from the centre too
    v = M.widen([[0, 0, 0], [0.9, 0, 0], [2.1, 0, 0], [1.0, 3.0, 0]])
    plain = M.farthest_points(v, 4, M.START_CENTROID)
    kept = M.farthest_points(v, 4, M.START_CENTROID_KEPT)
    assert plain["idx"][0] == kept["idx"][0] and plain["pick_d2"][0] == kept["pick_d2"][0]
    c = M.extent(v)["centroid"]
    md = np.minimum(M.d2(v, c), M.d2(v, v[kept["idx"][0]]))
    assert kept["idx"][1] == int(np.argmax(md)) and kept["pick_d2"][1] == md.max()
    assert (kept["pick_d2"][1:] <= plain["pick_d2"][1:]).all()
    rng = np.random.default_rng(3)
    w = M.widen(rng.normal(size=(200, 3)) * [1.0, 0.2, 0.2])
    assert M.farthest_points(w, 8, M.START_CENTROID)["idx"].tolist() != \
        M.farthest_points(w, 8, M.START_CENTROID_KEPT)["idx"].tolist()


def test_k_above_the_point_count_repeats():
    v = M.widen(np.random.default_rng(0).normal(size=(5, 3)))
    r5, r8 = M.farthest_points(v, 5), M.farthest_points(v, 8)
    assert sorted(r5["idx"].tolist()) == [0, 1, 2, 3, 4]
    assert r8["idx"][:5].tolist() == r5["idx"].tolist() and r8["idx"][5:].tolist() == [0, 0, 0]
    assert r8["pick_d2"][5:].tolist() == [0.0, 0.0, 0.0]


def test_absent_points_and_skips():
    rng = np.random.default_rng(1)
    p = rng.normal(size=(40, 3)).astype(np.float32)
    clean = M.farthest_points(M.widen(p), 6)
    far = int(clean["idx"][0])
    q = p.copy()
    q[far] = [np.nan, 0, 0]
    q[3] = [0, np.inf, 0]
    q[9] = [0, 0, -np.inf]
    v = M.widen(q)
    keep = np.array([i for i in range(40) if i not in (far, 3, 9)])
    r = M.farthest_points(v, 6)
    sub = M.farthest_points(v[keep], 6)
    assert not set(r["idx"].tolist()) & {far, 3, 9}
    np.testing.assert_array_equal(keep[sub["idx"]], r["idx"])       # as if the absent rows were not there
    assert M.extent(v)["count"] == 37 and M.diameter(v) == M.diameter(v[keep])
    np.testing.assert_array_equal(M.extent(v)["bbox_min"], v[keep].min(0))
    # index mode: out of range or absent -> dead
    for s in (-1, 40, far, 3):
        d = M.farthest_points(v, 3, M.START_INDEX, s)
        assert d["idx"].tolist() == [-1] * 3 and np.isnan(d["picked"]).all() and np.isnan(d["pick_d2"]).all()
    # nothing finite, nothing at all, skipped
    for w in (M.widen(np.full((4, 3), np.nan)), np.zeros((0, 3)), None):
        assert M.farthest_points(w, 2)["idx"].tolist() == [-1, -1]
        assert M.extent(w)["count"] == 0 and np.isnan(M.extent(w)["centroid"]).all() and np.isnan(M.diameter(w))
    off = np.array([0, 10, 5, 40, 41], np.int32)                        # model 1: hi < lo; model 2: over max_pn
    assert M.model_rows(q, off, 0, 20).shape == (10, 3) and M.model_rows(q, off, 1, 20) is None
    assert M.model_rows(q, off, 2, 20) is None and M.model_rows(q, off, 3, 20) is None
    assert M.table_farthest_points(q, np.array([0, 10, 40], np.int32), 30, 2)["idx"].shape == (2, 2)


def test_centroid_lane_order():
    x = np.zeros(769)
    x[0], x[256], x[512] = 2.0 ** 60, 1.0, -2.0 ** 60
    assert M.lane_sum(x) == 0.0                                     # lane 0: (2^60 + 1) - 2^60 = 0
    y = np.zeros(769)
    y[0], y[1], y[512] = 2.0 ** 60, 1.0, -2.0 ** 60
    assert M.lane_sum(y) == 1.0                                     # the 1 sits in lane 1 and survives
