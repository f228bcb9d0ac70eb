"""The numpy restatement of include/pvrender.h (tests/render_ref.py) pinned by cases whose answers
are known without it: the fill rule by hand, shared edges and vertices counted once, a sphere's
silhouette against the analytic disk, and independence of face order and winding."""
import numpy as np

from tests import render_ref as R


def raster_px(points_px, faces, H, W, z=None):
    """Vertices given in pixels (multiples of 1/256), all at depth 1 unless z says otherwise."""
    sxy = np.round(np.asarray(points_px, np.float64) * 256).astype(np.int32)
    Z = np.ones(len(sxy)) if z is None else np.asarray(z, np.float64)
    return R.raster_instance(sxy, Z, np.asarray(faces), H, W)


def test_top_left_rule_by_hand():
    # (1,1) -> (5,1) is a top edge and (1,5) -> (1,1) a left edge: their samples are covered;
    # the hypotenuse x + y = 6 is neither, so its samples, the two far vertices included, are not
    want = np.zeros((7, 7), np.int32)
    want[1, 1:5] = 1
    want[2, 1:4] = 1
    want[3, 1:3] = 1
    want[4, 1:2] = 1
    for tri in ([0, 1, 2], [0, 2, 1], [2, 0, 1]):                     # either winding, any first vertex
        r = raster_px([(1, 1), (5, 1), (1, 5)], [tri], 7, 7)
        np.testing.assert_array_equal(r["count"], want)
        np.testing.assert_array_equal(np.isfinite(r["depth"]), want.astype(bool))
    # the mirror triangle owns the hypotenuse (a left edge for it) but not its bottom and right edges
    r = raster_px([(5, 1), (5, 5), (1, 5)], [[0, 1, 2]], 7, 7)
    want2 = np.zeros((7, 7), np.int32)
    want2[2, 4:5] = 1
    want2[3, 3:5] = 1
    want2[4, 2:5] = 1
    np.testing.assert_array_equal(r["count"], want2)
    assert not (want & want2).any()


def test_quad_split_either_way_covers_each_sample_once():
    quad = [(2, 1), (13, 3), (11.5, 10), (1.25, 8)]                    # convex; (2,1) and (13,3) sit on samples
    a = raster_px(quad, [[0, 1, 2], [0, 2, 3]], 12, 16)["count"]
    b = raster_px(quad, [[0, 1, 3], [1, 2, 3]], 12, 16)["count"]
    assert a.max() == 1 and b.max() == 1
    np.testing.assert_array_equal(a, b)
    assert a.sum() > 60
    # a diagonal through sample points: the square (2,2)..(8,8) split along x == y
    sq = [(2, 2), (8, 2), (8, 8), (2, 8)]
    c = raster_px(sq, [[0, 1, 2], [0, 2, 3]], 10, 10)["count"]
    d = raster_px(sq, [[0, 1, 3], [1, 2, 3]], 10, 10)["count"]
    want = np.zeros((10, 10), np.int32)
    want[2:8, 2:8] = 1                                                 # top and left edges in, bottom and right out
    np.testing.assert_array_equal(c, want)
    np.testing.assert_array_equal(d, want)


def test_fan_covers_its_centre_once():
    ang = np.linspace(0, 2 * np.pi, 7, endpoint=False) + 0.3
    ring = np.round(np.stack([6 + 4.3 * np.cos(ang), 6 + 4.3 * np.sin(ang)], 1) * 256) / 256
    pts = [(6, 6), *ring]
    faces = [[0, 1 + i, 1 + (i + 1) % 7] for i in range(7)]
    cnt = raster_px(pts, faces, 13, 13)["count"]
    assert cnt[6, 6] == 1 and cnt.max() == 1
    # spokes through samples: the axis-aligned fan of four
    cnt = raster_px([(6, 6), (10, 6), (6, 10), (2, 6), (6, 2)], [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], 13, 13)["count"]
    assert cnt[6, 6] == 1 and cnt.max() == 1 and cnt[6, 7] == 1 and cnt[7, 6] == 1


def test_sphere_silhouette_has_the_disk_area():
    H, W, f, r, d = 48, 64, 60.0, 0.05, 0.3
    K = np.array([[f, 0, 31.5], [0, f, 23.5], [0, 0, 1]])
    out = R.render([R.icosphere(3, r)], [(0, 1, R.pose(np.eye(3), [0, 0, d]))], K, H, W)
    radius = f * r / np.sqrt(d * d - r * r)                            # the tangent cone of a centred sphere
    area = int(np.count_nonzero(out["label"]))
    assert abs(area - np.pi * radius ** 2) <= 2 * np.pi * radius
    assert out["won"][0] == area and out["inst"].max() == 0
    # the nearest point of the sphere is at d - r, and nothing is nearer
    assert abs(float(out["depth"].min()) - (d - r)) < 1e-3 and out["depth"][0, 0] == np.inf


def test_face_order_and_winding_change_nothing():
    v, f = R.icosphere(2, 0.05)
    rng = np.random.default_rng(5)
    K = np.array([[70.0, 0, 31.3], [0, 71.0, 23.8], [0, 0, 1]])
    Rt = R.pose(R.random_rotation(rng), [0.01, -0.005, 0.32])
    a = R.render([(v, f)], [(0, 7, Rt)], K, 48, 64)
    g = f[rng.permutation(len(f))].copy()
    flip = rng.random(len(g)) < 0.5
    g[flip] = g[flip][:, [0, 2, 1]]
    b = R.render([(v, g)], [(0, 7, Rt)], K, 48, 64)
    for k in ("label", "inst", "depth"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["label"].max() == 7 and a["snap_margin"] > 0


def test_z_buffer_tie_goes_to_the_lower_instance():
    m = [R.box()]
    K = np.array([[80.0, 0, 31.5], [0, 80.0, 23.5], [0, 0, 1]])
    Rt = R.pose(R.random_rotation(np.random.default_rng(2)), [0, 0, 0.4])
    out = R.render(m, [(0, 3, Rt), (0, 9, Rt)], K, 48, 64)
    assert set(np.unique(out["label"])) == {0, 3} and out["won"][1] == 0 and out["won"][0] > 100
    assert out["depth_margin"] == 0.0


def test_vertex_field_per_class():
    label = np.zeros((6, 8), np.int32)
    label[1:3, 1:4] = 1
    label[3:5, 4:7] = 2
    label[5, 7] = 3                                                    # above class_num: background
    kp = np.array([[[2.0, 1.0], [9.5, -3.0]], [[0.0, 0.0], [5.0, 4.0]]])
    v = R.vertex_field(label, kp)
    assert v.shape == (6, 8, 4, 2) and v.dtype == np.float32
    assert not v[label == 0].any() and not v[5, 7].any()
    assert not v[label == 1][:, 2:].any() and not v[label == 2][:, :2].any()
    np.testing.assert_array_equal(v[1, 2, 0], [0.0, 0.0])              # the keypoint's own pixel
    np.testing.assert_allclose(v[4, 4, 3], [1.0, 0.0])
    np.testing.assert_allclose(np.linalg.norm(v[2, 3, :2], axis=1), 1.0, atol=1e-6)
