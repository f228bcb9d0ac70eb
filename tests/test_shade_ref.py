"""tests/shade_ref.py (the numpy restatement of include/pvshade.h) is fair, and the scenes the GPU
tests use are usable: no value sits on a rounding boundary and few pixels are contested.  CPU only."""
import numpy as np
import pytest

from tests import render_ref as R
from tests import shade_ref as S


@pytest.fixture(scope="module")
def refs():
    return {name: S.scene_reference(sc) for name, sc in S.scenes().items()}


def test_maps_equal_the_label_restatement(refs):
    for name, sc in S.scenes().items():
        plain = [m[:2] for m in S.models(sc["smooth"])]
        for i, f in enumerate(sc["frames"]):
            want = R.render(plain, f, sc["K"], sc["H"], sc["W"])
            got = refs[name][i]
            for k in ("label", "inst", "won"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} frame {i} {k}")
            np.testing.assert_array_equal(got["depth"].view(np.int32), want["depth"].view(np.int32))
            assert np.array_equal(got["face"] >= 0, want["label"] > 0) and np.array_equal(got["covered"], want["label"] > 0)


def test_scenes_are_usable(refs):
    """Conditions on the inputs, asserted here so the GPU test cannot hide a failure behind them."""
    for name, frames in refs.items():
        for i, r in enumerate(frames):
            fg = np.count_nonzero(r["covered"])
            assert fg > 100, (name, i)
            assert r["margin"][r["covered"]].min() >= 1e-9, (name, i, r["margin"][r["covered"]].min())
            assert np.isinf(r["margin"][~r["covered"]]).all()
            assert np.count_nonzero(r["contested"] & r["covered"]) <= 0.01 * fg, (name, i)
            assert len(np.unique(r["face"][r["covered"]])) > 5, (name, i)
    # the scenes reach the states their names promise
    r = refs["clamp_flat"][0]
    px = r["image"][r["covered"]]
    assert (px[:, 0] == 255).sum() > 20 and (px[:, 2] == 255).sum() > 50 and (px[:, 1] < 255).all()   # 1.37, 2.41 and 0.33
    assert len(np.unique(refs["occlusion3_smooth"][0]["inst"])) == 4


def test_reversing_the_winding_changes_no_pixel():
    for name in ("occlusion2_flat", "occlusion3_smooth"):
        sc = S.scenes()[name]
        ms = S.models(sc["smooth"])
        rev = [S.reverse_winding(m) for m in ms]
        f = sc["frames"][0]
        light = sc["lights"] if np.ndim(sc["lights"]) == 1 else sc["lights"][0]
        a = S.render(ms, f, sc["K"], sc["H"], sc["W"], light)
        b = S.render(rev, f, sc["K"], sc["H"], sc["W"], light)
        for k in ("image", "label", "inst", "face"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
        np.testing.assert_array_equal(a["depth"].view(np.int32), b["depth"].view(np.int32))
        assert a["covered"].sum() > 100


def test_constant_colour_under_ambient_one():
    v, f = R.icosphere(2, 0.05)
    col = np.tile(np.array([[200, 31, 97]], np.uint8), (len(v), 1))
    light = np.array([0.3, 0.1, -0.9, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    for normals in (None, S.vertex_normals(v, f)):
        r = S.render([(v, f, col, normals)], [(0, 1, S.seeded_poses(3, 1)[0])], S.K_SMALL, 48, 64, light, (1, 2, 3))
        assert r["covered"].sum() > 100
        assert (r["image"][r["covered"]] == [200, 31, 97]).all() and (r["image"][~r["covered"]] == [1, 2, 3]).all()


def test_lambert_on_a_face_on_plate():
    """A plate facing the camera, lit at 60 degrees: value = colour (ambient + diffuse / 2), everywhere."""
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 24.0], [0, 0, 1]])
    v = np.array([[-0.5, -0.25, 0], [0.5, -0.25, 0], [0.5, 0.25, 0], [-0.5, 0.25, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    col = np.tile(np.array([[200, 100, 40]], np.uint8), (4, 1))
    light = np.array([np.sqrt(3.0), 0.0, -1.0, 0.25, 0.25, 0.25, 0.5, 0.5, 0.5])
    for normals in (None, np.tile([[0.0, 0.0, -2.0]], (4, 1)), np.tile([[0.0, 0.0, 3.0]], (4, 1))):
        r = S.render([(v, f, col, normals)], [(0, 7, R.pose(np.eye(3), [0, 0, 2.0]))], K, 48, 64, light)
        want = np.zeros((48, 64), bool)
        want[16:32, 16:48] = True                                      # top and left edges in, bottom and right out
        np.testing.assert_array_equal(r["covered"], want)
        np.testing.assert_array_equal(r["face"][16:32, 16:48] >= 0, True)
        # cos 60 degrees = 0.5 up to rounding: 200 * 0.5 = 100, 100 * 0.5 = 50, 40 * 0.5 = 20
        assert (r["image"][want] == [100, 50, 20]).all() and (r["image"][~want] == 0).all()
    # lit from behind: ambient only
    back = light.copy()
    back[:3] = [0.0, 0.0, 1.0]
    r = S.render([(v, f, col, None)], [(0, 7, R.pose(np.eye(3), [0, 0, 2.0]))], K, 48, 64, back)
    assert (r["image"][want] == [50, 25, 10]).all()


def test_vertex_normals():
    v, f = R.icosphere(2, 1.0)
    n = S.vertex_normals(v, f)
    unit = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12 and (np.sum(n * unit, 1) > 0.99).all()   # outward on a sphere
    # an unused vertex gives zero; a face with an index out of range is skipped; a repeated index counts once
    v2 = np.concatenate([v, [[5.0, 5.0, 5.0]]]).astype(np.float32)
    f2 = np.concatenate([f, [[0, 1, len(v2)], [-1, 2, 3]]]).astype(np.int32)
    n2 = S.vertex_normals(v2, f2)
    np.testing.assert_array_equal(n2[:-1], n)
    assert (n2[-1] == 0).all()
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    np.testing.assert_array_equal(S.vertex_normals(tri, [[0, 1, 2], [0, 0, 1]]), np.tile([[0.0, 0.0, 1.0]], (3, 1)))


def test_contested_flag_and_the_tie_rule():
    """Two coplanar instances: the lower instance wins every pixel and every pixel is contested; a
    duplicated face: the lower face index wins."""
    box = S.colored(R.box(0.5, 0.25, 0.125), 1)
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 24.0], [0, 0, 1]])
    Rt = R.pose(np.eye(3), [0.0, 0.0, 2.125])
    r = S.render([box], [(0, 5, Rt), (0, 6, Rt)], K, 48, 64)
    assert (r["inst"][r["covered"]] == 0).all() and r["contested"][r["covered"]].all() and r["won"].tolist() == [512, 0]
    assert (r["depth"][r["covered"]] == 2.0).all()
    dup = (box[0], np.concatenate([box[1][:1], box[1]]), box[2], None)
    a, b = S.render([box], [(0, 5, Rt)], K, 48, 64), S.render([dup], [(0, 5, Rt)], K, 48, 64)
    np.testing.assert_array_equal(a["image"], b["image"])
    first = a["face"] == 0
    assert first.sum() > 50 and (b["face"][first] == 0).all() and (b["face"][a["face"] == 1] == 2).all()
