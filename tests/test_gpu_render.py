"""pvnet_amd.render on the device against the numpy restatement (tests/render_ref.py): snap parity,
exact coverage, the drop and skip rules, the z-buffer and its tie rule, determinism under graph
capture, the vector field, and the closed loop pose -> labels and field -> votes -> EPnP -> pose."""
import numpy as np
import pytest
import torch

from pvnet_amd import synth
from tests import render_ref as R

pytestmark = pytest.mark.gpu

K_SMALL = np.array([[70.0, 0.0, 31.5], [0.0, 71.5, 23.5], [0.0, 0.0, 1.0]])
K_SKEW = np.array([[40.0, 0.7, 26.1], [0.0, 41.0, 18.2], [0.0, 0.0, 1.0]])
INVALID = -2 ** 31


@pytest.fixture(scope="module")
def Rn(device):
    import __graft_entry__ as g
    g.build()
    from pvnet_amd import render
    return render


@pytest.fixture(scope="module")
def meshes():
    return [R.box(), R.icosphere(2, 0.05), R.bumpy_ellipsoid(2), R.icosphere(3, 0.05)]


def seeded_poses(seed, n, spread=0.03, near=0.3, far=0.5):
    rng = np.random.default_rng(seed)
    return [R.pose(R.random_rotation(rng), [rng.uniform(-spread, spread), rng.uniform(-spread, spread),
                                            rng.uniform(near, far)]) for _ in range(n)]


def cu(a, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(device)


def run(Rn, device, models, frames, K, H, W, znear=1e-3, table=None, **kw):
    """frames: per frame a list of (model_id, label, Rt), all frames the same length -> the three
    maps, won [b, n] and the snapped vertices per instance as numpy (one synchronisation)."""
    table = table or Rn.MeshTable(models, device=device)
    b, n = len(frames), len(frames[0])
    poses = cu(np.array([[i[2] for i in f] for f in frames], np.float64).reshape(b, n, 3, 4), device)
    mid = np.array([[i[0] for i in f] for f in frames], np.int64).reshape(b, n)
    lab = np.array([[i[1] for i in f] for f in frames], np.int64).reshape(b, n)
    diag = {}
    out = Rn.render_labels(table, poses, cu(mid, device), cu(lab, device), cu(K, device), H, W, znear, diag=diag, **kw)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["won"] = diag["won"].cpu().numpy().reshape(b, n)
    res["snap_xy"] = diag["snap_xy"].cpu().numpy().reshape(b, n, table.max_verts, 2)
    res["snap_z"] = diag["snap_z"].cpu().numpy().reshape(b, n, table.max_verts)
    return res


def reference(models, frames, K, H, W, dev=None, znear=1e-3):
    """The restatement per frame; with dev (run()'s result) it rasterises the device's own snapped vertices."""
    refs = []
    for i, f in enumerate(frames):
        snapped = None
        if dev is not None:
            snapped = []
            for j, (mid, _, _) in enumerate(f):
                nv = len(models[mid][0]) if 0 <= mid < len(models) else 0
                snapped.append((dev["snap_xy"][i, j, :nv], dev["snap_z"][i, j, :nv]))
        refs.append(R.render(models, f, K if np.ndim(K) == 2 else K[i], H, W, znear, snapped=snapped))
    return refs


def ulp_apart(a, b):
    """Distance in f32 representations (equal infinities are 0 apart)."""
    ai, bi = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ai - bi)


def assert_frames_equal(dev, refs, depth_ulps=1):
    for i, r in enumerate(refs):
        np.testing.assert_array_equal(dev["label"][i], r["label"], err_msg=f"label, frame {i}")
        np.testing.assert_array_equal(dev["inst"][i], r["inst"], err_msg=f"inst, frame {i}")
        np.testing.assert_array_equal(dev["won"][i], r["won"], err_msg=f"won, frame {i}")
        assert ulp_apart(dev["depth"][i], r["depth"]).max() <= depth_ulps, f"depth, frame {i}"
        assert np.array_equal(np.isinf(dev["depth"][i]), r["label"] == 0)


# ---- 1. snap parity ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,K", [(48, 64, K_SMALL), (37, 53, K_SKEW)])
def test_snap_parity(device, Rn, meshes, H, W, K):
    models = meshes[:3]
    poses = [seeded_poses(100 + m, 8) for m in range(3)]
    frames = [[(m, m + 1, poses[m][i]) for m in range(3)] for i in range(8)]
    dev = run(Rn, device, models, frames, K, H, W)
    for i, f in enumerate(frames):
        for j, (mid, _, Rt) in enumerate(f):
            s = R.project_snap(models[mid][0], Rt, K, 1e-3)
            assert s["margin"] >= 1e-6 and s["ok"].all()               # a condition on the inputs, met by these seeds
            nv = len(models[mid][0])
            np.testing.assert_array_equal(dev["snap_xy"][i, j, :nv], s["sxy"])
            np.testing.assert_allclose(dev["snap_z"][i, j, :nv], s["Z"], rtol=1e-15, atol=0)


# ---- 2. coverage -------------------------------------------------------------------------------------
def face_on_box():
    """A box whose front face projects onto integer pixels: corners (16, 16), (48, 16), (48, 32), (16, 32)."""
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 24.0], [0, 0, 1]])
    return R.box(0.5, 0.25, 0.125), R.pose(np.eye(3), [0.0, 0.0, 2.125]), K


def test_coverage_box_face_on(device, Rn):
    box, Rt, K = face_on_box()
    frames = [[(0, 5, Rt)]]
    dev = run(Rn, device, [box], frames, K, 48, 64)
    front = dev["snap_xy"][0, 0, :4]
    assert sorted(map(tuple, front.tolist())) == sorted([(16 * 256, 16 * 256), (48 * 256, 16 * 256), (16 * 256, 32 * 256),
                                                         (48 * 256, 32 * 256)])
    refs = reference([box], frames, K, 48, 64, dev)
    assert_frames_equal(dev, refs)
    want = np.zeros((48, 64), np.int32)
    want[16:32, 16:48] = 5                                             # top and left edges in, bottom and right out
    np.testing.assert_array_equal(dev["label"][0], want)
    assert (dev["depth"][0][want > 0] == 2.0).all() and dev["won"][0, 0] == 16 * 32


@pytest.mark.parametrize("H,W,K", [(48, 64, K_SMALL), (37, 53, K_SKEW)])
def test_coverage_small_triangles(device, Rn, meshes, H, W, K):
    """The 1,280-triangle sphere: sub-pixel and few-pixel triangles, many covering no sample;
    53 is no multiple of 8 or 64."""
    models = [meshes[3], meshes[2]]
    frames = [[(0, 1, p)] for p in seeded_poses(7, 2, near=0.18, far=0.3)] + [[(1, 2, p)] for p in seeded_poses(8, 2)]
    dev = run(Rn, device, models, frames, K, H, W)
    refs = reference(models, frames, K, H, W, dev)
    assert_frames_equal(dev, refs)
    assert all(r["won"][0] > 30 for r in refs)


def test_coverage_borders_and_huge_triangle(device, Rn, meshes):
    tri = (np.array([[-10, -10, 0], [10, -10, 0], [0, 15, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    models = [meshes[1], tri]
    H, W, K = 37, 53, K_SKEW
    t = [(-0.33, 0, 0.5), (0.32, 0.01, 0.5), (0.0, -0.22, 0.5), (0.01, 0.23, 0.5), (3.0, 0.0, 0.5), (0.0, -2.0, 0.5)]
    frames = [[(0, 9, R.pose(np.eye(3), ti))] for ti in t] + [[(1, 200, R.pose(np.eye(3), [0.3, -0.2, 1.0]))]]
    dev = run(Rn, device, models, frames, K, H, W)
    refs = reference(models, frames, K, H, W, dev)
    assert_frames_equal(dev, refs)
    for i, (col, row) in enumerate([(0, H // 2), (W - 1, H // 2), (W // 2, 0), (W // 2, H - 1)]):
        assert 0 < refs[i]["won"][0] < 150 and refs[i]["label"][row, col] == 9, i   # cut by that border
    assert refs[4]["won"][0] == 0 and refs[5]["won"][0] == 0          # wholly outside
    assert (dev["label"][6] == 200).all() and dev["won"][6, 0] == H * W  # larger than the image


def test_coverage_one_pixel_image(device, Rn):
    box, Rt, _ = face_on_box()
    K = np.array([[64.0, 0, 0.0], [0, 64.0, 0.0], [0, 0, 1]])
    frames = [[(0, 1, Rt)], [(0, 1, R.pose(np.eye(3), [5.0, 0, 2.125]))]]
    dev = run(Rn, device, [box], frames, K, 1, 1)
    assert_frames_equal(dev, reference([box], frames, K, 1, 1, dev))
    assert dev["label"].tolist() == [[[1]], [[0]]] and dev["inst"].tolist() == [[[0]], [[-1]]]


# ---- 3. drop and skip rules ----------------------------------------------------------------------------
def test_drop_and_skip_rules(device, Rn, meshes):
    v, f = meshes[1]
    nv = len(v)
    v_bad = np.concatenate([v, [[0.0, 0.0, -1.0]]]).astype(np.float32)              # lands behind the camera
    extra = np.array([[0, 0, 5], [3, 3, 3], [0, nv + 7, 5], [-1, 2, 3], [2 ** 30, 1, 2], [nv, 0, 1], [4, nv, 9]], np.int32)
    f_bad = np.concatenate([f[:100], extra, f[100:]])
    # a collinear triple: three copies of one vertex's direction would not snap collinear; reuse an edge instead
    f_bad = np.concatenate([f_bad, [[f[0, 0], f[0, 1], f[0, 0]]]]).astype(np.int32)
    models = [(v_bad, f_bad), meshes[0]]
    clean = [(v, f), meshes[0]]
    nan_pose = R.pose(np.eye(3), [0, 0, 0.4])
    nan_pose[1, 2] = np.nan
    inf_pose = R.pose(np.eye(3), [0, np.inf, 0.4])
    A, B = R.pose(np.eye(3), [-0.04, 0.0, 0.4]), R.pose(seeded_poses(3, 1)[0][:, :3], [0.05, 0.01, 0.45])
    H, W, K = 48, 64, K_SMALL
    frames = [[(0, 1, A), (7, 2, A), (1, 3, B), (0, 4, nan_pose)],
              [(-1, 5, A), (1, 6, B), (0, 7, inf_pose), (0, 8, A)]]
    dev = run(Rn, device, models, frames, K, H, W)
    refs = reference(models, frames, K, H, W, dev)
    assert_frames_equal(dev, refs)
    # ... and the frame equals the restatement with those items removed
    kept = [[(0, 1, A), (1, 3, B)], [(1, 6, B), (0, 8, A)]]
    index = [[0, 2], [1, 3]]
    for i, r in enumerate(reference(clean, kept, K, H, W)):
        np.testing.assert_array_equal(dev["label"][i], r["label"])
        assert ulp_apart(dev["depth"][i], r["depth"]).max() <= 1
        np.testing.assert_array_equal(dev["inst"][i], np.where(r["inst"] < 0, -1, np.take(index[i], r["inst"])))
        assert dev["won"][i].tolist() == [int(r["won"][index[i].index(j)]) if j in index[i] else 0 for j in range(4)]
        assert r["won"].min() > 50
    # the vertex behind znear is marked, and drops only its own triangles
    assert (dev["snap_xy"][0, 0, nv] == INVALID).all() and (dev["snap_xy"][0, 0, :nv] != INVALID).all()


def test_znear_drops_whole_triangles(device, Rn, meshes):
    models = [meshes[1]]
    frames = [[(0, 1, R.pose(np.eye(3), [0, 0, 0.4]))]]
    dev = run(Rn, device, models, frames, K_SMALL, 48, 64, znear=0.4)    # the sphere's centre plane
    refs = reference(models, frames, K_SMALL, 48, 64, dev, znear=0.4)
    assert_frames_equal(dev, refs)
    assert dev["won"][0, 0] > 50 and dev["depth"][0][dev["label"][0] > 0].min() >= 0.4


def test_zero_instances_is_background(device, Rn, meshes):
    table = Rn.MeshTable(meshes[:1], device=device)
    out = Rn.render_labels(table, torch.zeros((2, 0, 3, 4), dtype=torch.float64, device=device),
                           np.zeros((2, 0), np.int64), None, cu(K_SMALL, device), 37, 53)
    assert (out["label"] == 0).all() and (out["inst"] == -1).all() and torch.isinf(out["depth"]).all()
    assert out["label"].dtype == torch.uint8 and tuple(out["inst"].shape) == (2, 37, 53)
    empty = Rn.render_labels(table, torch.zeros((0, 3, 3, 4), dtype=torch.float64, device=device),
                             np.zeros((0, 3), np.int64), None, cu(K_SMALL, device), 37, 53)
    assert tuple(empty["depth"].shape) == (0, 37, 53)


def test_instance_offsets_cameras_per_frame_and_label_kinds(device, Rn, meshes):
    """The ([total, 3, 4], inst_off) form with 2, 0, 3 and 1 instances per frame, a camera per frame,
    every label kind; a frame whose range runs backwards has no instances."""
    two, three = occlusion_frames()
    frames = [two[0], [], three[1], [(2, 40, seeded_poses(9, 1)[0])]]
    Ks = np.stack([K_SMALL, K_SKEW, K_SMALL + np.array([[3.0, 0.2, -1.5], [0, -2.0, 2.25], [0, 0, 0]]), K_SKEW])
    H, W = 37, 53
    flat = [i for f in frames for i in f]
    off = np.cumsum([0] + [len(f) for f in frames])
    table = Rn.MeshTable(meshes, device=device)
    poses = cu(np.array([i[2] for i in flat]), device)
    mid, lab = [i[0] for i in flat], [i[1] for i in flat]
    refs = [R.render(meshes, f, Ks[i], H, W) for i, f in enumerate(frames)]
    assert all(r["snap_margin"] >= 1e-6 for r in refs) and refs[0]["won"].min() > 0 and refs[2]["won"].min() > 0
    for dt in (torch.uint8, torch.int32, torch.int64):
        diag = {}
        out = Rn.render_labels(table, (poses, off), mid, lab, cu(Ks, device), H, W, label_dtype=dt, diag=diag)
        assert out["label"].dtype == dt and tuple(out["label"].shape) == (4, H, W)
        won = diag["won"].cpu().numpy()
        for i, r in enumerate(refs):
            np.testing.assert_array_equal(out["label"][i].cpu().numpy(), r["label"])
            np.testing.assert_array_equal(out["inst"][i].cpu().numpy(), r["inst"])
            assert ulp_apart(out["depth"][i].cpu().numpy(), r["depth"]).max() <= 1
            np.testing.assert_array_equal(won[off[i]:off[i + 1]], r["won"])
    assert (out["label"][1] == 0).all()
    bad = off.copy()
    bad[1] = 7                                                         # frame 0 = [0, 7) overruns, frame 1 = [7, 2) runs backwards
    out = Rn.render_labels(table, (poses, bad), mid, lab, cu(Ks, device), H, W)
    assert (out["label"][:2] == 0).all() and (out["inst"][:2] == -1).all()
    np.testing.assert_array_equal(out["label"][2].cpu().numpy(), refs[2]["label"])


# ---- 4. z-buffer -----------------------------------------------------------------------------------------
def occlusion_frames():
    """Two and three instances with real occlusion; frame 1 has interpenetrating spheres."""
    I = np.eye(3)
    rot = seeded_poses(21, 3)
    two = [[(1, 1, R.pose(I, [-0.01, 0.0, 0.40])), (0, 2, R.pose(rot[0][:, :3], [0.02, 0.01, 0.33]))],
           [(1, 3, R.pose(I, [-0.015, 0.0, 0.40])), (3, 4, R.pose(rot[1][:, :3], [0.02, 0.01, 0.42]))]]
    three = [[(1, 1, R.pose(I, [-0.03, 0.0, 0.40])), (3, 2, R.pose(rot[2][:, :3], [0.03, 0.0, 0.43])),
              (2, 3, R.pose(rot[0][:, :3], [0.0, 0.01, 0.36]))],
             [(2, 7, R.pose(rot[1][:, :3], [0.0, -0.035, 0.45])), (0, 8, R.pose(rot[2][:, :3], [0.04, 0.0, 0.38])),
              (1, 9, R.pose(I, [-0.035, 0.01, 0.41]))]]
    return two, three


@pytest.mark.parametrize("which", [0, 1])
def test_z_buffer_occlusion(device, Rn, meshes, which):
    frames = occlusion_frames()[which]
    H, W, K = 48, 64, K_SMALL
    dev = run(Rn, device, meshes, frames, K, H, W)
    refs = reference(meshes, frames, K, H, W, dev)
    for i, r in enumerate(refs):
        fg = r["label"] > 0
        sure = r["depth_margin_map"] >= 1e-9
        assert np.count_nonzero(fg & ~sure) <= 1e-3 * np.count_nonzero(fg)      # a condition on the scene
        assert all(0 < w < np.count_nonzero(fg) for w in r["won"])           # every instance visible, none alone
        overlap = np.isfinite(r["depth_margin_map"])
        assert np.count_nonzero(overlap) > 100                                 # real occlusion
        np.testing.assert_array_equal(dev["label"][i][sure], r["label"][sure])
        np.testing.assert_array_equal(dev["inst"][i][sure], r["inst"][sure])
        assert ulp_apart(dev["depth"][i][sure], r["depth"][sure]).max() <= 1
    if which == 0:
        # the spheres of frame 1 interpenetrate: each owns part of the overlap
        r = refs[1]
        overlap = np.isfinite(r["depth_margin_map"])
        assert {0, 1} <= set(np.unique(r["inst"][overlap]).tolist())


def test_z_buffer_exact_tie(device, Rn, meshes):
    Rt = seeded_poses(33, 1)[0]
    frames = [[(2, 11, Rt), (2, 12, Rt)], [(0, 4, Rt), (0, 3, Rt)]]
    dev = run(Rn, device, meshes, frames, K_SMALL, 48, 64)
    for i, owner in enumerate((11, 4)):
        assert set(np.unique(dev["label"][i]).tolist()) == {0, owner}
        assert set(np.unique(dev["inst"][i]).tolist()) == {-1, 0}
        assert dev["won"][i, 1] == 0 and dev["won"][i, 0] == np.count_nonzero(dev["label"][i]) > 100
    assert_frames_equal(dev, reference(meshes, frames, K_SMALL, 48, 64, dev))


def test_permuting_instances_permutes_inst_only(device, Rn, meshes):
    frame = occlusion_frames()[1][1]
    r = R.render(meshes, frame, K_SMALL, 48, 64)
    assert r["depth_margin"] > 4 * 2.0 ** -23                                  # no two instances tie in f32
    base = run(Rn, device, meshes, [frame], K_SMALL, 48, 64)
    for perm in ([2, 0, 1], [1, 2, 0], [0, 2, 1]):
        dev = run(Rn, device, meshes, [[frame[p] for p in perm]], K_SMALL, 48, 64)
        np.testing.assert_array_equal(dev["label"], base["label"])
        np.testing.assert_array_equal(dev["depth"].view(np.int32), base["depth"].view(np.int32))
        np.testing.assert_array_equal(np.where(dev["inst"] < 0, -1, np.take(perm, dev["inst"])), base["inst"])
        np.testing.assert_array_equal(dev["won"][0], base["won"][0][perm])


# ---- 5. determinism and capture -----------------------------------------------------------------------------
def test_determinism_capture_and_batching(device, Rn, meshes):
    two, three = occlusion_frames()
    frames = [three[0], three[1], [*two[1], (0, 5, seeded_poses(4, 1)[0])]]
    H, W = 37, 53
    table = Rn.MeshTable(meshes, device=device)
    poses = cu(np.array([[i[2] for i in f] for f in frames]), device)
    mid = cu(np.array([[i[0] for i in f] for f in frames]), device, torch.int32)
    lab = cu(np.array([[i[1] for i in f] for f in frames]), device, torch.int32)
    K = cu(K_SKEW, device)

    def maps(**kw):
        return Rn.render_labels(table, poses, mid, lab, K, H, W, **kw)

    def bits(d):
        return {k: v.cpu().numpy().view(np.uint8 if k == "label" else np.int32) for k, v in d.items()}

    a, b2 = bits(maps()), bits(maps())
    assert a["label"].any()
    for k in ("label", "inst", "depth"):
        np.testing.assert_array_equal(a[k], b2[k])
    # a batch of 3 frames equals the three frames rendered one at a time
    for i in range(3):
        one = bits(Rn.render_labels(table, poses[i:i + 1], mid[i:i + 1], lab[i:i + 1], K, H, W))
        for k in ("label", "inst", "depth"):
            np.testing.assert_array_equal(one[k][0], a[k][i])
    # captured on a side stream and replayed twice, all three maps and the label alone
    for want in (("label", "inst", "depth"), ("label",)):
        out = {w: torch.zeros((3, H, W), dtype={"label": torch.uint8, "inst": torch.int32, "depth": torch.float32}[w],
                              device=device) for w in want}
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            with torch.cuda.graph(gph, stream=side):
                maps(want=want, out=out)
        for _ in range(2):
            for t in out.values():
                t.fill_(77)
            gph.replay()
            torch.cuda.synchronize()
            got = bits(out)
            assert set(got) == set(want)
            for k in want:
                np.testing.assert_array_equal(got[k], a[k])


# ---- 6. the vector field ------------------------------------------------------------------------------------
def blob_labels(b, H, W, top, seed):
    """Label maps with labels 0..top in blobs (labels above class_num among them when top is larger)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((b, H, W), np.int64)
    for i in range(b):
        for v in range(1, top + 1):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(4, 0.3 * W)
            lab[i][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = v
        for v in range(top + 1):                                       # every label, 0 included, keeps some pixels
            lab[i, 2 + 3 * v:4 + 3 * v, 3:9] = v
    return lab


@pytest.fixture(scope="module")
def field_cases():
    """(H, W, class_num, vn) -> (labels i64 [2, H, W], keypoints f64 [2, class_num, vn, 2], reference f32
    [2, H, W, class_num * vn, 2]), computed once."""
    cases = {}
    for H, W, ncls, vn in [(37, 53, 1, 1), (37, 53, 1, 9), (37, 53, 3, 9), (37, 53, 3, 1), (48, 64, 2, 9), (48, 64, 3, 9)]:
        lab = blob_labels(2, H, W, ncls + 1, 50 + ncls * 10 + vn)
        rng = np.random.default_rng(ncls * 100 + vn)
        kp = rng.uniform([-10.0, -10.0], [W + 10.0, H + 10.0], size=(2, ncls, vn, 2))
        for i in range(2):                                             # a keypoint exactly on a pixel of its class
            for c in range(ncls):
                ys, xs = np.nonzero(lab[i] == c + 1)
                assert len(ys) > 0
                kp[i, c, 0] = (xs[len(xs) // 2], ys[len(ys) // 2])
        ref = np.stack([R.vertex_field(lab[i], kp[i]) for i in range(2)])
        assert (lab == ncls + 1).any() and (lab == 0).any()
        cases[(H, W, ncls, vn)] = (lab, kp, ref)
    return cases


LABEL_DTYPES = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}


@pytest.mark.parametrize("layout", ["bhwk2", "network"])
@pytest.mark.parametrize("shape", [(37, 53, 1, 1), (37, 53, 1, 9), (37, 53, 3, 9), (37, 53, 3, 1), (48, 64, 2, 9),
                                   (48, 64, 3, 9)])
def test_vertex_field_f32(device, Rn, field_cases, shape, layout):
    lab, kp, ref = field_cases[shape]
    H, W, ncls, vn = shape
    C = ncls * vn
    for name, dt in LABEL_DTYPES.items():
        out = Rn.vertex_field(cu(lab, device, dt), cu(kp, device), ncls, layout=layout)
        assert out.dtype == torch.float32 and out.is_contiguous()
        got = out.cpu().numpy()
        if layout == "network":
            assert got.shape == (2, 2 * C, H, W)
            got = got.transpose(0, 2, 3, 1).reshape(2, H, W, C, 2)
        assert np.abs(got.astype(np.float64) - ref).max() <= 2.0 ** -23, name
        zero = ref == 0                                                # background, other classes, labels above class_num
        assert (got[zero] == 0).all() and zero.mean() > 0.3
        for i in range(2):
            for c in range(ncls):
                x, y = kp[i, c, 0].astype(int)
                assert (got[i, y, x, c * vn] == 0).all()               # the n < 1e-3 branch
    kp32 = Rn.vertex_field(cu(lab, device, torch.int32), cu(kp.astype(np.float32), device), ncls, layout=layout)
    ref32 = np.stack([R.vertex_field(lab[i], kp[i].astype(np.float32).astype(np.float64)) for i in range(2)])
    got = kp32.cpu().numpy()
    if layout == "network":
        got = got.transpose(0, 2, 3, 1).reshape(2, H, W, C, 2)
    assert np.abs(got.astype(np.float64) - ref32).max() <= 2.0 ** -23


@pytest.mark.parametrize("layout", ["bhwk2", "network"])
@pytest.mark.parametrize("shape", [(37, 53, 3, 9), (48, 64, 2, 9), (48, 64, 3, 9), (37, 53, 1, 1)])
def test_vertex_field_f16(device, Rn, field_cases, shape, layout):
    lab, kp, ref = field_cases[shape]
    H, W, ncls, vn = shape
    C = ncls * vn
    out = Rn.vertex_field(cu(lab, device, torch.uint8), cu(kp, device), ncls, dtype=torch.float16, layout=layout)
    assert out.dtype == torch.float16
    got = out.cpu().numpy()
    if layout == "network":
        got = got.transpose(0, 2, 3, 1).reshape(2, H, W, C, 2)
    want = ref.astype(np.float32).astype(np.float16)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert (got[ref == 0] == 0).all()


@pytest.mark.parametrize("layout", ["bhwk2", "network"])
def test_vertex_field_overwrites_a_strided_output(device, Rn, field_cases, layout):
    lab, kp, ref = field_cases[(48, 64, 2, 9)]
    H, W, C = 48, 64, 18
    if layout == "bhwk2":
        big = torch.full((2, H, W, C + 3, 2), float("nan"), device=device)
        view = big[:, :, :, 1:C + 1]
    else:
        big = torch.full((2, 2 * C + 1, H, W + 4), float("nan"), device=device)
        view = big[:, 1:, :, 2:W + 2]
    assert not view.is_contiguous()
    res = Rn.vertex_field(cu(lab, device, torch.uint8), cu(kp, device), 2, layout=layout, out=view)
    assert res.data_ptr() == view.data_ptr()
    got = view.cpu().numpy()
    if layout == "network":
        got = got.transpose(0, 2, 3, 1).reshape(2, H, W, C, 2)
    assert np.isfinite(got).all() and np.abs(got.astype(np.float64) - ref).max() <= 2.0 ** -23
    assert int(torch.isnan(big).sum()) == big.numel() - view.numel()    # and nothing outside the view
    # a contiguous output pre-filled with NaN comes back fully overwritten too
    full = torch.full((2, H, W, C, 2) if layout == "bhwk2" else (2, 2 * C, H, W), float("nan"), device=device)
    Rn.vertex_field(cu(lab, device, torch.uint8), cu(kp, device), 2, layout=layout, out=full)
    assert not torch.isnan(full).any()


def test_vertex_field_more_rows_than_a_grid_dimension(device, Rn):
    """65,536 rows: the pixel-major kernel's (chunks, rows, images) grid does not fit, and its linear form runs."""
    H = 65536
    lab = np.zeros((1, H, 1), np.int64)
    lab[0, 100:60000:7, 0] = 1
    lab[0, -1, 0] = 1
    kp = np.array([[[[0.25, 30000.5], [-3.0, 70000.0]]]])
    ref = R.vertex_field(lab[0], kp[0])[None]
    out = Rn.vertex_field(cu(lab, device, torch.int32), cu(kp, device), 1)
    got = out.cpu().numpy()
    assert got.shape == (1, H, 1, 2, 2) and np.abs(got.astype(np.float64) - ref).max() <= 2.0 ** -23
    assert (got[ref == 0] == 0).all() and np.abs(got[0, -1, 0]).max() > 0.9


# ---- 7. the loop closes ----------------------------------------------------------------------------------------
def loop_scene():
    """4 frames of 480 x 640 with the LINEMOD camera, two objects per frame (the bumpy ellipsoid and the
    box, 9 keypoints each); in frames 2 and 3 one partly occludes the other."""
    models = [R.bumpy_ellipsoid(3), R.box(0.05, 0.04, 0.03)]
    p3 = np.stack([R.spread_keypoints(m[0], 8) for m in models])
    rot = [p[:, :3] for p in seeded_poses(77, 8)]
    t = [[(-0.09, -0.03, 0.75), (0.10, 0.04, 0.80)], [(0.08, 0.05, 0.90), (-0.10, -0.04, 0.70)],
         [(0.00, 0.00, 0.80), (0.045, 0.01, 0.68)], [(0.02, 0.01, 0.66), (-0.035, 0.015, 0.82)]]
    poses = np.array([[R.pose(rot[2 * i + c], t[i][c]) for c in range(2)] for i in range(4)])
    diam = [float(np.max(np.linalg.norm(m[0][:, None].astype(np.float64) - m[0][None], axis=2))) for m in models]
    return dict(models=models, p3=p3, poses=poses, diameter=diam, K=synth.LINEMOD_K, H=480, W=640)


# The CPU chain on these frames (the restatement's label map and field -> the oracle's voting with 512
# hypotheses -> tests/epnp_ref.py), worst over the 8 (frame, class) pairs against the poses rendered;
# DESIGN 10d records the run.  The device's bounds are 4 x these: the factor covers the two sides'
# different hypothesis draws.
CPU_WORST = dict(keypoint_px=1.595e-4, add_over_diameter=5.232e-6, proj_px=4.441e-5)


def test_loop_closes(device, Rn):
    from pvnet_amd import evaluation_utils as EU
    from pvnet_amd import extend_utils as X
    from pvnet_amd import ransac_voting_gpu as rvg
    s = loop_scene()
    H, W, K = s["H"], s["W"], cu(s["K"], device)
    table = Rn.MeshTable(s["models"], device=device)
    poses = cu(s["poses"], device)
    mid = torch.tensor([0, 1], dtype=torch.int32, device=device)
    label, vertex, kp_true = Rn.render_ground_truth(table, s["p3"], poses, mid, K, H, W)
    assert tuple(label.shape) == (4, H, W) and tuple(vertex.shape) == (4, H, W, 18, 2) and tuple(kp_true.shape) == (4, 2, 9, 2)
    np.testing.assert_allclose(kp_true.cpu().numpy()[1, 1], synth.project(s["p3"][1], s["poses"][1, 1]), atol=1e-9)
    area = torch.stack([(label == c + 1).sum((1, 2)) for c in range(2)], 1).cpu().numpy()
    assert area.min() > 1000                                            # both objects visible in every frame

    kp = rvg.ransac_voting_layer_v3_multi(label, vertex, 2, 512, _seed=20240)
    p3 = cu(s["p3"], device)[None].expand(4, 2, 9, 3).reshape(8, 9, 3)
    est = X.pnp_batch(kp.reshape(8, 9, 2).to(torch.float64), p3, K, method="epnp")
    gt = poses.reshape(8, 3, 4)
    ids = mid.repeat(4)
    etable = EU.ModelTable([(m[0], d, False) for m, d in zip(s["models"], s["diameter"])], device=device)
    m = EU.pose_metrics(est, gt, etable, K, ids, metrics=("add", "proj"))
    kp_err = float((kp.to(torch.float64) - kp_true).norm(dim=-1).max())
    diam = np.array(s["diameter"])[[0, 1] * 4]
    add, proj = m["add"].cpu().numpy() / diam, m["proj"].cpu().numpy()
    print(f"loop: keypoints {kp_err:.3e} px, ADD/diameter {add.max():.3e}, projection {proj.max():.3e} px")
    # (b) every pose passes the usual thresholds
    assert (add < 0.1).all() and (proj < 5.0).all()
    # (a) ... and is as good as the CPU chain's, within the factor for the draws
    assert kp_err <= 4 * CPU_WORST["keypoint_px"]
    assert add.max() <= 4 * CPU_WORST["add_over_diameter"]
    assert proj.max() <= 4 * CPU_WORST["proj_px"]
    # (c) the estimated poses redraw the label map
    again = Rn.render_labels(table, est.reshape(4, 2, 3, 4), mid, None, K, H, W, want=("label",))["label"]
    iou = Rn.mask_iou(again, label, 2).cpu().numpy()
    print("loop: mask IoU", iou.min())
    assert iou.shape == (4, 2) and (iou >= 0.98).all()
    # occlusion is real in frames 2 and 3: the label map has fewer pixels of the far object than its own render
    for i, far in ((2, 0), (3, 1)):
        alone = Rn.render_labels(table, poses[i:i + 1, far:far + 1], mid[far:far + 1], None, K, H, W, want=("label",))["label"]
        assert int((alone > 0).sum()) > area[i, far] + 200


# ---- 8. the Python layer's errors ----------------------------------------------------------------------------------
def test_python_errors(device, Rn, meshes):
    table = Rn.MeshTable(meshes[:2], device=device)
    host_table = Rn.MeshTable(meshes[:2], device="cpu")
    poses = torch.zeros((2, 2, 3, 4), dtype=torch.float64, device=device)
    K = cu(K_SMALL, device)
    ok = dict(model_id=[0, 1], labels=[1, 2], K=K, H=16, W=16)

    def bad(match, table=table, poses=poses, **kw):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(RuntimeError, match=match):
            Rn.render_labels(table, poses, a["model_id"], a["labels"], a["K"], a["H"], a["W"],
                             **{k: v for k, v in a.items() if k not in ok})

    bad("device", poses=poses.cpu())
    bad("same device", table=host_table)
    bad("poses must be", poses=poses[0])
    bad("poses must be", poses=poses[..., :3])
    bad("model_id must be", model_id=[0, 1, 1])
    bad("labels must be", labels=[[1, 2, 3]] * 2)
    bad("1..255", labels=[0, 1])
    bad("1..255", labels=[1, 256])
    bad("K must be", K=np.eye(4))
    bad("K must be", K=np.zeros((3, 3, 3)))
    bad("H and W", H=0)
    bad("znear", znear=0.0)
    bad("want", want=())
    bad("want", want=("label", "normals"))
    bad("out", out={"label": torch.zeros((2, 16, 16), dtype=torch.uint8)})
    bad("out", out={"depth": torch.zeros((2, 16, 17), device=device)})
    bad("MeshTable", table=object())
    lab = torch.zeros((2, 16, 16), dtype=torch.uint8, device=device)
    kp = torch.zeros((2, 2, 9, 2), dtype=torch.float64, device=device)
    for match, args, kw in [("device", (lab.cpu(), kp, 2), {}), ("same device", (lab, kp.cpu(), 2), {}),
                            ("keypoints_2d", (lab, kp, 3), {}), ("keypoints_2d", (lab, kp[0], 2), {}),
                            ("label must be", (lab.float(), kp, 2), {}), ("label must be", (lab[0], kp, 2), {}),
                            ("dtype", (lab, kp, 2), dict(dtype=torch.float64)), ("layout", (lab, kp, 2), dict(layout="nchw")),
                            ("out must be", (lab, kp, 2), dict(out=torch.zeros((2, 16, 16, 18, 3), device=device))),
                            ("class_num", (lab, kp, 0), {})]:
        with pytest.raises(RuntimeError, match=match):
            Rn.vertex_field(*args, **kw)
    with pytest.raises(RuntimeError, match="points_3d"):
        Rn.render_ground_truth(table, np.zeros((3, 9, 3)), poses, [0, 1], K, 16, 16)
    with pytest.raises(RuntimeError, match="poses"):
        Rn.render_ground_truth(table, np.zeros((2, 9, 3)), (poses.reshape(4, 3, 4), [0, 2, 4]), [0, 1, 0, 1], K, 16, 16)
    with pytest.raises(RuntimeError, match="same device"):
        Rn.mask_iou(lab, lab.cpu(), 2)
    # nothing above launched anything or left an error behind: a valid call still works
    out = Rn.render_labels(table, poses, [0, 1], [1, 2], K, 16, 16)
    assert (out["label"] == 0).all()                                   # all-zero poses: every vertex at Z = 0, dropped
