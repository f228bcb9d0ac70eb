"""pvnet_amd.models on the device against the numpy restatement (tests/model_ref.py).  Every
comparison is exact -- indices and f64 bits -- unless it says otherwise: that is what the fp64,
no-contraction definition of include/pvmodel.h is for."""
import numpy as np
import pytest
import torch

from tests import model_ref as M
from tests import render_ref as R

pytestmark = pytest.mark.gpu

STARTS = {"centroid": M.START_CENTROID, "centroid_kept": M.START_CENTROID_KEPT, "index": M.START_INDEX}
# around the wave, PV_MODEL_SUM_LANES and PV_MODEL_TILE (both 256: +-1 and 2 TILE + 1), 1024, the diameter's
# largest exact check, PV_MODEL_BLOCK_MAX_PN, and one model of 3 chunks + 1
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2 * M.TILE + 1, 1023, 1024, 1025, 4097,
         M.BLOCK_MAX_PN - 1, M.BLOCK_MAX_PN, M.BLOCK_MAX_PN + 1, 3 * M.CHUNK + 1]


@pytest.fixture(scope="module")
def Mo(device):
    import __graft_entry__ as g
    g.build()
    from pvnet_amd import models
    return models


class Table:
    """Any points, offsets and max_pn (pvnet_amd.models takes whatever has a ModelTable's three fields)."""

    def __init__(self, points, off, max_pn, device):
        self.np_points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        self.np_off = np.asarray(off, np.int32)
        self.max_pn = int(max_pn)
        self.points = torch.from_numpy(self.np_points).to(device)
        self.offsets = torch.from_numpy(self.np_off).to(device)
        self.nmodels = len(off) - 1
        self._extent = None

    @classmethod
    def of(cls, models, device, max_pn=None):
        models = [np.asarray(m, np.float32).reshape(-1, 3) for m in models]
        off = np.concatenate([[0], np.cumsum([m.shape[0] for m in models])])
        return cls(np.concatenate(models), off, max(m.shape[0] for m in models) if max_pn is None else max_pn, device)

    def ref_extent(self):
        if self._extent is None:
            self._extent = M.table_extent(self.np_points, self.np_off, self.max_pn)
        return self._extent

    def ref_fps(self, k, start, start_idx=None):
        return M.table_farthest_points(self.np_points, self.np_off, self.max_pn, k, start, start_idx,
                                       self.ref_extent()["centroid"])

    def ref_diameter(self):
        return M.table_diameter(self.np_points, self.np_off, self.max_pn)


def same_bits(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.int64), want[ok].view(np.int64), err_msg=what)


def check_fps(Mo, tab, k, start, start_idx=None):
    arg = start if start_idx is None else torch.as_tensor(start_idx, dtype=torch.int32).to(tab.points.device)
    idx, picked, pd2 = Mo.farthest_points(tab, k, arg, with_d2=True)
    ref = tab.ref_fps(k, STARTS["index" if start_idx is not None else start], start_idx)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (tab.nmodels, k)
    assert picked.dtype == torch.float64 and tuple(picked.shape) == (tab.nmodels, k, 3)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref["idx"])
    same_bits(picked.cpu().numpy(), ref["picked"], "picked")
    same_bits(pd2.cpu().numpy(), ref["pick_d2"], "pick_d2")
    return idx.cpu().numpy(), ref


def check_extent(Mo, tab):
    e = {k: v.cpu().numpy() for k, v in Mo.extent(tab).items()}
    ref = tab.ref_extent()
    np.testing.assert_array_equal(e["count"], ref["count"])
    for k in ("bbox_min", "bbox_max", "centroid"):
        same_bits(e[k], ref[k], k)
    return e


def ball(rng, n, radius=1.0):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3)).astype(np.float32)


# ---- 1. sizes around every boundary ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def size_table(device):
    rng = np.random.default_rng(11)
    tab = Table.of([rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, 3) + rng.normal(size=3) for n in SIZES], device)
    tab.start_idx = np.array([rng.integers(0, n) for n in SIZES], np.int32)
    return tab


@pytest.mark.parametrize("k", [1, 8, 9])
@pytest.mark.parametrize("start", ["centroid", "centroid_kept", "index"])
def test_fps_sizes(Mo, size_table, start, k):
    idx, _ = check_fps(Mo, size_table, k, start, size_table.start_idx if start == "index" else None)
    assert (idx >= 0).all()


def test_extent_sizes(Mo, size_table):
    e = check_extent(Mo, size_table)
    np.testing.assert_array_equal(e["count"], SIZES)


def test_diameter_sizes(Mo, device):
    rng = np.random.default_rng(12)
    sizes = [n for n in SIZES if n <= 4097]
    tab = Table.of([rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, 3) for n in sizes], device)
    got = Mo.diameter(tab)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(sizes),)
    same_bits(got.cpu().numpy(), tab.ref_diameter(), "diameter")
    assert got[0] == 0.0


# ---- 2. one table with mixed models -----------------------------------------------------------------------------
def test_mixed_table(Mo, device):
    rng = np.random.default_rng(13)
    small, large, over = M.BLOCK_MAX_PN - 288, M.BLOCK_MAX_PN + 112, M.BLOCK_MAX_PN + 212
    bad = rng.normal(size=(300, 3)).astype(np.float32)
    clean = M.farthest_points(M.widen(bad), 8)["idx"]
    bad[clean[0]] = [np.nan, 0.0, 0.0]                   # the index that would otherwise win pick 0
    bad[clean[1]] = [0.0, np.inf, 0.0]
    bad[7], bad[299] = [-np.inf, np.nan, 1.0], [1.0, 2.0, -np.inf]
    planted = []
    for n in (small, large):                            # the diameter of the two big ones is known without n^2 work
        v = ball(rng, n)
        v[n // 3], v[n - 2] = [2.0, 0.0, 0.0], [-2.0, 0.0, 0.0]
        planted.append(v)
    models = [rng.normal(size=(1, 3)), rng.normal(size=(100, 3)), np.zeros((0, 3)), ball(rng, over), bad,
              planted[0], np.full((5, 3), np.nan), planted[1]]
    tab = Table.of(models, device, max_pn=large)
    skipped = [2, 3, 6]
    e = check_extent(Mo, tab)
    assert e["count"].tolist() == [1, 100, 0, 0, 296, small, 0, large]
    sidx = np.array([0, 99, 0, 5, 11, 17, 0, large - 1], np.int32)
    for start, k in (("centroid", 8), ("centroid_kept", 9), ("index", 8)):
        idx, ref = check_fps(Mo, tab, k, start, sidx if start == "index" else None)
        assert (idx[skipped] == -1).all() and (np.delete(idx, skipped, 0) >= 0).all()
        assert not set(idx[4].tolist()) & {int(clean[0]), int(clean[1]), 7, 299}
    d = Mo.diameter(tab).cpu().numpy()
    want = np.array([0.0, M.diameter(M.widen(models[1])), np.nan, np.nan, M.diameter(M.widen(bad)), 4.0, np.nan, 4.0])
    same_bits(d, want, "diameter")


def test_offsets_that_are_not_monotone_skip(Mo, device):
    rng = np.random.default_rng(14)
    pts = rng.normal(size=(200, 3))
    for off in ([0, 50, 30, 120, 100, 260], [-5, 10, 20, 200], [0, 0, 0, 200], [200, 0, 100, 2 ** 31 - 1]):
        tab = Table(pts, off, 150, device)
        e = check_extent(Mo, tab)
        for start in ("centroid", "centroid_kept"):
            check_fps(Mo, tab, 4, start)
        check_fps(Mo, tab, 4, "index", np.full(tab.nmodels, 3, np.int32))
        same_bits(Mo.diameter(tab).cpu().numpy(), tab.ref_diameter(), "diameter")
        assert (e["count"] == 0).any()


# ---- 3. ties ----------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_index(Mo, device):
    g = np.arange(9, dtype=np.float32)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    five = np.random.default_rng(15).normal(size=(5, 3))
    tab = Table.of([R.box(0.05, 0.04, 0.03)[0], R.icosphere(3)[0], grid, np.full((50, 3), 0.25), five], device)
    e = check_extent(Mo, tab)
    assert e["centroid"][2].tolist() == [4.0, 4.0, 4.0]
    for start in ("centroid", "centroid_kept"):
        for k in (5, 8, 9):                                            # k = n and k = n + 3 of the 5-point model
            idx, _ = check_fps(Mo, tab, k, start)
            assert (idx[3] == 0).all()                                 # identical points: the lowest index every time
        assert idx[0, 0] == 0 and idx[2, 0] == 0                       # all 8 corners tie for pick 0
    idx, _ = check_fps(Mo, tab, 8, "index", np.array([3, 100, 364, 49, 4], np.int32))
    assert idx[3].tolist() == [49, 0, 0, 0, 0, 0, 0, 0] and sorted(idx[4, :5].tolist()) == [0, 1, 2, 3, 4]
    assert idx[4, 5:].tolist() == [0, 0, 0]
    d = Mo.diameter(tab).cpu().numpy()
    same_bits(d, tab.ref_diameter(), "diameter")
    assert d[3] == 0.0 and d[2] == np.sqrt(192.0)


def test_equal_farthest_points_in_different_waves_tiles_and_chunks(Mo, device):
    rng = np.random.default_rng(16)
    models = []
    for n in (300, 5000, 2 * M.CHUNK + 10):              # block form (two sizes) and the per-step form
        v = ball(rng, n, 0.5)
        v[7] = [-3.5, 0.0, 0.0]
        v[5] = v[n - 1] = [3.0, 0.25, 0.0]               # from the point at 7 these two tie, and n - 1 sits in the
        models.append(v)                                 # last wave, tile and chunk
    tab = Table.of(models, device)
    for start in ("centroid", "centroid_kept"):
        idx, _ = check_fps(Mo, tab, 4, start)
        assert (idx[:, 0] == 7).all() and (idx[:, 1] == 5).all()
    idx, _ = check_fps(Mo, tab, 4, "index", np.full(3, 7, np.int32))
    assert (idx[:, 1] == 5).all()
    # the diameter is reached twice, from tiles far apart: (7, 5) and (7, n - 1), 6.5 along x and 0.25 along y
    same_bits(Mo.diameter(tab).cpu().numpy(), np.full(3, np.sqrt(6.5 * 6.5 + 0.25 * 0.25)), "diameter")
    # and with the pair farthest from the centroid itself: pick 0 is a tie
    for v in models:
        v[7] = [0.0, 0.0, 0.0]
    tab = Table.of(models, device)
    idx, _ = check_fps(Mo, tab, 3, "centroid")
    assert (idx[:, 0] == 5).all()


# ---- 4. the diameter of a large model ---------------------------------------------------------------------------
def test_diameter_placement_on_a_large_model(Mo, device):
    n = 70001
    rng = np.random.default_rng(17)
    base = ball(rng, n)
    models = []
    for a, b in ((0, n - 1), (M.TILE * 4 + 6, M.TILE * 4 + 76), (n - 101, n - 1)):   # ends, one tile, the last partial tile
        assert (a // M.TILE == b // M.TILE) == (a != 0) and (a == 0 or a // M.TILE in (4, (n - 1) // M.TILE))
        v = base.copy()
        v[a], v[b] = [2.0, 0.0, 0.0], [-2.0, 0.0, 0.0]
        models.append(v)
    tab = Table.of(models, device)
    d = Mo.diameter(tab).cpu().numpy()
    assert d.tolist() == [4.0, 4.0, 4.0]
    # without the planted pair nothing reaches 2 (the ball's own diameter), so the 4 came from that pair
    assert Mo.diameter(Table.of([base], device)).item() <= 2.0


# ---- 5. the centroid's order -------------------------------------------------------------------------------------
def test_centroid_order(Mo, device):
    p = np.zeros((769, 3), np.float32)
    p[0, 0], p[256, 0], p[512, 0] = 2.0 ** 60, 1.0, -2.0 ** 60
    q = p[np.random.default_rng(0).permutation(769)]
    tab = Table.of([p, q], device)
    e = check_extent(Mo, tab)
    # lane 0 of the first model holds all three: (2^60 + 1) - 2^60 = 0; in the shuffled copy they sit in three
    # lanes and the 1 survives, where a sequential sum loses it
    assert e["centroid"][0, 0] == 0.0 and e["centroid"][1, 0] == 1.0 / 769.0
    assert float(np.sum(M.widen(q)[:, 0])) / 769.0 == 0.0


# ---- 6. start_idx ---------------------------------------------------------------------------------------------------
def test_start_idx(Mo, device):
    rng = np.random.default_rng(18)
    models = [rng.normal(size=(100, 3)).astype(np.float32) for _ in range(5)]
    models[3][42] = [0.0, np.nan, 0.0]
    tab = Table.of(models, device)
    idx, _ = check_fps(Mo, tab, 6, "index", np.array([17, -1, 100, 42, 99], np.int32))
    assert idx[0, 0] == 17 and idx[4, 0] == 99 and (idx[1:4] == -1).all()
    with pytest.raises(RuntimeError, match="start"):
        Mo.farthest_points(tab, 6, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="start"):
        Mo.farthest_points(tab, 6, "random")
    for k in (0, M.MAX_K + 1):
        with pytest.raises(RuntimeError, match="k must"):
            Mo.farthest_points(tab, k)


# ---- 7. determinism and capture --------------------------------------------------------------------------------
def test_determinism_and_capture(Mo, device):
    rng = np.random.default_rng(19)
    tab = Table.of([ball(rng, 500), ball(rng, M.BLOCK_MAX_PN + 700), ball(rng, 3000)], device)

    def calls():
        e = Mo.extent(tab)
        idx, picked, pd2 = Mo.farthest_points(tab, 8, "centroid_kept", with_d2=True)
        return dict(bbox_min=e["bbox_min"], centroid=e["centroid"], count=e["count"], idx=idx, picked=picked, pd2=pd2,
                    diameter=Mo.diameter(tab))

    def bits(d):
        return {k: v.cpu().numpy().copy().view(np.int32 if v.dtype == torch.int32 else np.int64) for k, v in d.items()}

    a, b = bits(calls()), bits(calls())
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (a["idx"] >= 0).all()
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gph, stream=side):
            out = calls()
    for _ in range(2):
        for t in out.values():
            t.fill_(77)
        gph.replay()
        torch.cuda.synchronize()
        got = bits(out)
        for k in a:
            np.testing.assert_array_equal(got[k], a[k], err_msg=k)


# ---- 8. the Python layer --------------------------------------------------------------------------------------------
def test_python_layer(Mo, device):
    from pvnet_amd import evaluation_utils as EU
    from pvnet_amd import render as Rn
    meshes = [R.box(0.05, 0.04, 0.03), R.bumpy_ellipsoid(2), R.icosphere(2, 0.04)]
    table = Rn.MeshTable(meshes, device=device)
    v = [M.widen(m[0]) for m in meshes]
    ext = [M.extent(x) for x in v]
    c = Mo.corners_3d(table)
    assert c.dtype == torch.float64 and tuple(c.shape) == (3, 8, 3) and c.device == table.verts.device
    for m in range(3):
        lo, hi = ext[m]["bbox_min"], ext[m]["bbox_max"]
        want = np.array([[hi[0] if i & 4 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 1 else lo[2]] for i in range(8)])
        np.testing.assert_array_equal(c[m].cpu().numpy(), want)
    for centre in ("centroid", "bbox"):
        kp = Mo.keypoints_3d(table, 8, centre=centre)
        assert kp.dtype == torch.float64 and tuple(kp.shape) == (3, 9, 3)
        for m in range(3):
            np.testing.assert_array_equal(kp[m, :8].cpu().numpy(), M.farthest_points(v[m], 8)["picked"])
            mid = ext[m]["centroid"] if centre == "centroid" else (ext[m]["bbox_min"] + ext[m]["bbox_max"]) * 0.5
            np.testing.assert_array_equal(kp[m, 8].cpu().numpy(), mid)
    kept = Mo.keypoints_3d(table, 4, start="centroid_kept")
    np.testing.assert_array_equal(kept[1, :4].cpu().numpy(), M.farthest_points(v[1], 4, M.START_CENTROID_KEPT)["picked"])
    with pytest.raises(RuntimeError, match="centre"):
        Mo.keypoints_3d(table, 8, centre="middle")
    # a ModelTable is taken as well as a MeshTable, with the same answers
    diam = [M.diameter(x) for x in v]
    hand = EU.ModelTable([(m[0], d, s) for m, d, s in zip(meshes, diam, (True, False, False))], device=device)
    same_bits(Mo.diameter(hand).cpu().numpy(), np.array(diam))
    np.testing.assert_array_equal(Mo.farthest_points(hand, 8)[0].cpu().numpy(), Mo.farthest_points(table, 8)[0].cpu().numpy())
    # from_meshes: the mesh table's own storage, the device's diameter
    made = EU.ModelTable.from_meshes(table, symmetric=(True, False, False))
    assert made.points.data_ptr() == table.verts.data_ptr() and made.offsets.data_ptr() == table.vert_off.data_ptr()
    assert made.points is table.verts and made.offsets is table.vert_off
    assert (made.nmodels, made.total, made.max_pn, made.counts) == (hand.nmodels, hand.total, hand.max_pn, hand.counts)
    assert (made.any_symmetric, made.all_symmetric) == (True, False) and made.symmetric.tolist() == [True, False, False]
    assert made.diameter.dtype == torch.float64 and made.diameter.device == table.verts.device
    same_bits(made.diameter.cpu().numpy(), np.array(diam))
    plain = EU.ModelTable.from_meshes(table)
    assert not plain.any_symmetric and plain.symmetric.tolist() == [False] * 3
    rng = np.random.default_rng(20)
    gt = torch.from_numpy(np.array([R.pose(R.random_rotation(rng), [0.0, 0.0, 0.8]) for _ in range(6)])).to(device)
    pred = gt.clone()
    pred[:, :, 3] += torch.from_numpy(rng.normal(size=(6, 3)) * 1e-3).to(device)
    ids = torch.tensor([0, 1, 2, 2, 1, 0], dtype=torch.int32, device=device)
    K = torch.eye(3, dtype=torch.float64, device=device)
    m0 = EU.pose_metrics(pred, gt, hand, K, ids, metrics=("add", "adds"))
    m1 = EU.pose_metrics(pred, gt, made, K, ids, metrics=("add", "adds"))
    for k in ("add", "adds"):
        np.testing.assert_array_equal(m0[k].cpu().numpy(), m1[k].cpu().numpy())
    assert float(m0["add"].min()) > 0.0


# ---- 9. the loop from meshes alone ---------------------------------------------------------------------------------
def test_loop_closes_from_meshes_alone(Mo, device):
    from pvnet_amd import evaluation_utils as EU
    from pvnet_amd import extend_utils as X
    from pvnet_amd import ransac_voting_gpu as rvg
    from pvnet_amd import render as Rn
    from tests.test_gpu_render import CPU_WORST, cu, loop_scene
    s = loop_scene()
    H, W, K = s["H"], s["W"], cu(s["K"], device)
    table = Rn.MeshTable(s["models"], device=device)
    points_3d = Mo.keypoints_3d(table)
    etable = EU.ModelTable.from_meshes(table)
    got = points_3d.cpu().numpy()
    np.testing.assert_array_equal(got[:, :8], s["p3"][:, :8])             # the same vertices
    assert np.abs(got[:, 8] - s["p3"][:, 8]).max() <= 1e-15               # the centre
    diam = etable.diameter.cpu().numpy()
    assert (np.abs(diam - np.array(s["diameter"])) <= np.spacing(np.array(s["diameter"]))).all()   # 1 ulp

    poses = cu(s["poses"], device)
    mid = torch.tensor([0, 1], dtype=torch.int32, device=device)
    label, vertex, kp_true = Rn.render_ground_truth(table, points_3d, poses, mid, K, H, W)
    assert tuple(label.shape) == (4, H, W) and tuple(vertex.shape) == (4, H, W, 18, 2) and tuple(kp_true.shape) == (4, 2, 9, 2)
    area = torch.stack([(label == c + 1).sum((1, 2)) for c in range(2)], 1).cpu().numpy()
    assert area.min() > 1000
    kp = rvg.ransac_voting_layer_v3_multi(label, vertex, 2, 512, _seed=20240)
    p3 = points_3d[None].expand(4, 2, 9, 3).reshape(8, 9, 3)
    est = X.pnp_batch(kp.reshape(8, 9, 2).to(torch.float64), p3, K, method="epnp")
    gt = poses.reshape(8, 3, 4)
    ids = mid.repeat(4)
    m = EU.pose_metrics(est, gt, etable, K, ids, metrics=("add", "proj"))
    kp_err = float((kp.to(torch.float64) - kp_true).norm(dim=-1).max())
    add, proj = m["add"].cpu().numpy() / diam[[0, 1] * 4], m["proj"].cpu().numpy()
    print(f"loop from meshes: keypoints {kp_err:.3e} px, ADD/diameter {add.max():.3e}, projection {proj.max():.3e} px")
    assert (add < 0.1).all() and (proj < 5.0).all()
    assert kp_err <= 4 * CPU_WORST["keypoint_px"]
    assert add.max() <= 4 * CPU_WORST["add_over_diameter"]
    assert proj.max() <= 4 * CPU_WORST["proj_px"]
    again = Rn.render_labels(table, est.reshape(4, 2, 3, 4), mid, None, K, H, W, want=("label",))["label"]
    iou = Rn.mask_iou(again, label, 2).cpu().numpy()
    assert iou.shape == (4, 2) and (iou >= 0.98).all()
    for i, far in ((2, 0), (3, 1)):
        alone = Rn.render_labels(table, poses[i:i + 1, far:far + 1], mid[far:far + 1], None, K, H, W, want=("label",))["label"]
        assert int((alone > 0).sum()) > area[i, far] + 200
