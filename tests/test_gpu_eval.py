"""GPU tests of the pose evaluation (libpveval.so: pv_nearest_point_idx, pv_pose_metrics)
and its Python layers, against the numpy restatement of tests/test_eval_abi.py.

Sizes: the kernels stage references in LDS tiles of T = 512, track the minimum per
sub-tile of S = 64 references and give a block Q = 512 queries (four per lane of 128);
the shapes below sit on and around each of these."""
import numpy as np
import pytest
import torch

from tests.test_eval_abi import COLS, K_LM, UNIT, make_pose, nearest_f32, pose_columns, rodrigues, symmetric_cloud

pytestmark = pytest.mark.gpu

T = Q = 512
S = 64
L = 128                    # threads of a block: query k of a lane is L * k further on
SIZES = sorted({1, 2, 63, 64, 65, 257, 1031, S - 1, S, S + 1, 2 * S + 1, L - 1, L, L + 1,
                T - 1, T, T + 1, 2 * T + 1})
B = 3


@pytest.fixture(scope="module")
def X():
    from pvnet_amd import build, extend_utils
    build.build()
    return extend_utils


@pytest.fixture(scope="module")
def EV(X):
    from pvnet_amd import evaluation_utils
    return evaluation_utils


def cu(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def nearest_gpu(X, device, ref, que):
    return X.find_nearest_point_idx_batch(cu(ref, device), cu(que, device)).cpu().numpy()


# ----------------------------------------------------------------------------
# pv_nearest_point_idx
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("pn1", SIZES)
def test_nearest_bit_equal(device, X, dim, pn1):
    rng = np.random.default_rng(1000 * dim + pn1)
    refs = [rng.standard_normal((B, pn1, dim)).astype(np.float32) for _ in SIZES]
    ques = [rng.standard_normal((B, pn2, dim)).astype(np.float32) for pn2 in SIZES]
    outs = [X.find_nearest_point_idx_batch(cu(r, device), cu(q, device)) for r, q in zip(refs, ques)]
    for r, q, o in zip(refs, ques, outs):
        o = o.cpu().numpy()
        assert o.dtype == np.int32 and o.shape == q.shape[:2]
        for i in range(B):
            np.testing.assert_array_equal(o[i], nearest_f32(r[i], q[i])[0], err_msg=f"pn2={q.shape[1]} image {i}")


@pytest.mark.parametrize("dim", [2, 3])
def test_nearest_bit_equal_many_blocks(device, X, dim):
    """Query sets of many blocks, ending just before, on and after a block's edge."""
    rng = np.random.default_rng(77 + dim)
    for pn2 in (9 * Q - 1, 9 * Q, 9 * Q + 1):
        for pn1 in (S + 1, T + 1, 2 * T + 1):
            ref = rng.standard_normal((B, pn1, dim)).astype(np.float32)
            que = rng.standard_normal((B, pn2, dim)).astype(np.float32)
            que[:, -5:] = ref[:, -5:] if pn1 >= 5 else que[:, -5:]      # exact hits in the last block
            got = nearest_gpu(X, device, ref, que)
            for i in range(B):
                np.testing.assert_array_equal(got[i], nearest_f32(ref[i], que[i])[0], err_msg=f"{pn1} {pn2} {i}")


def test_nearest_numpy_form(device, X):
    rng = np.random.default_rng(5)
    ref, que = rng.standard_normal((300, 3)), rng.standard_normal((70, 3))
    idx = X.find_nearest_point_idx(ref, que)
    assert isinstance(idx, np.ndarray) and idx.dtype == np.int32 and idx.shape == (70,)
    np.testing.assert_array_equal(idx, nearest_f32(ref, que)[0])
    assert X.find_nearest_point_idx_batch(cu(ref[None], device), cu(que[None, :0], device)).shape == (1, 0)


@pytest.mark.parametrize("dim", [2, 3])
def test_nearest_ties_lowest_index(device, X, dim):
    rng = np.random.default_rng(dim)
    pn1 = 2 * T + 7
    # integer grid: many duplicated references, in every sub-tile and tile ...
    ref = rng.integers(-3, 4, (B, pn1, dim)).astype(np.float32)
    # ... and queries on the half-integer grid, equidistant from several of them
    for nq in (700, 2 * Q + 3):
        que = (rng.integers(-7, 8, (B, nq, dim)) * 0.5).astype(np.float32)
        got = nearest_gpu(X, device, ref, que)
        for i in range(B):
            np.testing.assert_array_equal(got[i], nearest_f32(ref[i], que[i])[0])
    # explicit ties across the sub-tile boundary (63 | 64) and the tile boundary (511 | 512)
    ref = np.full((1, pn1, dim), 100.0, np.float32) + np.arange(pn1, dtype=np.float32)[None, :, None]
    que = np.zeros((1, 4, dim), np.float32)
    ref[0, [S - 1, S]] = 0.0
    ref[0, S - 1, 0], ref[0, S, 0] = 9.0, 11.0
    que[0, 0, 0] = 10.0                               # equidistant from S-1 and S
    ref[0, [T - 1, T]] = 0.0
    ref[0, T - 1, 0], ref[0, T, 0] = -9.0, -11.0
    que[0, 1, 0] = -10.0                              # equidistant from T-1 and T
    ref[0, 10] = ref[0, T + 100] = ref[0, 2 * T + 3] = 50.0
    que[0, 2] = 50.0                                  # three exact duplicates, one per tile
    ref[0, 2 * T + 5] = ref[0, 70] = -50.0
    que[0, 3] = -50.0                                 # the later tile is scanned last and must not win
    for pad in (0, 2 * Q + L - 2):                    # alone, and in a later block, spread over two lanes' slots
        q = np.concatenate([np.full((1, pad, dim), 3000.0, np.float32), que], 1)
        got = nearest_gpu(X, device, ref, q)[0]
        assert got[pad:].tolist() == [S - 1, T - 1, 10, 70]
        np.testing.assert_array_equal(got, nearest_f32(ref[0], q[0])[0])


@pytest.mark.parametrize("dim", [2, 3])
def test_nearest_nan(device, X, dim):
    rng = np.random.default_rng(17 + dim)
    pn1 = T + 9
    ref = rng.standard_normal((B, pn1, dim)).astype(np.float32)
    que = rng.standard_normal((B, 130, dim)).astype(np.float32)
    best = nearest_gpu(X, device, ref, que)
    # image 0: the winners themselves become NaN (one coordinate is enough) and are never chosen again
    ref[0, np.unique(best[0]), dim - 1] = np.nan
    ref[0, 0] = np.nan
    # image 1: every reference NaN -> 0; image 2: NaN queries -> 0
    ref[1] = np.nan
    que[2, ::3, 0] = np.nan
    got = nearest_gpu(X, device, ref, que)
    assert not np.isnan(ref[0][got[0]]).any()
    assert (got[1] == 0).all() and (got[2, ::3] == 0).all()
    for i in range(B):
        np.testing.assert_array_equal(got[i], nearest_f32(ref[i], que[i])[0])


# ----------------------------------------------------------------------------
# pv_pose_metrics
# ----------------------------------------------------------------------------
def models():
    rng = np.random.default_rng(42)
    m0 = (rng.standard_normal((5, 3)) * 0.04).astype(np.float32)
    m1 = symmetric_cloud(rng, 32)
    m2 = np.concatenate([symmetric_cloud(rng, 515), np.array([[0, 0, 0.03]], np.float32)])
    return [(m0, 0.11, False), (m1, 0.18, True), (m2, 0.2, True)]


def batch():
    """b = 5 over the three models: identical, 1e-4 rad / 1e-5 m apart, generic, 180 deg about the
    symmetry axis, generic."""
    gt = [make_pose([0.2, -0.4, 0.9], 0.8, [0.03, -0.05, 0.85]),
          make_pose([1, 0.3, -0.2], 2.1, [-0.08, 0.02, 1.1]),
          make_pose([0.1, 0.9, 0.4], 1.3, [0.0, 0.06, 0.7]),
          make_pose([-0.5, 0.5, 0.7], 0.4, [0.1, 0.1, 0.95]),
          make_pose([0.3, 0.3, -0.9], 2.9, [-0.02, -0.07, 1.3])]
    d = 1e-5 / np.sqrt(3)
    pred = [gt[0].copy(),
            np.concatenate([rodrigues([0.6, -0.1, 0.8], 1e-4) @ gt[1][:, :3], gt[1][:, 3:] + d], 1),
            np.concatenate([rodrigues([0.2, 1, 0.1], 0.21) @ gt[2][:, :3], gt[2][:, 3:] + [[0.01], [-0.02], [0.03]]], 1),
            np.concatenate([gt[3][:, :3] @ rodrigues([0, 0, 1], np.pi), gt[3][:, 3:]], 1),
            np.concatenate([rodrigues([1, 1, 1], 0.05) @ gt[4][:, :3], gt[4][:, 3:] + [[0.004], [0.0], [-0.01]]], 1)]
    return np.stack(pred), np.stack(gt), np.array([2, 0, 1, 2, 1], np.int32)


def per_pose_K(b):
    K = np.repeat(K_LM[None], b, 0).copy()
    for i in range(b):
        K[i, 0, 0] *= 1 + 0.03 * i
        K[i, 1, 1] *= 1 - 0.02 * i
        K[i, 0, 2] += 3.0 * i
        K[i, 0, 1] = 0.1 * i
    return K


def reference(pred, gt, mid, mods, K):
    """The restatement's columns for each pose: ([b][6] float64, [b] (M3, M2), [b] pn)."""
    cols, Ms, pns = [], [], []
    for i in range(len(pred)):
        pts = mods[mid[i]][0]
        c, M = pose_columns(pred[i], gt[i], pts, K[i] if K.ndim == 3 else K)
        cols.append([c[k] for k in COLS])
        Ms.append(M)
        pns.append(len(pts))
    return np.array(cols), Ms, pns


def check_columns(got, want, Ms, pns, rot_close=()):
    """The tolerances of DESIGN 10b: relative 1e-12 pn for the float64 columns, 32 units of
    2^-24 M for the nearest-neighbour columns; ROT_DEG of identical poses within 1e-5 deg."""
    for i in range(len(got)):
        g, w = dict(zip(COLS, got[i])), dict(zip(COLS, want[i]))
        rel = 1e-12 * pns[i]
        print(f"pose {i} pn {pns[i]}: " + " ".join(
            f"{k} {g[k]:.6e} (err {abs(g[k] - w[k]):.2e})" for k in COLS) +
            f" | adds {abs(g['adds'] - w['adds']) / (UNIT * Ms[i][0]):.2f} u, proj_sym "
            f"{abs(g['proj_sym'] - w['proj_sym']) / (UNIT * Ms[i][1]):.2f} u")
        for k in ("add", "proj", "trans_cm"):
            assert abs(g[k] - w[k]) <= rel * abs(w[k]), (i, k, g[k], w[k])
        assert abs(g["adds"] - w["adds"]) <= 32 * UNIT * Ms[i][0], (i, g["adds"], w["adds"])
        assert abs(g["proj_sym"] - w["proj_sym"]) <= 32 * UNIT * Ms[i][1], (i, g["proj_sym"], w["proj_sym"])
        if w["rot_deg"] >= 1.0:
            assert abs(g["rot_deg"] - w["rot_deg"]) <= rel * w["rot_deg"], (i, g["rot_deg"], w["rot_deg"])
        elif i in rot_close:
            # below 1 deg arccos amplifies the trace's rounding (nine products and eight sums of
            # magnitude <= 3, at most 17 * 3 * 2^-53) by 1 / (2 sin(angle))
            tol = np.degrees(17 * 3 * 2.0 ** -53 / (2 * np.sin(np.radians(w["rot_deg"]))))
            assert abs(g["rot_deg"] - w["rot_deg"]) <= tol, (i, g["rot_deg"], w["rot_deg"], tol)
        else:
            assert w["rot_deg"] <= 1e-5 and 0.0 <= g["rot_deg"] <= 1e-5, (i, g["rot_deg"], w["rot_deg"])


def run_metrics(EV, device, pred, gt, mid, table, K, **kw):
    m = EV.pose_metrics(cu(pred, device), cu(gt, device), table, cu(np.asarray(K, np.float64), device),
                        None if mid is None else cu(mid, device), **kw)
    return {k: v.cpu().numpy() for k, v in m.items()}


@pytest.fixture(scope="module")
def scene(device, EV):
    mods = models()
    pred, gt, mid = batch()
    return dict(mods=mods, table=EV.ModelTable(mods, device), pred=pred, gt=gt, mid=mid)


@pytest.mark.parametrize("shared_K", [True, False])
def test_pose_metrics_against_restatement(device, EV, scene, shared_K):
    s = scene
    K = K_LM if shared_K else per_pose_K(5)
    m = run_metrics(EV, device, s["pred"], s["gt"], s["mid"], s["table"], K)
    assert sorted(m) == sorted(COLS) and all(v.dtype == np.float64 and v.shape == (5,) for v in m.values())
    got = np.stack([m[k] for k in COLS], 1)
    want, Ms, pns = reference(s["pred"], s["gt"], s["mid"], s["mods"], K)
    check_columns(got, want, Ms, pns, rot_close=(1,))
    # identical poses: exactly zero; the 180 deg pose about the symmetry axis: ADD large, ADD-S ~ 0
    assert got[0, 0] == 0.0 and got[0, 1] == 0.0 and got[0, 2] == 0.0 and got[0, 3] == 0.0 and got[0, 4] == 0.0
    assert got[3, 0] > 0.05 and got[3, 1] <= 32 * UNIT * Ms[3][0] and abs(got[3, 5] - 180.0) < 1e-6


def test_unrequested_columns_untouched(device, EV, scene):
    s = scene
    full = run_metrics(EV, device, s["pred"], s["gt"], s["mid"], s["table"], K_LM)
    for want in (("adds", "cmdeg"), ("add",), ("proj", "proj_sym"), ("cmdeg",)):
        out = torch.full((5, 6), -7.0, dtype=torch.float64, device=device)
        m = run_metrics(EV, device, s["pred"], s["gt"], s["mid"], s["table"], K_LM, metrics=want, out=out)
        o = out.cpu().numpy()
        for c, name in enumerate(COLS):
            if name in m:
                np.testing.assert_array_equal(bits(o[:, c]), bits(full[name]), err_msg=name)
                np.testing.assert_array_equal(bits(m[name]), bits(full[name]))
            else:
                assert (o[:, c] == -7.0).all(), name


def test_bad_model_ids_and_poses_give_nan(device, EV, scene):
    s = scene
    mods = [s["mods"][0], (np.zeros((0, 3), np.float32), 1.0, False), s["mods"][2]]
    table = EV.ModelTable(mods, device)
    pred = np.concatenate([s["pred"], s["pred"][:2]])
    gt = np.concatenate([s["gt"], s["gt"][:2]])
    good = np.array([2, 0, 0, 2, 0, 2, 0], np.int32)
    base = run_metrics(EV, device, pred, gt, good, table, K_LM)
    mid = good.copy()
    mid[1], mid[2], mid[4] = 1, 7, -1                 # the empty model, past the table, negative
    pred2 = pred.copy()
    pred2[5, 1, 2] = np.nan
    pred2[6, 0, 3] = np.inf
    m = run_metrics(EV, device, pred2, gt, mid, table, K_LM)
    for k in ("add", "adds", "proj", "proj_sym"):
        assert np.isnan(m[k][[1, 2, 4, 5, 6]]).all(), k
        np.testing.assert_array_equal(bits(m[k][[0, 3]]), bits(base[k][[0, 3]]))
    for k in ("trans_cm", "rot_deg"):
        assert np.isnan(m[k][[5, 6]]).all(), k
        np.testing.assert_array_equal(bits(m[k][:5]), bits(base[k][:5]))
    # model_id None = model 0 for every pose
    none = run_metrics(EV, device, pred, gt, None, table, K_LM)
    zero = run_metrics(EV, device, pred, gt, np.zeros(7, np.int32), table, K_LM)
    for k in COLS:
        np.testing.assert_array_equal(bits(none[k]), bits(zero[k]))
        assert np.isfinite(none[k]).all()


def test_two_calls_bit_equal(device, EV, scene):
    s = scene
    K = per_pose_K(5)
    a = run_metrics(EV, device, s["pred"], s["gt"], s["mid"], s["table"], K)
    b = run_metrics(EV, device, s["pred"], s["gt"], s["mid"], s["table"], K)
    for k in COLS:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]))


def test_graph_capture_on_side_stream(device, EV, scene):
    """One call captured on a side stream (a linear chain of two launches); two replays equal the eager call."""
    s = scene
    pred, gt, mid, K = (cu(a, device) for a in (s["pred"], s["gt"], s["mid"], K_LM))
    ref = torch.empty((5, 6), dtype=torch.float64, device=device)
    EV.pose_metrics(pred, gt, s["table"], K, mid, out=ref)
    torch.cuda.synchronize()
    out = torch.zeros((5, 6), dtype=torch.float64, device=device)
    gph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gph, stream=side):
            EV.pose_metrics(pred, gt, s["table"], K, mid, out=out)
    for _ in range(2):
        out.zero_()
        gph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(ref.cpu().numpy()))


# ----------------------------------------------------------------------------
# chained on uncertainty_pnp_batch, and the Evaluator
# ----------------------------------------------------------------------------
def keypoints_3d(pts):
    """Nine 3-D keypoints of a model: its bounding box's corners and its centre."""
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    return np.concatenate([c, (lo + hi)[None] / 2])


def test_chained_on_pnp_output(device, X, EV, scene):
    from pvnet_amd import synth
    s = scene
    p3 = np.stack([keypoints_3d(s["mods"][m][0]) for m in s["mid"]])
    rng = np.random.default_rng(9)
    p2 = np.stack([synth.project(p3[i], s["gt"][i]) for i in range(5)]) + rng.standard_normal((5, 9, 2)) * 0.05
    w = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64, device=device).expand(5, 9, 3)
    Rt = X.uncertainty_pnp_batch(cu(p2, device), w, cu(p3, device), cu(K_LM, device), mode="weights")
    assert Rt.dtype == torch.float64 and Rt.is_contiguous()
    m = EV.pose_metrics(Rt, cu(s["gt"], device), s["table"], cu(K_LM, device), cu(s["mid"], device))
    got = np.stack([m[k].cpu().numpy() for k in COLS], 1)
    rt = Rt.cpu().numpy()
    want, Ms, pns = reference(rt, s["gt"], s["mid"], s["mods"], K_LM)
    check_columns(got, want, Ms, pns, rot_close=range(5))
    assert (got[:, 0] < 0.01).all() and (got[:, 2] < 5).all()       # 0.05 px of noise: poses near the truth


def test_evaluator_against_restatement(device, EV, scene):
    from pvnet_amd import synth
    s = scene
    mods, table = s["mods"], s["table"]
    kp3 = np.stack([keypoints_3d(m[0]) for m in mods])
    ev = EV.Evaluator(table, kp3)
    mid = np.array([0, 1, 2, 0, 1, 2], np.int32)
    gt = np.stack([s["gt"][i % 5] for i in range(6)])
    # exact keypoints of the true pose, except: pose 1 rotated by 180 deg about the symmetry axis
    # (a hit for a symmetric model), pose 3 shifted by 8 cm, pose 4 rotated by 20 deg and shifted by 10 cm
    src = gt.copy()
    src[1] = np.concatenate([gt[1][:, :3] @ rodrigues([0, 0, 1], np.pi), gt[1][:, 3:]], 1)
    src[3][:, 3] += [0.08, 0.0, 0.0]
    src[4] = np.concatenate([rodrigues([0, 1, 0], np.radians(20)) @ gt[4][:, :3],
                             gt[4][:, 3:] + [[0.0], [0.1], [0.0]]], 1)
    p2 = np.stack([synth.project(kp3[mid[i]], src[i]) for i in range(6)])
    Rt = ev.evaluate(cu(p2, device), cu(gt, device), cu(mid, device), K_LM).cpu().numpy()
    want, _, _ = reference(Rt, gt, mid, mods, K_LM)
    w = {k: want[:, c] for c, k in enumerate(COLS)}
    sym = np.array([mods[m][2] for m in mid])
    diam = np.array([mods[m][1] for m in mid])
    proj = np.where(sym, w["proj_sym"], w["proj"]) < 5.0
    add = np.where(sym, w["adds"], w["add"]) < 0.1 * diam
    cm5 = (w["trans_cm"] < 5.0) & (w["rot_deg"] < 5.0)
    assert proj.tolist() == [True, True, True, False, False, True]
    assert add.tolist() == [True, True, True, False, False, True]
    assert cm5.tolist() == [True, False, True, False, False, True]
    np.testing.assert_array_equal(ev.projection_2d_recorder[0].cpu().numpy(), proj)
    np.testing.assert_array_equal(ev.add_recorder[0].cpu().numpy(), add)
    np.testing.assert_array_equal(ev.cm_degree_5_recorder[0].cpu().numpy(), cm5)
    assert ev.average_precision() == pytest.approx((proj.mean(), add.mean(), cm5.mean()), abs=1e-12)
    # evaluate_uncertainty: the same keypoints with tight isotropic covariances, a second batch
    cov = torch.eye(2, device=device).expand(6, 9, 2, 2) * 0.01
    Rt2 = ev.evaluate_uncertainty(cu(p2.astype(np.float32), device), cov, cu(gt, device), cu(mid, device), K_LM)
    want2, _, _ = reference(Rt2.cpu().numpy(), gt, mid, mods, K_LM)
    w2 = {k: want2[:, c] for c, k in enumerate(COLS)}
    add2 = np.where(sym, w2["adds"], w2["add"]) < 0.1 * diam
    np.testing.assert_array_equal(ev.add_recorder[1].cpu().numpy(), add2)
    assert len(ev.add_recorder) == 2
    assert ev.average_precision()[1] == pytest.approx(np.concatenate([add, add2]).mean(), abs=1e-12)
