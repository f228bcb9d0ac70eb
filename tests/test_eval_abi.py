"""CPU-side checks of libpveval.so (include/pveval.h) and of the numpy restatement the
GPU tests of the pose evaluation compare against (tests/test_gpu_eval.py).

The restatement is the checker of this feature:
* :func:`nearest_f32` -- the float32 arithmetic of pv_nearest_point_idx, operation for
  operation, with ``argmin`` over NaN-to-inf distances (first minimum wins);
* :func:`pose_columns` -- the six columns of pv_pose_metrics in (long) double precision.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K_LM = np.array([[572.4114, 0., 325.2611], [0., 573.57043, 242.04899], [0., 0., 1.]])
COLS = ("add", "adds", "proj", "proj_sym", "trans_cm", "rot_deg")
UNIT = 2.0 ** -24          # the nearest-neighbour columns' bound is 32 * UNIT * M


# ----------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------
def nearest_f32(ref, que, chunk=128):
    """include/pveval.h's definition in numpy float32 (every operation rounded, no fused
    multiply-add): (idx int32 [pn2], min d2 float32 [pn2]); a NaN d2 counts as +inf."""
    ref = np.ascontiguousarray(ref, np.float32)
    que = np.ascontiguousarray(que, np.float32)
    dim = ref.shape[1]
    idx = np.zeros(que.shape[0], np.int32)
    dmin = np.full(que.shape[0], np.inf, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, que.shape[0], chunk):
            q = que[s:s + chunk]
            dx = q[:, None, 0] - ref[None, :, 0]
            dy = q[:, None, 1] - ref[None, :, 1]
            d = dx * dx + dy * dy
            if dim == 3:
                dz = q[:, None, 2] - ref[None, :, 2]
                d = d + dz * dz
            assert d.dtype == np.float32
            d[np.isnan(d)] = np.inf
            idx[s:s + chunk] = np.argmin(d, axis=1)
            dmin[s:s + chunk] = np.min(d, axis=1)
    return idx, dmin


def _nearest_dist_f64(ref, que, chunk=128):
    out = np.empty(que.shape[0])
    for s in range(0, que.shape[0], chunk):
        d = que[s:s + chunk, None, :] - ref[None, :, :]
        out[s:s + chunk] = np.sqrt((d * d).sum(-1).min(1))
    return out


def centred_clouds(pp, pg, pts, K):
    """The ground-truth-centred clouds of the two nearest-neighbour columns in float64:
    (g3, q3, g2, q2) = queries / references in 3-D (metres) and 2-D (pixels)."""
    pp, pg, pts, K = (np.asarray(a, np.float64) for a in (pp, pg, pts, K))
    g3 = pts @ pg[:, :3].T
    q3 = pts @ pp[:, :3].T + (pp[:, 3] - pg[:, 3])
    c = K @ pg[:, 3]

    def pix(X):
        h = X @ K.T
        return h[:, :2] / h[:, 2:] - c[:2] / c[2]
    return g3, q3, pix(g3 + pg[:, 3]), pix(pts @ pp[:, :3].T + pp[:, 3])


def pose_columns(pp, pg, pts, K, f32_pairs=False):
    """The six columns for one pose (pp, pg [3,4]; pts [pn,3] float32 as the table holds them).

    ADD and PROJ are evaluated as (R_pred - R_gt) p + (t_pred - t_gt) and its image through K
    -- algebraically the columns' definition, without the cancellation of two nearly equal
    clouds -- in long double.  The nearest-neighbour columns are float64 throughout, or, with
    f32_pairs, the float32 pair loop of the library on the float32-rounded centred clouds.
    Also returns M = (largest |centred coordinate| in 3-D, in 2-D)."""
    L = np.longdouble
    pts = np.asarray(pts, np.float32)
    pn = pts.shape[0]
    ppl, pgl, P, Kl = (np.asarray(a, np.float64).astype(L) for a in (pp, pg, pts, K))
    d = P @ (ppl[:, :3] - pgl[:, :3]).T + (ppl[:, 3] - pgl[:, 3])
    add = np.sqrt((d * d).sum(1)).sum() / pn
    bg = (P @ pgl[:, :3].T + pgl[:, 3]) @ Kl.T
    kd = d @ Kl.T
    den = (bg[:, 2] + kd[:, 2]) * bg[:, 2]
    du = (kd[:, 0] * bg[:, 2] - bg[:, 0] * kd[:, 2]) / den
    dv = (kd[:, 1] * bg[:, 2] - bg[:, 1] * kd[:, 2]) / den
    proj = np.sqrt(du * du + dv * dv).sum() / pn
    g3, q3, g2, q2 = centred_clouds(pp, pg, pts, K)
    if f32_pairs:
        adds = np.sqrt(nearest_f32(q3, g3)[1].astype(np.float64)).mean()
        psym = np.sqrt(nearest_f32(q2, g2)[1].astype(np.float64)).mean()
    else:
        adds = _nearest_dist_f64(q3, g3).mean()
        psym = _nearest_dist_f64(q2, g2).mean()
    dt = ppl[:, 3] - pgl[:, 3]
    tr = (ppl[:, :3] * pgl[:, :3]).sum()
    cs = max((min(tr, L(3)) - 1) / 2, L(-1))
    cols = dict(add=float(add), adds=float(adds), proj=float(proj), proj_sym=float(psym),
                trans_cm=float(100 * np.sqrt((dt * dt).sum())), rot_deg=float(np.degrees(np.arccos(cs))))
    M3 = max(np.abs(g3.astype(np.float32)).max(), np.abs(q3.astype(np.float32)).max())
    M2 = max(np.abs(g2.astype(np.float32)).max(), np.abs(q2.astype(np.float32)).max())
    return cols, (float(M3), float(M2))


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def make_pose(axis, angle, t):
    return np.concatenate([rodrigues(axis, angle), np.asarray(t, np.float64)[:, None]], 1)


def symmetric_cloud(rng, n_half, scale=0.05):
    """Points closed under the 180 deg rotation about z: (x, y, z) and (-x, -y, z)."""
    h = (rng.standard_normal((n_half, 3)) * scale).astype(np.float32)
    return np.concatenate([h, h * np.array([-1, -1, 1], np.float32)])


# ----------------------------------------------------------------------------
# the library on the host
# ----------------------------------------------------------------------------
def declared_functions():
    src = open(os.path.join(REPO, "include", "pveval.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pv_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _eval_lib
    build.build()
    return _eval_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    assert build.LIBS["eval"].out == os.path.join(REPO, "pvnet_amd", "libpveval.so")
    assert b"gfx950" in open(build.LIBS["eval"].out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()


def test_header_symbols_exported(lib):
    from pvnet_amd import _eval_lib
    names = declared_functions()
    assert names == ["pv_eval_workspace_size", "pv_nearest_point_idx", "pv_pose_metrics"]
    bound = {n for n, _, _ in _eval_lib.SIGNATURES}
    for n in names:
        assert hasattr(lib, n), f"{n} declared in pveval.h but not exported"
        assert n in bound, f"{n} has no ctypes signature in pvnet_amd/_eval_lib.py"


def test_exports_only_the_abi(lib):
    from pvnet_amd import build
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIBS["eval"].out], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    names = {n for n in names if not re.fullmatch(r"__hip_cuid_[0-9a-f]+", n)}
    assert names == set(declared_functions())


def test_header_constants_match_binding():
    from pvnet_amd import _eval_lib as E
    src = open(os.path.join(REPO, "include", "pveval.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define (PV_EVAL_[A-Z_]+) (\d+u?)", src)}
    assert (defs["PV_EVAL_ADD"], defs["PV_EVAL_ADDS"], defs["PV_EVAL_PROJ"], defs["PV_EVAL_PROJ_SYM"],
            defs["PV_EVAL_CMDEG"], defs["PV_EVAL_ALL"]) == (E.PV_EVAL_ADD, E.PV_EVAL_ADDS, E.PV_EVAL_PROJ,
                                                            E.PV_EVAL_PROJ_SYM, E.PV_EVAL_CMDEG, E.PV_EVAL_ALL)
    assert defs["PV_EVAL_NCOL"] == E.PV_EVAL_NCOL == len(E.COLUMNS) == len(COLS)
    for i, c in enumerate(E.COLUMNS):
        assert defs["PV_EVAL_COL_" + c.upper()] == i and COLS[i] == c


def test_nearest_argument_errors_without_device(lib):
    p = 256     # any non-NULL value: rejected calls touch no pointer
    f = lib.pv_nearest_point_idx
    assert f(p, p, p, -1, 4, 4, 3, None) == -1
    assert f(p, p, p, 1, 0, 4, 3, None) == -1
    assert f(p, p, p, 1, 4, -1, 3, None) == -1
    for dim in (0, 1, 4):
        assert f(p, p, p, 1, 4, 4, dim, None) == -1
    assert f(None, p, p, 1, 4, 4, 3, None) == -1
    assert f(p, None, p, 1, 4, 4, 2, None) == -1
    assert f(p, p, None, 1, 4, 4, 2, None) == -1
    # nothing to do: success, no launch
    assert f(None, None, None, 0, 4, 4, 3, None) == 0
    assert f(p, None, None, 3, 4, 0, 2, None) == 0


def test_metrics_argument_errors_without_device(lib):
    from pvnet_amd import _eval_lib as E
    p = 256

    def batch(**kw):
        d = dict(b=2, total=10, pose_pred=p, pose_gt=p, model=p, model_off=p, model_id=None, nmodels=1, max_pn=10,
                 K=p, K_stride=0, metrics=E.PV_EVAL_ALL)
        d.update(kw)
        return E.EvalBatch(**d)

    def call(bt, out=p, ws=p, nbytes=1 << 20):
        return lib.pv_pose_metrics(ctypes.byref(bt) if bt is not None else None, out, ws, nbytes, None)

    assert call(None) == -1
    assert call(batch(b=-1)) == -1
    assert call(batch(nmodels=0)) == -1
    assert call(batch(max_pn=-1)) == -1
    assert call(batch(total=-1)) == -1
    assert call(batch(K_stride=-9)) == -1
    assert call(batch(metrics=32)) == -1
    assert call(batch(metrics=E.PV_EVAL_ALL | 64)) == -1
    assert call(batch(pose_pred=None)) == -1
    assert call(batch(pose_gt=None)) == -1
    assert call(batch(model=None)) == -1
    assert call(batch(model_off=None)) == -1
    assert call(batch(K=None)) == -1
    assert call(batch(), out=None) == -1
    need = lib.pv_eval_workspace_size(2, 10)
    assert need > 0
    assert call(batch(), ws=None) == -2
    assert call(batch(), nbytes=need - 1) == -2
    assert call(batch(), out=p + 4) == -3
    assert call(batch(), ws=p + 2) == -3
    # nothing to do: success, no launch
    assert call(batch(b=0), out=None, ws=None, nbytes=0) == 0
    assert call(batch(metrics=0)) == 0


def test_workspace_size_host_only(lib):
    f = lib.pv_eval_workspace_size
    assert f(0, 100) == 0 and f(-1, 100) == 0 and f(4, -1) == 0
    bs = [f(b, 1031) for b in (1, 2, 5, 64, 4096)]
    ps = [f(64, pn) for pn in (0, 1, 511, 512, 513, 2048, 4096, 4097, 32768, 1 << 20)]
    assert bs == sorted(bs) and ps == sorted(ps)
    assert bs[-1] > bs[0] and ps[-1] > ps[0]
    assert f(64, 32768) >= 64 * (32768 // 512) * 4 * 8


def test_model_table_layout():
    import torch
    from pvnet_amd.evaluation_utils import ModelTable
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal((n, 3)) for n in (5, 64, 1031))
    t = ModelTable([(a, 0.1, False), (b.astype(np.float32), 0.2, True), (c.tolist(), 0.3, False)], device="cpu")
    assert t.nmodels == 3 and t.total == 1100 and t.max_pn == 1031 and t.counts == (5, 64, 1031)
    assert t.points.dtype == torch.float32 and tuple(t.points.shape) == (1100, 3) and t.points.is_contiguous()
    assert t.offsets.dtype == torch.int32 and t.offsets.tolist() == [0, 5, 69, 1100]
    assert t.diameter.dtype == torch.float64 and t.diameter.tolist() == [0.1, 0.2, 0.3]
    assert t.symmetric.dtype == torch.bool and t.symmetric.tolist() == [False, True, False]
    assert t.any_symmetric and not t.all_symmetric
    np.testing.assert_array_equal(t.points[5:69].numpy(), b.astype(np.float32))
    e = ModelTable([(np.zeros((0, 3)), 1.0, False)], device="cpu")
    assert e.total == 0 and e.max_pn == 0 and e.offsets.tolist() == [0, 0] and tuple(e.points.shape) == (0, 3)
    with pytest.raises(ValueError):
        ModelTable([], device="cpu")


def test_python_layer_rejects_host_tensors():
    import torch
    from pvnet_amd import extend_utils as X
    from pvnet_amd.evaluation_utils import ModelTable, pose_metrics
    with pytest.raises(RuntimeError, match="device"):
        X.find_nearest_point_idx_batch(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    t = ModelTable([(np.zeros((4, 3)), 1.0, False)], device="cpu")
    with pytest.raises(RuntimeError, match="device"):
        pose_metrics(torch.zeros(1, 3, 4), torch.zeros(1, 3, 4), t, K_LM)


# ----------------------------------------------------------------------------
# the restatement, pinned
# ----------------------------------------------------------------------------
def test_restatement_nearest_known_answers():
    ref = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0]], np.float32)
    que = np.array([[0.9, 0, 0], [0.5, 0, 0], [0, 1.1, 0], [np.nan, 0, 0], [0, 0, 5]], np.float32)
    idx, d = nearest_f32(ref, que)
    # duplicate references and an equidistant query take the lowest index; NaN never wins
    assert idx.tolist() == [1, 0, 4, 0, 0] and idx.dtype == np.int32
    assert d[1] == np.float32(0.25) and np.isinf(d[3])
    assert nearest_f32(np.full((3, 2), np.nan, np.float32), que[:, :2])[0].tolist() == [0] * 5


def test_restatement_symmetric_known_answer():
    rng = np.random.default_rng(7)
    pts = symmetric_cloud(rng, 100)
    pg = make_pose([0.3, -0.5, 0.8], 0.7, [0.05, -0.02, 0.9])
    pp = np.concatenate([pg[:, :3] @ rodrigues([0, 0, 1], np.pi), pg[:, 3:]], 1)
    cols, _ = pose_columns(pp, pg, pts, K_LM)
    closed = (2 * np.sqrt(pts[:, 0].astype(np.float64) ** 2 + pts[:, 1].astype(np.float64) ** 2)).mean()
    assert cols["adds"] < 1e-12 and cols["proj_sym"] < 1e-9
    assert abs(cols["add"] - closed) <= 1e-12 * closed and closed > 0.05
    assert cols["trans_cm"] == 0.0 and abs(cols["rot_deg"] - 180.0) < 1e-6


def test_restatement_matches_naive_forms():
    """ADD / PROJ through the difference (R_pred - R_gt) p + dt equal the literal definitions."""
    rng = np.random.default_rng(3)
    pts = (rng.standard_normal((257, 3)) * 0.04).astype(np.float32)
    pg = make_pose([1, 2, 3], 0.4, [0.02, 0.01, 0.8])
    pp = make_pose([1, 2.2, 2.9], 0.47, [0.03, 0.0, 0.83])
    cols, _ = pose_columns(pp, pg, pts, K_LM)
    P = pts.astype(np.float64)
    a, b = P @ pp[:, :3].T + pp[:, 3], P @ pg[:, :3].T + pg[:, 3]
    ua, ub = a @ K_LM.T, b @ K_LM.T
    ua, ub = ua[:, :2] / ua[:, 2:], ub[:, :2] / ub[:, 2:]
    assert abs(cols["add"] - np.linalg.norm(a - b, axis=1).mean()) < 1e-13
    assert abs(cols["proj"] - np.linalg.norm(ua - ub, axis=1).mean()) < 1e-10
    assert abs(cols["trans_cm"] - 100 * np.linalg.norm(pp[:, 3] - pg[:, 3])) < 1e-12
    tr = np.trace(pp[:, :3] @ pg[:, :3].T)
    assert abs(cols["rot_deg"] - np.degrees(np.arccos((tr - 1) / 2))) < 1e-10


def test_f32_pair_loop_is_inside_the_bound():
    """The float32 arithmetic alone against float64: well inside 32 units of 2^-24 M."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for case in range(12):
        pn = int(rng.choice([65, 257, 1031]))
        if case % 3 == 0:       # grid-tied set
            pts = (rng.integers(-8, 9, (pn, 3)) * 0.01).astype(np.float32)
        else:
            pts = (rng.standard_normal((pn, 3)) * 0.05).astype(np.float32)
        ang = [1e-4, 1e-2, 0.3, np.pi][case % 4]
        pg = make_pose(rng.standard_normal(3), rng.uniform(0, np.pi), [0.03, -0.04, 0.9])
        pp = np.concatenate([rodrigues(rng.standard_normal(3), ang) @ pg[:, :3],
                             pg[:, 3:] + rng.standard_normal((3, 1)) * 1e-3], 1)
        c64, (M3, M2) = pose_columns(pp, pg, pts, K_LM)
        c32, _ = pose_columns(pp, pg, pts, K_LM, f32_pairs=True)
        worst = max(worst, abs(c32["adds"] - c64["adds"]) / (UNIT * M3),
                    abs(c32["proj_sym"] - c64["proj_sym"]) / (UNIT * M2))
    print(f"float32 pair loop vs float64: worst {worst:.3f} units of 2^-24 M")
    assert worst < 32.0
