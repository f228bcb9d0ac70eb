"""Scoring poses in the BOP Challenge's terms on the device: the three pose errors MSSD, MSPD and
VSD and their average recall (include/pvbop.h; Hodan et al., "BOP Challenge 2020 on 6D Object
Localization").  The 2018 LINEMOD protocol is ``pvnet_amd.evaluation_utils``; this module is what a
result on LM-O or YCB-V since 2019 is reported in.

* :class:`SymmetryTable` holds every model's symmetry transformations on the device, made from
  BOP's ``models_info.json`` entries as BOP's ``misc.get_symmetry_transformations`` makes them.
* :func:`sym_errors` returns MSSD and MSPD, and the symmetry that attained each.
* :func:`vsd` renders the estimate's and the ground truth's depth maps (``render_labels``) and
  compares them with the sensor's.
* :func:`recall` and :func:`average_recall` turn errors into BOP19's AR_VSD, AR_MSSD, AR_MSPD and
  their mean AR.  **One estimate per ground-truth instance is assumed** (PVNet gives one pose per
  class): row i of the errors is the estimate for target i.  BOP's matching of several estimates to
  the targets of an image is out of scope.

No CPU fallback: without libpvbop.so or a ROCm device the calls raise.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _bop_lib
from .evaluation_utils import ModelTable
from .ransac_voting_gpu import VotingWorkspace

ALL_METRICS = ("mssd", "mspd")
# BOP19: the misalignment tolerances of VSD and the correctness thresholds of VSD and MSSD, as
# fractions (of the diameter, or of 1): 0.05, 0.10 .. 0.50; MSPD's are 5, 10 .. 50 px at 640 columns
FRACTIONS = tuple(0.05 * k for k in range(1, 11))
MSPD_PIXELS = tuple(5.0 * k for k in range(1, 11))

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own


def _rotation(axis, angle: float) -> np.ndarray:
    """The rotation by `angle` about `axis` (normalised here), Rodrigues' formula."""
    a = np.asarray(axis, np.float64).reshape(3)
    n = math.sqrt(float(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))
    if not n > 0.0:
        raise ValueError("a continuous symmetry's axis must not be zero")
    x, y, z = (float(v) / n for v in a)
    c, s = math.cos(angle), math.sin(angle)
    t = 1.0 - c
    return np.array([[c + x * x * t, x * y * t - z * s, x * z * t + y * s],
                     [y * x * t + z * s, c + y * y * t, y * z * t - x * s],
                     [z * x * t - y * s, z * y * t + x * s, c + z * z * t]], np.float64)


def symmetry_transformations(info: dict, max_sym_disc_step: float = 0.01) -> np.ndarray:
    """One ``models_info.json`` entry -> f64 [ns, 3, 4] rows [R | t], on the host.

    The identity first, then the discrete transformations (``symmetries_discrete``: 16 row-major
    floats each).  Each continuous symmetry (``symmetries_continuous``: ``{axis, offset}``) is
    discretised into n = ceil(pi / max_sym_disc_step) steps: the rotations by 2 pi i / n, i = 1 .. n-1,
    about the axis through the offset, t = offset - R offset.  Every discrete transformation (the
    identity included) is composed with every continuous one: R = R_d R_c, t = R_d t_c + t_d."""
    if not 0.0 < float(max_sym_disc_step) <= math.pi:
        raise ValueError("max_sym_disc_step must be in (0, pi]")
    disc = [np.eye(4)[:3]]
    for m in info.get("symmetries_discrete", ()) or ():
        m = np.asarray(m, np.float64)
        if m.size != 16:
            raise ValueError("a discrete symmetry is 16 row-major floats (a 4 x 4 transformation)")
        disc.append(m.reshape(4, 4)[:3])
    cont = []
    n = int(math.ceil(math.pi / float(max_sym_disc_step)))
    for sym in info.get("symmetries_continuous", ()) or ():
        off = np.asarray(sym.get("offset", (0.0, 0.0, 0.0)), np.float64).reshape(3)
        for i in range(1, n):
            R = _rotation(sym["axis"], 2.0 * math.pi * i / n)
            cont.append(np.concatenate([R, (off - R @ off)[:, None]], 1))
    out = []
    for d in disc:
        out.append(d)
        out += [np.concatenate([d[:, :3] @ c[:, :3], (d[:, :3] @ c[:, 3] + d[:, 3])[:, None]], 1) for c in cont]
    return np.ascontiguousarray(np.stack(out))


class SymmetryTable:
    """Every model's symmetry transformations, concatenated, on the device.

    models_info  one entry per model, in the order of the :class:`ModelTable`, each in the form of
                 BOP's ``models_info.json`` (see :func:`symmetry_transformations`); an entry without
                 symmetries gives the identity alone
    device       where the table lives (default: the current ROCm device)

    syms f64 [total_s, 3, 4], offsets i32 [nmodels + 1] (model m is rows [offsets[m], offsets[m + 1])),
    counts, max_ns."""

    def __init__(self, models_info, device=None, max_sym_disc_step: float = 0.01):
        if isinstance(models_info, dict):
            models_info = list(models_info.values())
        if len(models_info) < 1:
            raise ValueError("SymmetryTable needs at least one model")
        self._fill([symmetry_transformations(info, max_sym_disc_step) for info in models_info], device)

    def _fill(self, tables, device):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("SymmetryTable lives on the ROCm device (no CPU path)")
            device = torch.device("cuda", torch.cuda.current_device())
        tables = [np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1, 3, 4)) for t in tables]
        off = np.zeros(len(tables) + 1, np.int64)
        np.cumsum([t.shape[0] for t in tables], out=off[1:])
        if off[-1] > np.iinfo(np.int32).max:
            raise ValueError("the models have more than 2^31 - 1 symmetry transformations in all")
        self.device = torch.device(device)
        self.nmodels = len(tables)
        self.total = int(off[-1])
        self.counts = tuple(int(t.shape[0]) for t in tables)
        self.max_ns = max(self.counts)
        self.syms = torch.from_numpy(np.concatenate(tables)).to(self.device)
        self.offsets = torch.from_numpy(off.astype(np.int32)).to(self.device)

    @classmethod
    def identity(cls, nmodels: int, device=None):
        """The table for `nmodels` objects without symmetries: MSSD is then the largest vertex distance."""
        return cls.from_arrays([np.eye(4)[None, :3]] * int(nmodels), device)

    @classmethod
    def from_arrays(cls, tables, device=None):
        """From one f64 [ns, 3, 4] array per model, taken as they are."""
        if len(tables) < 1:
            raise ValueError("SymmetryTable needs at least one model")
        self = cls.__new__(cls)
        self._fill(tables, device)
        return self


def _camera(K, b, dev):
    Kt = torch.as_tensor(K, dtype=torch.float64).to(dev).contiguous()
    if tuple(Kt.shape) == (3, 3):
        return Kt, 0
    if tuple(Kt.shape) == (b, 3, 3):
        return Kt, 9
    raise RuntimeError("K must be [3, 3] or [b, 3, 3]")


def _ids(x, b, dev, name):
    if x is None:
        return None
    t = torch.as_tensor(x).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(t.shape) != (b,):
        raise RuntimeError(f"{name} must be [b]")
    return t


def sym_errors(pose_est: torch.Tensor, pose_gt: torch.Tensor, table: ModelTable, syms: SymmetryTable, K,
               model_id=None, metrics=ALL_METRICS, out: dict | None = None) -> dict:
    """MSSD and MSPD of a batch of poses on the device (``pv_bop_sym_errors``, include/pvbop.h).

    pose_est, pose_gt  [b, 3, 4] device tensors of any float dtype (converted to float64)
    table     :class:`~pvnet_amd.evaluation_utils.ModelTable` on the same device
    syms      :class:`SymmetryTable` with one entry per model of `table`
    K         [3, 3] shared or [b, 3, 3] camera matrix (read for MSPD)
    model_id  int [b], None = model 0
    metrics   any of "mssd", "mspd"
    out       optional {"err": f64 [b, 2], "best": i32 [b, 2]} to write into (an unrequested
              column is left as it is)

    Returns {"mssd", "mspd", "best_mssd", "best_mspd"} (those requested): f64 / i32 [b] views.  MSSD is
    in the model's units, MSPD in pixels; best_* is the index of the symmetry that attained the
    minimum, -1 where the error is NaN.  Nothing is read back and nothing synchronises."""
    if not isinstance(pose_est, torch.Tensor) or pose_est.device.type != "cuda":
        raise RuntimeError("pose_est must be a device tensor (no CPU path)")
    dev = pose_est.device
    if not isinstance(table, ModelTable) or not isinstance(syms, SymmetryTable):
        raise RuntimeError("table must be a ModelTable and syms a SymmetryTable")
    if table.device != dev or syms.device != dev or pose_gt.device != dev:
        raise RuntimeError("the poses, the model table and the symmetry table must be on the same device")
    if syms.nmodels != table.nmodels:
        raise RuntimeError("the symmetry table must have one entry per model")
    if pose_est.dim() != 3 or tuple(pose_est.shape[1:]) != (3, 4) or pose_gt.shape != pose_est.shape:
        raise RuntimeError("pose_est and pose_gt must be [b, 3, 4]")
    b = int(pose_est.shape[0])
    bits = 0
    for m in metrics:
        if m not in _bop_lib.METRICS:
            raise ValueError(f"unknown metric {m!r}: choose from {ALL_METRICS}")
        bits |= _bop_lib.METRICS[m][0]
    pe = pose_est.to(torch.float64).contiguous()
    pg = pose_gt.to(torch.float64).contiguous()
    Kt, ks = _camera(K, b, dev)
    mid = _ids(model_id, b, dev, "model_id")
    out = {} if out is None else out
    err, best = out.get("err"), out.get("best")
    if err is None:
        err = torch.empty((b, 2), dtype=torch.float64, device=dev)
    if best is None:
        best = torch.empty((b, 2), dtype=torch.int32, device=dev)
    for t, dt in ((err, torch.float64), (best, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (b, 2) or t.device != dev or not t.is_contiguous():
            raise RuntimeError("out['err'] must be float64 [b, 2] and out['best'] int32 [b, 2], contiguous, on the poses' device")
    L = _bop_lib.load()
    need = int(L.pv_bop_workspace_size(b, table.max_pn, syms.max_ns))
    ws = _ws.get(dev, need)
    bt = _bop_lib.BopBatch(b, table.total, syms.total, table.nmodels, table.max_pn, syms.max_ns, bits, 0,
                           pe.data_ptr(), pg.data_ptr(), table.points.data_ptr(), table.offsets.data_ptr(),
                           None if mid is None else mid.data_ptr(), syms.syms.data_ptr(), syms.offsets.data_ptr(),
                           Kt.data_ptr(), ks)
    with torch.cuda.device(dev):
        _bop_lib.check(L.pv_bop_sym_errors(ctypes.byref(bt), err.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream(dev).cuda_stream), "pv_bop_sym_errors")
    res = {}
    for m in metrics:
        c = _bop_lib.METRICS[m][1]
        res[m], res["best_" + m] = err[:, c], best[:, c]
    return res


def vsd_maps(depth_test: torch.Tensor, depth_est: torch.Tensor, depth_gt: torch.Tensor, K, taus: torch.Tensor,
             delta: float, img_id=None) -> dict:
    """VSD from three depth maps (``pv_bop_vsd``): depth_test f32 [n_img, H, W] (0 = missing), depth_est
    and depth_gt f32 [b, H, W] as ``render_labels`` writes them, taus f64 [b, ntau] in depth units.
    Returns {"err": f64 [b, ntau], "counts": i64 [b, 2 + ntau] = (union, inter, ge_0 ..)}."""
    if not isinstance(depth_est, torch.Tensor) or depth_est.device.type != "cuda":
        raise RuntimeError("depth_est must be a device tensor (no CPU path)")
    dev = depth_est.device
    if depth_test.device != dev or depth_gt.device != dev or taus.device != dev:
        raise RuntimeError("the depth maps and taus must be on the same device")
    if depth_est.dim() != 3 or depth_gt.shape != depth_est.shape or depth_test.dim() != 3 or \
            depth_test.shape[1:] != depth_est.shape[1:]:
        raise RuntimeError("depth_test must be [n_img, H, W], depth_est and depth_gt [b, H, W]")
    b, H, W = (int(v) for v in depth_est.shape)
    if taus.dim() != 2 or int(taus.shape[0]) != b or not 1 <= int(taus.shape[1]) <= _bop_lib.PV_BOP_MAX_TAUS:
        raise RuntimeError("taus must be [b, ntau] with 1 <= ntau <= 32")
    if not (math.isfinite(float(delta)) and float(delta) >= 0.0):
        raise RuntimeError("delta must be finite and not negative")
    ntau = int(taus.shape[1])
    dt = depth_test.to(torch.float32).contiguous()
    de = depth_est.to(torch.float32).contiguous()
    dg = depth_gt.to(torch.float32).contiguous()
    tt = taus.to(torch.float64).contiguous()
    Kt, ks = _camera(K, b, dev)
    iid = _ids(img_id, b, dev, "img_id")
    counts = torch.empty((b, 2 + ntau), dtype=torch.int64, device=dev)
    err = torch.empty((b, ntau), dtype=torch.float64, device=dev)
    bt = _bop_lib.VsdBatch(b, int(dt.shape[0]), H, W, ntau, 0, dt.data_ptr(), None if iid is None else iid.data_ptr(),
                           de.data_ptr(), dg.data_ptr(), Kt.data_ptr(), ks, float(delta), tt.data_ptr())
    L = _bop_lib.load()
    with torch.cuda.device(dev):
        _bop_lib.check(L.pv_bop_vsd(ctypes.byref(bt), counts.data_ptr(), err.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream), "pv_bop_vsd")
    return {"err": err, "counts": counts}


def vsd(depth_test: torch.Tensor, pose_est: torch.Tensor, pose_gt: torch.Tensor, mesh_table, K, model_id, diameter,
        img_id=None, delta: float = 15.0, taus=FRACTIONS, znear: float = 1e-3, max_frames: int = 64) -> dict:
    """VSD of a batch of poses: both poses' depth maps are rendered (``render_labels``, one instance per
    virtual frame) in chunks of `max_frames` poses, and each chunk is scored by one ``pv_bop_vsd`` call.

    depth_test  f32 [n_img, H, W] device tensor: the sensor's depth, 0 where it is missing, in the
                units of the meshes and the poses' translations
    pose_est, pose_gt  [b, 3, 4] device tensors
    mesh_table  :class:`~pvnet_amd.render.MeshTable`
    K           [3, 3] shared or [b, 3, 3]
    model_id    int [b], or None = model 0
    diameter    f64 [nmodels] (e.g. ``ModelTable.diameter``) or one number: scales `taus`
    img_id      int [b]: the sensor image of each pose; None = image i for pose i
    delta       the visibility tolerance in depth units (BOP: 15 mm)
    taus        the misalignment tolerances as fractions of the diameter (BOP19: 0.05 .. 0.5)

    Returns {"err": f64 [b, ntau], "counts": i64 [b, 2 + ntau]}."""
    from .render import render_labels
    if not isinstance(pose_est, torch.Tensor) or pose_est.device.type != "cuda":
        raise RuntimeError("pose_est must be a device tensor (no CPU path)")
    dev = pose_est.device
    if pose_est.dim() != 3 or tuple(pose_est.shape[1:]) != (3, 4) or pose_gt.shape != pose_est.shape:
        raise RuntimeError("pose_est and pose_gt must be [b, 3, 4]")
    if depth_test.dim() != 3:
        raise RuntimeError("depth_test must be [n_img, H, W]")
    if int(max_frames) < 1:
        raise RuntimeError("max_frames must be at least 1")
    b, H, W = int(pose_est.shape[0]), int(depth_test.shape[1]), int(depth_test.shape[2])
    Kt, ks = _camera(K, b, dev)
    mid = torch.zeros(b, dtype=torch.int32, device=dev) if model_id is None else _ids(model_id, b, dev, "model_id")
    iid = torch.arange(b, dtype=torch.int32, device=dev) if img_id is None else _ids(img_id, b, dev, "img_id")
    dia = torch.as_tensor(diameter, dtype=torch.float64).to(dev).reshape(-1)
    frac = torch.as_tensor(taus, dtype=torch.float64).to(dev).reshape(-1)
    per_pose = dia[mid.long().clamp(0, dia.numel() - 1)] if dia.numel() > 1 else dia.expand(b)
    tt = per_pose[:, None] * frac[None, :]                              # on the device: nothing is read back
    errs, counts = [], []
    for lo in range(0, b, int(max_frames)):
        hi = min(b, lo + int(max_frames))
        Kc = Kt if ks == 0 else Kt[lo:hi]
        maps = [render_labels(mesh_table, p[lo:hi, None].to(torch.float64), mid[lo:hi, None], None, Kc, H, W, znear=znear,
                              want=("depth",))["depth"] for p in (pose_est, pose_gt)]
        r = vsd_maps(depth_test, maps[0], maps[1], Kc, tt[lo:hi], delta, iid[lo:hi])
        errs.append(r["err"])
        counts.append(r["counts"])
    if not errs:
        return {"err": torch.empty((0, frac.numel()), dtype=torch.float64, device=dev),
                "counts": torch.empty((0, 2 + frac.numel()), dtype=torch.int64, device=dev)}
    return {"err": torch.cat(errs), "counts": torch.cat(counts)}


def recall(err: torch.Tensor, thresholds) -> torch.Tensor:
    """The fraction of (error, threshold) pairs with error < threshold -> f64 device scalar.

    err         [b] or [b, k] device tensor; NaN is a miss
    thresholds  [t] (the same for every pose) or [b, t] (per pose, e.g. fractions of each diameter)"""
    e = err.to(torch.float64).reshape(err.shape[0], -1)
    th = torch.as_tensor(thresholds, dtype=torch.float64).to(e.device)
    th = th.reshape(1, -1) if th.dim() < 2 else th
    if e.numel() == 0:
        return torch.zeros((), dtype=torch.float64, device=e.device)
    return (e[:, :, None] < th[:, None, :]).to(torch.float64).mean()    # a NaN compares false


def average_recall(mssd: torch.Tensor, mspd: torch.Tensor, vsd_err: torch.Tensor, diameter: torch.Tensor, width: int,
                   fractions=FRACTIONS, pixels=MSPD_PIXELS) -> dict:
    """BOP19's average recall of one estimate per ground-truth instance.

    mssd, mspd  f64 [b] (:func:`sym_errors`);  vsd_err f64 [b, ntau] (:func:`vsd` at BOP19's taus)
    diameter    f64 [b]: each pose's model diameter (``table.diameter[model_id]``)
    width       the image's columns: MSPD's thresholds are 5 .. 50 px times width / 640

    AR_VSD is the recall of vsd_err < theta over every tau and theta in `fractions`, AR_MSSD that of
    mssd < theta * diameter, AR_MSPD that of mspd < theta px * width / 640; AR is their mean.
    Returns {"ar_vsd", "ar_mssd", "ar_mspd", "ar"} as floats: the one host readback."""
    dev = mssd.device
    fr = torch.as_tensor(fractions, dtype=torch.float64).to(dev)
    px = torch.as_tensor(pixels, dtype=torch.float64).to(dev) * (float(width) / 640.0)
    dia = torch.as_tensor(diameter, dtype=torch.float64).to(dev).reshape(-1)
    parts = torch.stack([recall(vsd_err, fr), recall(mssd, dia[:, None] * fr[None, :]), recall(mspd, px)])
    v, s, p = (float(x) for x in parts.cpu())
    return {"ar_vsd": v, "ar_mssd": s, "ar_mspd": p, "ar": (v + s + p) / 3.0}
