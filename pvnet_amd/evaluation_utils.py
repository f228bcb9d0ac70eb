"""Pose evaluation on the device -- the replacement for the reference's
``lib/utils/evaluation_utils.py`` (``Evaluator``, EU:63-225): ADD < 10 % of the
diameter, ADD-S for symmetric objects, 2-D projection < 5 px and 5 cm 5 deg, for a
batch of poses and a table of models in one library call (``pv_pose_metrics``,
include/pveval.h), chained onto ``uncertainty_pnp_batch``'s output without a host
round trip.

* :class:`ModelTable` holds the models' vertices (concatenated), offsets,
  diameters and symmetry flags on the device.
* :func:`pose_metrics` returns the raw metric columns as device tensors.
* :class:`Evaluator` keeps the reference's method names (``evaluate``,
  ``evaluate_uncertainty``, ``average_precision``) with this project's argument
  lists: the reference's model database and ``cfg`` are out of
  scope.  The one host readback is in ``average_precision``.

No CPU fallback: without libpveval.so or a ROCm device the calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _eval_lib
from .ransac_voting_gpu import VotingWorkspace

ALL_METRICS = ("add", "adds", "proj", "proj_sym", "cmdeg")

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own


class ModelTable:
    """The models poses are scored against.

    models  list of ``(points [pn, 3], diameter, symmetric)``; a pose's ``model_id`` indexes it
    device  where the table lives (default: the current ROCm device)

    points f32 [total, 3] (all models, concatenated), offsets i32 [nmodels + 1] (model m is rows
    [offsets[m], offsets[m + 1])), diameter f64 [nmodels], symmetric bool [nmodels]."""

    def __init__(self, models, device=None):
        if len(models) < 1:
            raise ValueError("ModelTable needs at least one model")
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("ModelTable lives on the ROCm device (no CPU path)")
            device = torch.device("cuda", torch.cuda.current_device())
        pts, counts = [], []
        for points, _, _ in models:
            p = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
            pts.append(p)
            counts.append(p.shape[0])
        off = np.zeros(len(models) + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        if off[-1] > np.iinfo(np.int32).max:
            raise ValueError("the models have more than 2^31 - 1 vertices in all")
        self.device = torch.device(device)
        self.nmodels = len(models)
        self.total = int(off[-1])
        self.max_pn = int(max(counts))
        self.counts = tuple(int(c) for c in counts)
        self.any_symmetric = any(bool(s) for _, _, s in models)
        self.all_symmetric = all(bool(s) for _, _, s in models)
        self.points = torch.from_numpy(np.concatenate(pts) if self.total else np.zeros((0, 3), np.float32)).to(device)
        self.offsets = torch.from_numpy(off.astype(np.int32)).to(device)
        self.diameter = torch.tensor([float(d) for _, d, _ in models], dtype=torch.float64).to(device)
        self.symmetric = torch.tensor([bool(s) for _, _, s in models], dtype=torch.bool).to(device)

    @classmethod
    def from_meshes(cls, mesh_table, symmetric=False):
        """The table of a :class:`~pvnet_amd.render.MeshTable`'s models: ``points`` and ``offsets`` are
        the mesh table's own vertex tensors (not copies), and ``diameter`` is computed on the device
        (``pvnet_amd.models.diameter``), so nothing is brought from the host.

        symmetric  a bool for every model, or a sequence of one bool per model"""
        from . import models
        n = int(mesh_table.nmodels)
        sym = [bool(symmetric)] * n if isinstance(symmetric, (bool, int)) else [bool(s) for s in symmetric]
        if len(sym) != n:
            raise ValueError("symmetric must be a bool or one bool per model")
        self = cls.__new__(cls)
        self.device = mesh_table.device
        self.nmodels = n
        self.total = int(mesh_table.total_v)
        self.max_pn = int(mesh_table.max_verts)
        self.counts = tuple(int(c) for c in mesh_table.vert_counts)
        self.any_symmetric = any(sym)
        self.all_symmetric = all(sym)
        self.points = mesh_table.verts
        self.offsets = mesh_table.vert_off
        self.diameter = models.diameter(mesh_table)
        self.symmetric = torch.tensor(sym, dtype=torch.bool).to(self.device)
        return self


def _metric_bits(metrics) -> int:
    bits = 0
    for m in metrics:
        if m not in _eval_lib.METRICS:
            raise ValueError(f"unknown metric {m!r}: choose from {ALL_METRICS}")
        bits |= _eval_lib.METRICS[m][0]
    return bits


def pose_metrics(pose_pred: torch.Tensor, pose_gt: torch.Tensor, table: ModelTable, K, model_id=None,
                 metrics=ALL_METRICS, out: torch.Tensor | None = None) -> dict:
    """Score a batch of poses on the device.

    pose_pred, pose_gt  [b, 3, 4] device tensors of any float dtype (converted to float64;
                        ``uncertainty_pnp_batch``'s Rt is used in place)
    table     :class:`ModelTable` on the same device
    K         [3, 3] shared or [b, 3, 3] camera matrix
    model_id  int [b] (device tensor or anything ``torch.as_tensor`` takes), None = model 0
    metrics   any of "add", "adds", "proj", "proj_sym", "cmdeg"
    out       optional f64 [b, 6] to write into (columns of unrequested metrics are left as they are)

    Returns {"add", "adds", "proj", "proj_sym", "trans_cm", "rot_deg"} (those requested) as
    f64 [b] views of one [b, 6] tensor.  Nothing is read back and nothing synchronises."""
    dev = pose_pred.device
    if dev.type != "cuda":
        raise RuntimeError("pose_pred must be a device tensor (no CPU path)")
    if table.device != dev or pose_gt.device != dev:
        raise RuntimeError("pose_pred, pose_gt and the model table must be on the same device")
    if pose_pred.dim() != 3 or tuple(pose_pred.shape[1:]) != (3, 4) or pose_gt.shape != pose_pred.shape:
        raise RuntimeError("pose_pred and pose_gt must be [b, 3, 4]")
    b = int(pose_pred.shape[0])
    bits = _metric_bits(metrics)
    pp = pose_pred.to(torch.float64).contiguous()
    pg = pose_gt.to(torch.float64).contiguous()
    Kt = torch.as_tensor(K, dtype=torch.float64).to(dev).contiguous()
    if tuple(Kt.shape) == (3, 3):
        ks = 0
    elif tuple(Kt.shape) == (b, 3, 3):
        ks = 9
    else:
        raise RuntimeError("K must be [3, 3] or [b, 3, 3]")
    mid = None
    if model_id is not None:
        mid = torch.as_tensor(model_id).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(mid.shape) != (b,):
            raise RuntimeError("model_id must be [b]")
    if out is None:
        out = torch.empty((b, _eval_lib.PV_EVAL_NCOL), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (b, _eval_lib.PV_EVAL_NCOL) or out.device != dev or \
            not out.is_contiguous():
        raise RuntimeError("out must be a contiguous float64 [b, 6] tensor on the poses' device")
    L = _eval_lib.load()
    need = int(L.pv_eval_workspace_size(b, table.max_pn))
    ws = _ws.get(dev, need)
    bt = _eval_lib.EvalBatch(b, table.total, pp.data_ptr(), pg.data_ptr(), table.points.data_ptr(),
                             table.offsets.data_ptr(), None if mid is None else mid.data_ptr(), table.nmodels,
                             table.max_pn, Kt.data_ptr(), ks, bits)
    with torch.cuda.device(dev):
        _eval_lib.check(L.pv_pose_metrics(ctypes.byref(bt), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream(dev).cuda_stream), "pv_pose_metrics")
    res = {}
    for m in metrics:
        for c in _eval_lib.METRICS[m][1]:
            res[_eval_lib.COLUMNS[c]] = out[:, c]
    return res


class Evaluator:
    """The reference's ``Evaluator`` (EU:63-225) for batches, on the device.

    table        :class:`ModelTable`
    points_3d    [nmodels, vn, 3] (or [vn, 3] for one model): each model's 3-D keypoints, the
                 ones the voted 2-D keypoints correspond to

    ``evaluate`` and ``evaluate_uncertainty`` pose a batch, score it with :func:`pose_metrics`
    (ADD-S and the symmetric projection for models flagged symmetric, the plain forms
    otherwise) and append one device bool tensor [b] per call to the recorders
    ``projection_2d_recorder`` (< 5 px), ``add_recorder`` (< 0.1 diameter) and
    ``cm_degree_5_recorder`` (< 5 cm and < 5 deg).  ``average_precision`` reads them back."""

    def __init__(self, table: ModelTable, points_3d):
        self.table = table
        p3 = torch.as_tensor(points_3d, dtype=torch.float64).to(table.device)
        if p3.dim() == 2:
            p3 = p3[None]
        if p3.dim() != 3 or p3.shape[0] != table.nmodels or p3.shape[2] != 3:
            raise RuntimeError("points_3d must be [nmodels, vn, 3]")
        self.points_3d = p3.contiguous()
        self.projection_2d_recorder = []
        self.add_recorder = []
        self.cm_degree_5_recorder = []

    def _ids(self, model_id, b):
        dev = self.table.device
        if model_id is None:
            return torch.zeros(b, dtype=torch.int64, device=dev)
        return torch.as_tensor(model_id).to(device=dev, dtype=torch.int64)

    def _score(self, pose_pred, pose_targets, mid, K):
        t = self.table
        want = ["cmdeg"]
        if not t.all_symmetric:
            want += ["add", "proj"]
        if t.any_symmetric:
            want += ["adds", "proj_sym"]
        pose_gt = torch.as_tensor(pose_targets).to(t.device)
        m = pose_metrics(pose_pred, pose_gt, t, K, mid, want)
        safe = mid.clamp(0, t.nmodels - 1)          # an id outside the table scores NaN: a miss
        if t.all_symmetric:
            add, proj = m["adds"], m["proj_sym"]
        elif t.any_symmetric:
            sym = t.symmetric[safe]
            add = torch.where(sym, m["adds"], m["add"])
            proj = torch.where(sym, m["proj_sym"], m["proj"])
        else:
            add, proj = m["add"], m["proj"]
        self.projection_2d_recorder.append(proj < 5.0)
        self.add_recorder.append(add < 0.1 * t.diameter[safe])
        self.cm_degree_5_recorder.append((m["trans_cm"] < 5.0) & (m["rot_deg"] < 5.0))
        return pose_pred

    def evaluate(self, points_2d, pose_targets, model_id, K, method="p3p_lm"):
        """Pose from the keypoints alone, then score.  points_2d [b, vn, 2] device tensor,
        pose_targets [b, 3, 4], model_id int [b] or None, K [3, 3] or [b, 3, 3].

        method "p3p_lm" (the default): ``uncertainty_pnp_batch(..., mode="weights")`` at unit
        weights, that is P3P on points 0..3, then unweighted Levenberg-Marquardt over all points.
        method "epnp": EPnP over all points (``pnp_batch``), which is what the reference calls
        here (cv2's SOLVEPNP_EPNP, EU:19-52); needs vn >= 6.
        method "epnp_lm": EPnP, then the same Levenberg-Marquardt started from its pose."""
        from .extend_utils import pnp_batch, uncertainty_pnp_batch
        if method not in ("p3p_lm", "epnp", "epnp_lm"):
            raise ValueError(f"unknown method {method!r}: choose from 'p3p_lm', 'epnp', 'epnp_lm'")
        b, vn = int(points_2d.shape[0]), int(points_2d.shape[1])
        mid = self._ids(model_id, b)
        p3 = self.points_3d[mid.clamp(0, self.table.nmodels - 1)]
        if method == "p3p_lm":
            w = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64, device=points_2d.device).expand(b, vn, 3)
            Rt = uncertainty_pnp_batch(points_2d, w, p3, K, mode="weights")
        else:
            Rt = pnp_batch(points_2d, p3, K, method=method)
        return self._score(Rt, pose_targets, mid, K)

    def evaluate_uncertainty(self, mean, cov, pose_targets, model_id, K):
        """Pose from the voted keypoints and their covariances (``pose_from_voting``), then
        score.  mean [b, vn, 2], cov [b, vn, 2, 2] as ``estimate_voting_distribution_with_mean``
        returns them; the other arguments as in :meth:`evaluate`."""
        from .extend_utils import pose_from_voting
        mid = self._ids(model_id, int(mean.shape[0]))
        p3 = self.points_3d[mid.clamp(0, self.table.nmodels - 1)]
        Rt = pose_from_voting(mean, cov, p3, K)
        return self._score(Rt, pose_targets, mid, K)

    def bop_errors(self, pose_pred, pose_targets, syms, K, model_id=None, metrics=("mssd", "mspd")):
        """MSSD and MSPD of poses against this evaluator's table (``pvnet_amd.bop.sym_errors``; syms is a
        ``pvnet_amd.bop.SymmetryTable``).  Records nothing: the recorders keep the 2018 protocol."""
        from . import bop
        pose_gt = torch.as_tensor(pose_targets).to(self.table.device)
        return bop.sym_errors(pose_pred, pose_gt, self.table, syms, K, model_id, metrics)

    def refine_depth(self, pose_pred, model_id, depth, K, mesh_table, **kw):
        """Refine poses against the sensor's depth before they are scored (``pvnet_amd.icp.refine_depth``;
        mesh_table is a ``pvnet_amd.render.MeshTable``) -> (poses f64 [b, 3, 4], info).  Records nothing."""
        from . import icp
        return icp.refine_depth(mesh_table, pose_pred, model_id, depth, K, **kw)

    def average_precision(self, verbose: bool = False):
        """(projection 2-D, ADD, 5 cm 5 deg) hit rates over everything recorded so far: the one
        host readback of the evaluation."""
        if not self.add_recorder:
            return 0.0, 0.0, 0.0
        r = torch.stack([torch.cat(rec).to(torch.float64).mean() for rec in
                         (self.projection_2d_recorder, self.add_recorder, self.cm_degree_5_recorder)]).cpu()
        proj2d, add, cm5 = (float(v) for v in r)
        if verbose:
            print(f"2d projections metric: {proj2d}")
            print(f"ADD metric: {add}")
            print(f"5 cm 5 degree metric: {cm5}")
        return proj2d, add, cm5
