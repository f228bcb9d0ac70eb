"""Uncertainty-weighted PnP on the device -- drop-in for the reference's
``lib.utils.extend_utils.extend_utils.uncertainty_pnp`` / ``uncertainty_pnp_v2``
(extend_utils.py:63-166) and for the covariance -> weight step of
``Evaluator.evaluate_uncertainty`` (lib/utils/evaluation_utils.py:161-190).

The reference runs, per image and on the host, ``cv2.solvePnP(SOLVEPNP_P3P)``
for an initial pose and then Ceres (src/uncertainty_pnp.cpp) through cffi.
Here the whole stage is one batched HIP kernel (``pv_uncertainty_pnp``: one
wave per image, fp64) behind the same Python signatures:

* ``uncertainty_pnp(points_2d, weights_2d, points_3d, camera_matrix)`` and
  ``uncertainty_pnp_v2(points_2d, covars, points_3d, camera_matrix)`` take
  and return numpy arrays like the reference (Rt [3, 4] float64) and run on
  the current ROCm device;
* ``uncertainty_pnp_batch`` is the batched device form (torch tensors in,
  Rt [b, 3, 4] float64 out, on the inputs' device and current stream), fed
  directly by ``estimate_voting_distribution_with_mean``'s (mean, cov).

No CPU fallback: without libpvvote.so or a ROCm device the calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

_MODES = {"weights": _lib.PV_PNP_WEIGHTS, "cov": _lib.PV_PNP_COV, "cov_v2": _lib.PV_PNP_COV_V2}


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("uncertainty_pnp runs on the ROCm device (no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def uncertainty_pnp_batch(points_2d: torch.Tensor, wgt: torch.Tensor, points_3d, camera_matrix, mode: str = "cov",
                          init_rt: torch.Tensor | None = None, diag: dict | None = None) -> torch.Tensor:
    """Batched uncertainty PnP on the device.

    points_2d  [b, pn, 2] the voted keypoints (e.g. ransac_voting_layer_v3's output); float64
               points are used at full precision (the reference's single-image path passes
               float64, extend_utils.py:80), anything else as float32
    wgt        mode "cov" / "cov_v2": f32 [b, pn, 2, 2] covariances (estimate_voting_distribution*);
               mode "weights": f64 [b, pn, 3] (wxx, wxy, wyy)
    points_3d  f64 [pn, 3] shared, or [b, pn, 3]
    camera_matrix f64 [3, 3] shared, or [b, 3, 3]
    init_rt    optional f64 [b, 6]: skip the P3P initialisation and refine from these poses
               (src/uncertainty_pnp.cpp:58-92; mode "weights" only); the result is then [b, 6]
    Returns Rt f64 [b, 3, 4] (or the refined [b, 6] poses with init_rt).
    """
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {sorted(_MODES)}")
    dev = points_2d.device
    if dev.type != "cuda":
        raise RuntimeError("points_2d must be a device tensor")
    b, pn = int(points_2d.shape[0]), int(points_2d.shape[1])
    if points_2d.dim() != 3 or points_2d.shape[2] != 2:
        raise RuntimeError("points_2d must be [b, pn, 2]")
    if not 4 <= pn <= 64:
        raise RuntimeError("uncertainty_pnp needs 4 <= pn <= 64 points per image")
    p2 = points_2d.contiguous() if points_2d.dtype == torch.float64 else points_2d.to(torch.float32).contiguous()
    if mode == "weights":
        w = wgt.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(w.shape) != (b, pn, 3):
            raise RuntimeError("weights must be [b, pn, 3]")
    else:
        w = wgt.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(w.shape) != (b, pn, 2, 2):
            raise RuntimeError("covariances must be [b, pn, 2, 2]")
    p3 = torch.as_tensor(points_3d, dtype=torch.float64).to(dev).contiguous()
    K = torch.as_tensor(camera_matrix, dtype=torch.float64).to(dev).contiguous()
    if p3.dim() == 2:
        if tuple(p3.shape) != (pn, 3):
            raise RuntimeError("points_3d must be [pn, 3] or [b, pn, 3]")
        p3s = 0
    elif tuple(p3.shape) == (b, pn, 3):
        p3s = pn * 3
    else:
        raise RuntimeError("points_3d must be [pn, 3] or [b, pn, 3]")
    if K.dim() == 2:
        if tuple(K.shape) != (3, 3):
            raise RuntimeError("camera_matrix must be [3, 3] or [b, 3, 3]")
        ks = 0
    elif tuple(K.shape) == (b, 3, 3):
        ks = 9
    else:
        raise RuntimeError("camera_matrix must be [3, 3] or [b, 3, 3]")
    f64 = p2.dtype == torch.float64
    bt = _lib.PnpBatch(b, pn, _MODES[mode], None if f64 else p2.data_ptr(), w.data_ptr(), p3.data_ptr(), K.data_ptr(),
                       p3s, ks, p2.data_ptr() if f64 else None)
    dg = _lib.PnpDiag()
    keep = []
    if diag is not None:
        d = dict(init_rt=torch.zeros((b, 6), dtype=torch.float64, device=dev),
                 p3p_ok=torch.zeros(b, dtype=torch.int32, device=dev),
                 iterations=torch.zeros(b, dtype=torch.int32, device=dev),
                 status=torch.zeros(b, dtype=torch.int32, device=dev),
                 cost=torch.zeros(b, dtype=torch.float64, device=dev))
        dg = _lib.PnpDiag(*(d[k].data_ptr() for k in ("init_rt", "p3p_ok", "iterations", "status", "cost")))
        keep.append(d)
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if init_rt is not None:
            if mode != "weights":
                raise RuntimeError("init_rt needs mode='weights' (the reference C entry point takes weights)")
            x0 = init_rt.to(device=dev, dtype=torch.float64).contiguous()
            if tuple(x0.shape) != (b, 6):
                raise RuntimeError("init_rt must be [b, 6]")
            out = torch.empty((b, 6), dtype=torch.float64, device=dev)
            _lib.check(L.pv_uncertainty_pnp_refine(ctypes.byref(bt), x0.data_ptr(), out.data_ptr(), ctypes.byref(dg),
                                                   stream), "pv_uncertainty_pnp_refine")
        else:
            out = torch.empty((b, 3, 4), dtype=torch.float64, device=dev)
            _lib.check(L.pv_uncertainty_pnp(ctypes.byref(bt), out.data_ptr(), ctypes.byref(dg), stream),
                       "pv_uncertainty_pnp")
    if diag is not None:
        diag.update(keep[0])
    return out


def _single(points_2d, wgt, points_3d, camera_matrix, mode):
    pn = np.asarray(points_2d).shape[0]
    assert np.asarray(points_3d).shape[0] == pn and pn >= 4          # EU:72
    dev = _device()
    p2 = torch.from_numpy(np.ascontiguousarray(points_2d, np.float64)).to(dev)[None]   # EU:80
    w = np.ascontiguousarray(wgt, np.float64 if mode == "weights" else np.float32)
    w = torch.from_numpy(w).to(dev)[None]
    Rt = uncertainty_pnp_batch(p2, w, np.asarray(points_3d, np.float64), np.asarray(camera_matrix, np.float64), mode)
    return Rt[0].cpu().numpy()


def uncertainty_pnp(points_2d, weights_2d, points_3d, camera_matrix):
    """EU:63-114: points_2d [pn, 2], weights_2d [pn, 3] (wxx, wxy, wyy),
    points_3d [pn, 3], camera_matrix [3, 3] -> Rt [3, 4] float64."""
    return _single(points_2d, weights_2d, points_3d, camera_matrix, "weights")


def uncertainty_pnp_v2(points_2d, covars, points_3d, camera_matrix, type="single"):   # noqa: A002 (reference name)
    """EU:116-166: covars [pn, 2, 2] -> isotropic weights 1 / max eigenvalue -> Rt [3, 4]."""
    return _single(points_2d, covars, points_3d, camera_matrix, "cov_v2")


_PNP_METHODS = ("epnp", "epnp_lm")
# device -> every f64 [n, 3] buffer of rows (1, 0, 1) ever handed out, the largest last.  A captured
# graph holds a buffer's raw pointer, so none is ever released: a larger request adds a buffer.
_unit_weights: dict = {}


def _unit_w(dev: torch.device, n: int) -> torch.Tensor:
    bufs = _unit_weights.setdefault(dev, [])
    if not bufs or bufs[-1].shape[0] < n:
        bufs.append(torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64, device=dev).repeat(max(n, 1024), 1).contiguous())
    return bufs[-1][:n]


def pnp_batch(points_2d: torch.Tensor, points_3d, camera_matrix, method: str = "epnp",
              diag: dict | None = None) -> torch.Tensor:
    """Batched plain PnP on the device: EPnP (``pv_epnp``, include/pvpose.h), the reference's
    ``pnp()`` (lib/utils/evaluation_utils.py:19-52, cv2's SOLVEPNP_EPNP) for a batch.

    points_2d  [b, pn, 2] device tensor, 6 <= pn <= 64; float64 points are used at full
               precision, anything else as float32
    points_3d  f64 [pn, 3] shared, or [b, pn, 3]
    camera_matrix f64 [3, 3] shared, or [b, 3, 3]
    method     "epnp": the EPnP pose as cv2's EPNP flag returns it (no refinement);
               "epnp_lm": EPnP, then the unweighted Levenberg-Marquardt of
               ``pv_uncertainty_pnp_refine`` at unit weights over all points, started from it
    diag       optional dict, filled with the device tensors ``status`` i32 [b] (0 ok, 1 degenerate:
               the pose is then [I | 0]), ``n_used`` i32 [b] and ``cand_err`` f64 [b, 3]; for
               "epnp_lm" also the refinement's ``iterations``, ``lm_status`` and ``cost``
    Returns Rt f64 [b, 3, 4] on the inputs' device and current stream.  Nothing is read back and
    nothing synchronises; after one eager call of the same shape the call can be captured."""
    from . import _pose_lib
    if method not in _PNP_METHODS:
        raise ValueError(f"method must be one of {_PNP_METHODS}")
    dev = points_2d.device
    if dev.type != "cuda":
        raise RuntimeError("points_2d must be a device tensor")
    if points_2d.dim() != 3 or points_2d.shape[2] != 2:
        raise RuntimeError("points_2d must be [b, pn, 2]")
    b, pn = int(points_2d.shape[0]), int(points_2d.shape[1])
    if not _pose_lib.PV_EPNP_MIN_POINTS <= pn <= _pose_lib.PV_EPNP_MAX_POINTS:
        raise RuntimeError(f"EPnP needs 6 <= pn <= 64 points per image, got {pn}: with fewer than 6 the null "
                           "space of its linear system is not unique; use Evaluator.evaluate(method=\"p3p_lm\") "
                           "or uncertainty_pnp_batch (p3p_lm: P3P, then Levenberg-Marquardt) for 4 or 5 points")
    p2 = points_2d.contiguous() if points_2d.dtype == torch.float64 else points_2d.to(torch.float32).contiguous()
    p3 = torch.as_tensor(points_3d, dtype=torch.float64).to(dev).contiguous()
    K = torch.as_tensor(camera_matrix, dtype=torch.float64).to(dev).contiguous()
    if tuple(p3.shape) == (pn, 3):
        p3s = 0
    elif tuple(p3.shape) == (b, pn, 3):
        p3s = pn * 3
    else:
        raise RuntimeError("points_3d must be [pn, 3] or [b, pn, 3]")
    if tuple(K.shape) == (3, 3):
        ks = 0
    elif tuple(K.shape) == (b, 3, 3):
        ks = 9
    else:
        raise RuntimeError("camera_matrix must be [3, 3] or [b, 3, 3]")
    f64 = p2.dtype == torch.float64
    bt = _pose_lib.EpnpBatch(b, pn, None if f64 else p2.data_ptr(), p2.data_ptr() if f64 else None, p3.data_ptr(),
                             K.data_ptr(), p3s, ks)
    dg = _pose_lib.EpnpDiag()
    d = {}
    if diag is not None:
        d = dict(status=torch.zeros(b, dtype=torch.int32, device=dev),
                 n_used=torch.zeros(b, dtype=torch.int32, device=dev),
                 cand_err=torch.zeros((b, 3), dtype=torch.float64, device=dev))
        dg = _pose_lib.EpnpDiag(*(d[k].data_ptr() for k in ("status", "n_used", "cand_err")))
    P = _pose_lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((b, 3, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        if method == "epnp":
            _pose_lib.check(P.pv_epnp(ctypes.byref(bt), out.data_ptr(), None, ctypes.byref(dg), stream), "pv_epnp")
        else:
            L = _lib.load()
            x0 = torch.empty((b, 6), dtype=torch.float64, device=dev)
            x1 = torch.empty((b, 6), dtype=torch.float64, device=dev)
            w = _unit_w(dev, b * pn)
            _pose_lib.check(P.pv_epnp(ctypes.byref(bt), None, x0.data_ptr(), ctypes.byref(dg), stream), "pv_epnp")
            lbt = _lib.PnpBatch(b, pn, _lib.PV_PNP_WEIGHTS, None if f64 else p2.data_ptr(), w.data_ptr(),
                                p3.data_ptr(), K.data_ptr(), p3s, ks, p2.data_ptr() if f64 else None)
            ldg = _lib.PnpDiag()
            if diag is not None:
                d.update(iterations=torch.zeros(b, dtype=torch.int32, device=dev),
                         lm_status=torch.zeros(b, dtype=torch.int32, device=dev),
                         cost=torch.zeros(b, dtype=torch.float64, device=dev))
                ldg = _lib.PnpDiag(None, None, d["iterations"].data_ptr(), d["lm_status"].data_ptr(),
                                   d["cost"].data_ptr())
            _lib.check(L.pv_uncertainty_pnp_refine(ctypes.byref(lbt), x0.data_ptr(), x1.data_ptr(),
                                                   ctypes.byref(ldg), stream), "pv_uncertainty_pnp_refine")
            _pose_lib.check(P.pv_rt6_to_Rt(x1.data_ptr(), out.data_ptr(), b, stream), "pv_rt6_to_Rt")
    if diag is not None:
        diag.update(d)
    return out


def pnp(points_3d, points_2d, camera_matrix, method: str = "epnp"):
    """The reference's ``evaluation_utils.pnp`` (EU:19-52) in its own argument order: points_3d
    [pn, 3], points_2d [pn, 2], camera_matrix [3, 3] numpy -> Rt [3, 4] float64, on the current
    ROCm device (one image of :func:`pnp_batch`)."""
    dev = _device()
    p2 = torch.from_numpy(np.ascontiguousarray(points_2d, np.float64)).to(dev)[None]
    Rt = pnp_batch(p2, np.asarray(points_3d, np.float64), np.asarray(camera_matrix, np.float64), method)
    return Rt[0].cpu().numpy()


def find_nearest_point_idx_batch(ref_pts: torch.Tensor, que_pts: torch.Tensor) -> torch.Tensor:
    """Batched device form of :func:`find_nearest_point_idx`: ref [b, pn1, dim], que [b, pn2, dim]
    (dim 2 or 3) -> int32 [b, pn2], the lowest index of the nearest reference of each query
    (include/pveval.h states the fp32 arithmetic), on the inputs' device and current stream."""
    from . import _eval_lib
    if ref_pts.device.type != "cuda" or que_pts.device != ref_pts.device:
        raise RuntimeError("ref_pts and que_pts must be tensors on the same ROCm device")
    if ref_pts.dim() != 3 or que_pts.dim() != 3 or ref_pts.shape[2] not in (2, 3) or \
            que_pts.shape[2] != ref_pts.shape[2] or que_pts.shape[0] != ref_pts.shape[0]:
        raise RuntimeError("ref_pts must be [b, pn1, dim] and que_pts [b, pn2, dim] with dim 2 or 3")
    b, pn1, dim = (int(n) for n in ref_pts.shape)
    pn2 = int(que_pts.shape[1])
    if pn1 < 1:
        raise RuntimeError("find_nearest_point_idx needs at least one reference point")
    dev = ref_pts.device
    ref = ref_pts.to(torch.float32).contiguous()
    que = que_pts.to(torch.float32).contiguous()
    idx = torch.empty((b, pn2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _eval_lib.check(_eval_lib.load().pv_nearest_point_idx(ref.data_ptr(), que.data_ptr(), idx.data_ptr(), b, pn1,
                                                              pn2, dim, torch.cuda.current_stream(dev).cuda_stream),
                        "pv_nearest_point_idx")
    return idx


def find_nearest_point_idx(ref_pts, que_pts):
    """extend_utils.py's find_nearest_point_idx (the cffi wrapper of
    src/nearest_neighborhood.cu:48,84): ref_pts [pn1, dim], que_pts [pn2, dim] numpy,
    dim 2 or 3 -> int32 [pn2], on the current ROCm device."""
    dev = _device()
    ref = torch.from_numpy(np.ascontiguousarray(ref_pts, np.float32)).to(dev)[None]
    que = torch.from_numpy(np.ascontiguousarray(que_pts, np.float32)).to(dev)[None]
    return find_nearest_point_idx_batch(ref, que)[0].cpu().numpy()


def pose_from_voting(mean: torch.Tensor, cov: torch.Tensor, points_3d, camera_matrix) -> torch.Tensor:
    """Evaluator.evaluate_uncertainty's pose step (evaluation_utils.py:161-187)
    for a batch: keypoints [b, vn, 2] and covariances [b, vn, 2, 2] from
    estimate_voting_distribution_with_mean -> Rt [b, 3, 4] (weights
    inv(sqrtm(cov)), zero for cov[0,0] < 1e-6 or NaN)."""
    return uncertainty_pnp_batch(mean, cov, points_3d, camera_matrix, "cov")
