"""Model preparation on the device: everything the pipeline needs to know about a model, from its
points alone (include/pvmodel.h).

* :func:`extent`           bounding box, centroid and count of finite points
* :func:`farthest_points`  farthest-point sampling with a deterministic tie rule (the reference's
  ``extend_utils/src/farthest_point_sampling.cpp``, batched over the table)
* :func:`diameter`         the largest distance between two points of each model
* :func:`corners_3d`       the 8 box corners in the reference's ``get_corners_3d`` order
* :func:`keypoints_3d`     n farthest points and the centre: what ``render_ground_truth`` and
  ``pnp_batch`` take as ``points_3d``

Every function takes a :class:`~pvnet_amd.render.MeshTable` (its vertices) or a
:class:`~pvnet_amd.evaluation_utils.ModelTable` (its points), returns device tensors, reads nothing
back and synchronises nothing.  No CPU fallback: without libpvmodel.so or a ROCm device the calls
raise.  ``ModelTable.from_meshes`` (evaluation_utils) builds the metrics' table from a mesh table
with :func:`diameter`.
"""
from __future__ import annotations

import ctypes

import torch

from . import _model_lib
from .ransac_voting_gpu import VotingWorkspace

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own

_START = {"centroid": _model_lib.PV_FPS_START_CENTROID, "centroid_kept": _model_lib.PV_FPS_START_CENTROID_KEPT}


def _points(table):
    """-> (points f32 [total, 3], offsets i32 [nmodels + 1], nmodels, total, max_pn) of either table."""
    if all(hasattr(table, n) for n in ("verts", "vert_off", "max_verts")):
        pts, off, mx = table.verts, table.vert_off, table.max_verts
    elif all(hasattr(table, n) for n in ("points", "offsets", "max_pn")):
        pts, off, mx = table.points, table.offsets, table.max_pn
    else:
        raise RuntimeError("table must be a MeshTable or a ModelTable")
    if pts.device.type != "cuda":
        raise RuntimeError("the table must live on the ROCm device (no CPU path)")
    if pts.dtype != torch.float32 or off.dtype != torch.int32 or not pts.is_contiguous() or not off.is_contiguous() \
            or off.device != pts.device:
        raise RuntimeError("the table's points must be contiguous float32 [total, 3] and its offsets int32, on one device")
    return pts, off, int(off.shape[0]) - 1, int(pts.shape[0]), int(mx)


def _desc(pts, off, nmodels, total, max_pn):
    return _model_lib.ModelPoints(pts.data_ptr(), off.data_ptr(), nmodels, total, max_pn, 0)


def _workspace(L, dev, nmodels, total, k):
    need = int(L.pv_model_workspace_size(nmodels, total, k))
    if need == 0:
        raise RuntimeError("bad sizes for libpvmodel.so's workspace")
    return _ws.get(dev, need)


def extent(table) -> dict:
    """-> {"bbox_min", "bbox_max", "centroid": f64 [nmodels, 3], "count": i32 [nmodels]}.

    The box is the exact minimum and maximum over the model's finite points, the centroid their
    mean with the sum taken in include/pvmodel.h's fixed order (the same bits on every run), count
    their number.  A model without a finite point has count 0 and NaN elsewhere."""
    pts, off, nmodels, total, max_pn = _points(table)
    dev = pts.device
    bbox = torch.empty((nmodels, 2, 3), dtype=torch.float64, device=dev)
    cen = torch.empty((nmodels, 3), dtype=torch.float64, device=dev)
    cnt = torch.empty((nmodels,), dtype=torch.int32, device=dev)
    d = _desc(pts, off, nmodels, total, max_pn)
    with torch.cuda.device(dev):
        _model_lib.check(_model_lib.load().pv_model_extent(ctypes.byref(d), bbox.data_ptr(), cen.data_ptr(), cnt.data_ptr(),
                                                           torch.cuda.current_stream(dev).cuda_stream), "pv_model_extent")
    return {"bbox_min": bbox[:, 0], "bbox_max": bbox[:, 1], "centroid": cen, "count": cnt}


def farthest_points(table, k: int, start="centroid", with_d2: bool = False):
    """Farthest-point sampling of every model -> ``(idx i32 [nmodels, k], points f64 [nmodels, k, 3])``.

    start  "centroid": pick 0 is the point farthest from the centroid, and the sampling goes on from
           that point alone; "centroid_kept": the same pick 0, but the centroid counts as already
           sampled (the form for a keypoint set whose last member is the centre); or an int tensor
           [nmodels]: pick 0 is that index of each model (the reference's form, with its random
           first index made an argument)
    with_d2  also return f64 [nmodels, k]: the squared distance that won each pick

    A tie goes to the lowest index.  k may exceed a model's point count: picks then repeat.  A model
    without a finite point, or with a bad start index, has idx -1 and NaN points."""
    pts, off, nmodels, total, max_pn = _points(table)
    dev = pts.device
    k = int(k)
    if not 1 <= k <= _model_lib.PV_MODEL_MAX_K:
        raise RuntimeError(f"k must be in 1..{_model_lib.PV_MODEL_MAX_K}")
    sidx = None
    if isinstance(start, str):
        if start not in _START:
            raise RuntimeError("start must be 'centroid', 'centroid_kept' or an int tensor [nmodels]")
        mode = _START[start]
    else:
        sidx = torch.as_tensor(start).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(sidx.shape) != (nmodels,):
            raise RuntimeError("start must be 'centroid', 'centroid_kept' or an int tensor [nmodels]")
        mode = _model_lib.PV_FPS_START_INDEX
    idx = torch.empty((nmodels, k), dtype=torch.int32, device=dev)
    picked = torch.empty((nmodels, k, 3), dtype=torch.float64, device=dev)
    pd2 = torch.empty((nmodels, k), dtype=torch.float64, device=dev) if with_d2 else None
    L = _model_lib.load()
    ws = _workspace(L, dev, nmodels, total, k)
    d = _desc(pts, off, nmodels, total, max_pn)
    with torch.cuda.device(dev):
        _model_lib.check(L.pv_farthest_points(ctypes.byref(d), k, mode, None if sidx is None else sidx.data_ptr(),
                                              idx.data_ptr(), picked.data_ptr(), None if pd2 is None else pd2.data_ptr(),
                                              ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                         "pv_farthest_points")
    return (idx, picked, pd2) if with_d2 else (idx, picked)


def diameter(table) -> torch.Tensor:
    """The largest distance between two finite points of each model -> f64 [nmodels] (0 for a single
    point, NaN for none): all pairs, in fp64, the same bits on every run."""
    pts, off, nmodels, total, max_pn = _points(table)
    dev = pts.device
    out = torch.empty((nmodels,), dtype=torch.float64, device=dev)
    L = _model_lib.load()
    ws = _workspace(L, dev, nmodels, total, 1)
    d = _desc(pts, off, nmodels, total, max_pn)
    with torch.cuda.device(dev):
        _model_lib.check(L.pv_model_diameter(ctypes.byref(d), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream(dev).cuda_stream), "pv_model_diameter")
    return out


def corners_3d(table) -> torch.Tensor:
    """The 8 corners of each model's bounding box -> f64 [nmodels, 8, 3].  Corner c has x = max if
    c & 4 else min, y by c & 2 and z by c & 1: the reference's ``get_corners_3d`` order."""
    e = extent(table)
    c = torch.arange(8, device=e["centroid"].device)
    hi = torch.stack([(c & 4) != 0, (c & 2) != 0, (c & 1) != 0], 1)        # [8, 3]
    return torch.where(hi[None], e["bbox_max"][:, None], e["bbox_min"][:, None])


def keypoints_3d(table, n: int = 8, centre: str = "centroid", start="centroid") -> torch.Tensor:
    """The n farthest points of each model, then its centre -> f64 [nmodels, n + 1, 3]: the
    ``points_3d`` of ``render_ground_truth`` and ``pnp_batch``.

    centre  "centroid" (the mean of the points) or "bbox" (the middle of the bounding box)
    start   as :func:`farthest_points`"""
    if centre not in ("centroid", "bbox"):
        raise RuntimeError("centre must be 'centroid' or 'bbox'")
    _, picked = farthest_points(table, n, start)
    e = extent(table)
    c = e["centroid"] if centre == "centroid" else (e["bbox_min"] + e["bbox_max"]) * 0.5
    return torch.cat([picked, c[:, None]], 1)
