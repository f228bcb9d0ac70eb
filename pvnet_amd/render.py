"""Ground truth from a pose, on the device: the direction the rest of the package lacks.

* :class:`MeshTable` holds triangle meshes (vertices and faces, concatenated) on the device.
* :func:`render_labels` turns (meshes, poses, cameras) into a label map, an instance map and a
  depth map through a z-buffer (``pv_render_labels``, include/pvrender.h) -- the replacement for
  the reference's ``extend_utils/src/mesh_rasterization.cpp``, batched and with a depth test.
* :func:`vertex_field` turns (label map, projected keypoints) into the unit vector field
  (``pv_vertex_field``; the reference's ``compute_vertex``).
* :func:`render_ground_truth` chains the two: its result goes straight into
  ``ransac_voting_layer_v3_multi`` / ``estimate_voting_distribution_with_mean_multi``.
* :func:`mask_iou` compares two label maps per class.

Nothing is read back and nothing synchronises.  No CPU fallback: without libpvrender.so or a
ROCm device the calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _render_lib
from .ransac_voting_gpu import VotingWorkspace

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own

_LABEL_KIND = {torch.int64: _render_lib.PV_LABEL_I64, torch.uint8: _render_lib.PV_LABEL_U8,
               torch.int32: _render_lib.PV_LABEL_I32}
_FIELD_KIND = {torch.float32: _render_lib.PV_FIELD_F32, torch.float16: _render_lib.PV_FIELD_F16}
_KP_KIND = {torch.float64: _render_lib.PV_KP_F64, torch.float32: _render_lib.PV_KP_F32}
ALL_MAPS = ("label", "inst", "depth")
_MAP_DTYPE = {"inst": torch.int32, "depth": torch.float32}


class MeshTable:
    """The triangle meshes instances are rendered from.

    models  list of ``(vertices [pv, 3], faces [pf, 3])``; an instance's ``model_id`` indexes it,
            and a face's indices are local to its model
    device  where the table lives (default: the current ROCm device)

    verts f32 [total_v, 3] and faces i32 [total_f, 3] (all models, concatenated), vert_off and
    face_off i32 [nmodels + 1]."""

    def __init__(self, models, device=None):
        if len(models) < 1:
            raise ValueError("MeshTable needs at least one model")
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("MeshTable lives on the ROCm device (no CPU path)")
            device = torch.device("cuda", torch.cuda.current_device())
        vs, fs = [], []
        for vertices, faces in models:
            vs.append(np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3)))
            f = np.asarray(faces)
            if f.size and not np.issubdtype(f.dtype, np.integer):
                raise ValueError("faces must be integers")
            fs.append(np.ascontiguousarray(f.astype(np.int64).reshape(-1, 3)))
        voff = np.zeros(len(models) + 1, np.int64)
        foff = np.zeros(len(models) + 1, np.int64)
        np.cumsum([v.shape[0] for v in vs], out=voff[1:])
        np.cumsum([f.shape[0] for f in fs], out=foff[1:])
        if max(voff[-1], foff[-1]) > np.iinfo(np.int32).max:
            raise ValueError("the models have more than 2^31 - 1 vertices or faces in all")
        for f in fs:
            if f.size and (f.min() < np.iinfo(np.int32).min or f.max() > np.iinfo(np.int32).max):
                raise ValueError("a face index does not fit int32")
        self.device = torch.device(device)
        self.nmodels = len(models)
        self.total_v, self.total_f = int(voff[-1]), int(foff[-1])
        self.vert_counts = tuple(int(v.shape[0]) for v in vs)
        self.face_counts = tuple(int(f.shape[0]) for f in fs)
        self.max_verts, self.max_faces = max(self.vert_counts), max(self.face_counts)
        self.verts = torch.from_numpy(np.concatenate(vs) if self.total_v else np.zeros((0, 3), np.float32)).to(device)
        self.faces = torch.from_numpy((np.concatenate(fs) if self.total_f else np.zeros((0, 3), np.int64))
                                      .astype(np.int32)).to(device)
        self.vert_off = torch.from_numpy(voff.astype(np.int32)).to(device)
        self.face_off = torch.from_numpy(foff.astype(np.int32)).to(device)


def _on(x, dev, dtype):
    """x as a contiguous tensor of dtype on dev (used in place when it already is one)."""
    return torch.as_tensor(x).to(device=dev, dtype=dtype).contiguous()


def _instances(table, poses, model_id, labels):
    """-> (pose f64 [n, 3, 4], inst_off or None, b, per-image count, n, model_id i32 [n], labels i32 [n])."""
    if not isinstance(table, MeshTable):
        raise RuntimeError("table must be a MeshTable")
    inst_off = None
    if isinstance(poses, (tuple, list)):
        if len(poses) != 2:
            raise RuntimeError("poses must be [b, n, 3, 4] or ([total, 3, 4], inst_off)")
        poses, inst_off = poses
    if not isinstance(poses, torch.Tensor) or poses.device.type != "cuda":
        raise RuntimeError("poses must be a device tensor (no CPU path)")
    dev = poses.device
    if table.device != dev:
        raise RuntimeError("poses and the mesh table must be on the same device")
    if inst_off is None:
        if poses.dim() != 4 or tuple(poses.shape[2:]) != (3, 4):
            raise RuntimeError("poses must be [b, n, 3, 4] or ([total, 3, 4], inst_off)")
        b, per = int(poses.shape[0]), int(poses.shape[1])
        n = b * per
        lead = (b, per)
    else:
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
            raise RuntimeError("poses must be [b, n, 3, 4] or ([total, 3, 4], inst_off)")
        inst_off = _on(inst_off, dev, torch.int32)
        if inst_off.dim() != 1 or inst_off.shape[0] < 1:
            raise RuntimeError("inst_off must be [b + 1]")
        b, per, n = int(inst_off.shape[0]) - 1, 0, int(poses.shape[0])
        lead = (n,)

    def per_instance(x, name):
        if x is None:
            raise RuntimeError(f"{name} must be given")
        if not isinstance(x, torch.Tensor):
            x = np.asarray(x)
            if name == "labels" and x.size and (x.min() < 1 or x.max() > 255):
                raise RuntimeError("labels must be in 1..255")
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dim() > len(lead) or tuple(x.shape) != lead[len(lead) - x.dim():]:
            raise RuntimeError(f"{name} must be {list(lead)} (or its trailing dimensions)")
        return x.to(device=dev, dtype=torch.int32).expand(lead).reshape(n).contiguous()

    mid = per_instance(model_id, "model_id")
    lab = mid + 1 if labels is None else per_instance(labels, "labels")
    return poses.to(torch.float64).reshape(n, 3, 4).contiguous(), inst_off, b, per, n, mid, lab


def _camera(K, b, dev):
    Kt = _on(K, dev, torch.float64)
    if tuple(Kt.shape) == (3, 3):
        return Kt, 0
    if tuple(Kt.shape) == (b, 3, 3):
        return Kt, 9
    raise RuntimeError("K must be [3, 3] or [b, 3, 3]")


def render_labels(table: MeshTable, poses, model_id, labels, K, H: int, W: int, znear: float = 1e-3,
                  want=ALL_MAPS, out: dict | None = None, label_dtype=torch.uint8, diag: dict | None = None) -> dict:
    """Rasterise a batch of frames on the device.

    table     :class:`MeshTable`
    poses     [b, n, 3, 4] device tensor (n instances in every frame), or
              ``([total, 3, 4], inst_off)`` with inst_off int [b + 1]: frame i owns instances
              [inst_off[i], inst_off[i + 1])
    model_id  int per instance: [b, n] (or [n], the same in every frame), [total] in the second form
    labels    the value each instance writes into the label map, 1..255, shaped as model_id;
              None = model_id + 1
    K         [3, 3] shared or [b, 3, 3] camera matrix
    znear     a triangle with a vertex nearer than this is dropped whole (no clipping)
    want      any of "label", "inst", "depth"
    out       optional dict of contiguous [b, H, W] tensors to write into (label: uint8 / int32 /
              int64, inst: int32, depth: float32)
    diag      optional dict, filled with ``snap_xy`` i32 [total, max_verts, 2], ``snap_z`` f64
              [total, max_verts] (the snapped vertices; rows of skipped instances and rows past a
              model's vertex count hold what the allocator left there) and ``won`` i32 [total] (pixels
              each instance owns)

    Returns {"label", "inst", "depth"} (those wanted): label 0 / inst -1 / depth +inf on the
    background.  An instance with a model_id outside the table, a non-finite pose or a label
    outside 1..255 is skipped.  The semantics are include/pvrender.h's."""
    pose, inst_off, b, per, n, mid, lab = _instances(table, poses, model_id, labels)
    dev = pose.device
    H, W = int(H), int(W)
    if not (1 <= H <= _render_lib.PV_RENDER_MAX_DIM and 1 <= W <= _render_lib.PV_RENDER_MAX_DIM):
        raise RuntimeError("H and W must be in 1..2^20")
    if not float(znear) > 0.0:
        raise RuntimeError("znear must be positive")
    want = tuple(want)
    if not want or any(w not in ALL_MAPS for w in want):
        raise RuntimeError(f"want must name at least one of {ALL_MAPS}")
    if label_dtype not in _LABEL_KIND:
        raise RuntimeError("label_dtype must be uint8, int32 or int64")
    Kt, ks = _camera(K, b, dev)
    res = {}
    for w in want:
        dt = label_dtype if w == "label" else _MAP_DTYPE[w]
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty((b, H, W), dtype=dt, device=dev)
        elif not isinstance(t, torch.Tensor) or t.device != dev or tuple(t.shape) != (b, H, W) or \
                not t.is_contiguous() or (t.dtype not in _LABEL_KIND if w == "label" else t.dtype != dt):
            raise RuntimeError(f"out[{w!r}] must be a contiguous [b, H, W] tensor of the map's dtype on the poses' device")
        res[w] = t
    d = {}
    if diag is not None:
        d["snap_xy"] = torch.empty((n, table.max_verts, 2), dtype=torch.int32, device=dev)
        d["snap_z"] = torch.empty((n, table.max_verts), dtype=torch.float64, device=dev)
        d["won"] = torch.empty((n,), dtype=torch.int32, device=dev)
    if b == 0:
        if diag is not None:
            diag.update(d)
        return res

    def ptr(t):
        return None if t is None else t.data_ptr()

    L = _render_lib.load()
    need = int(L.pv_render_workspace_size(b, H, W, n * table.max_verts, n))
    ws = _ws.get(dev, need)
    m = _render_lib.RenderMeshes(table.verts.data_ptr(), table.vert_off.data_ptr(), table.faces.data_ptr(),
                                 table.face_off.data_ptr(), table.nmodels, table.total_v, table.total_f,
                                 table.max_verts, table.max_faces, 0)
    lt = res.get("label")
    bt = _render_lib.RenderBatch(b, H, W, per, n, _LABEL_KIND[lt.dtype if lt is not None else label_dtype],
                                 ptr(inst_off), mid.data_ptr(), lab.data_ptr(), pose.data_ptr(), Kt.data_ptr(), ks,
                                 float(znear))
    ot = _render_lib.RenderOut(ptr(lt), ptr(res.get("inst")), ptr(res.get("depth")), ptr(d.get("snap_xy")),
                               ptr(d.get("snap_z")), ptr(d.get("won")))
    with torch.cuda.device(dev):
        _render_lib.check(L.pv_render_labels(ctypes.byref(m), ctypes.byref(bt), ctypes.byref(ot), ws.data_ptr(),
                                             ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                          "pv_render_labels")
    if diag is not None:
        diag.update(d)
    return res


def vertex_field(label: torch.Tensor, keypoints_2d: torch.Tensor, class_num: int, dtype=torch.float32,
                 layout: str = "bhwk2", out: torch.Tensor | None = None) -> torch.Tensor:
    """The ground-truth unit vector field of a multi-object frame (``compute_vertex`` per class).

    label         [b, H, W] device tensor, uint8 / int32 / int64, any strides; class c = label c + 1
    keypoints_2d  [b, class_num, vn, 2] device tensor (float64 or float32 used as they are,
                  anything else as float64)
    dtype         float32 or float16 (float16 is the float32 value rounded, as ``.half()`` gives)
    layout        "bhwk2": a contiguous [b, H, W, class_num*vn, 2], what the voting layers take;
                  "network": [b, 2*class_num*vn, H, W], what the network emits
    out           optional tensor to write into, of the layout's shape and any strides

    Every element is written: zeros on the background, on other classes' channels and for labels
    above class_num."""
    if not (isinstance(label, torch.Tensor) and isinstance(keypoints_2d, torch.Tensor)):
        raise RuntimeError("label and keypoints_2d must be tensors")
    class_num = int(class_num)
    if class_num < 1:
        raise RuntimeError("class_num must be at least 1")
    if layout not in ("bhwk2", "network"):
        raise RuntimeError("layout must be 'bhwk2' or 'network'")
    if label.dim() != 3 or label.dtype not in _LABEL_KIND:
        raise RuntimeError("label must be a uint8 / int32 / int64 [b, H, W] tensor")
    b, H, W = (int(s) for s in label.shape)
    if keypoints_2d.dim() != 4 or tuple(keypoints_2d.shape[:2]) != (b, class_num) or keypoints_2d.shape[3] != 2 \
            or keypoints_2d.shape[2] < 1:
        raise RuntimeError(f"keypoints_2d must be [b, class_num, vn, 2] = [{b}, {class_num}, vn, 2]")
    vn = int(keypoints_2d.shape[2])
    C = class_num * vn
    if dtype not in _FIELD_KIND:
        raise RuntimeError("dtype must be float32 or float16")
    if label.device.type != "cuda":
        raise RuntimeError("label must be a device tensor (no CPU path)")
    dev = label.device
    if keypoints_2d.device != dev:
        raise RuntimeError("label and keypoints_2d must be on the same device")
    if H < 1 or W < 1:
        raise RuntimeError("label must have at least one pixel per image")
    kp = keypoints_2d if keypoints_2d.dtype in _KP_KIND else keypoints_2d.to(torch.float64)
    kp = kp.contiguous()
    shape = (b, H, W, C, 2) if layout == "bhwk2" else (b, 2 * C, H, W)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev or tuple(out.shape) != shape or out.dtype != dtype:
        raise RuntimeError(f"out must be a {dtype} tensor of shape {list(shape)} on the label's device")
    view = out if layout == "bhwk2" else out.permute(0, 2, 3, 1).unflatten(3, (C, 2))
    if b == 0:
        return out
    d = _render_lib.FieldDesc()
    d.label, d.keypoints, d.vertex = label.data_ptr(), kp.data_ptr(), out.data_ptr()
    for i in range(3):
        d.label_strides[i] = label.stride(i)
    for i in range(5):
        d.vertex_strides[i] = view.stride(i)
    d.label_kind, d.kp_kind, d.vertex_kind = _LABEL_KIND[label.dtype], _KP_KIND[kp.dtype], _FIELD_KIND[dtype]
    d.b, d.H, d.W, d.ncls, d.vn = b, H, W, class_num, vn
    with torch.cuda.device(dev):
        _render_lib.check(_render_lib.load().pv_vertex_field(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                          "pv_vertex_field")
    return out


def project_keypoints(points_3d: torch.Tensor, poses: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """points_3d f64 [..., vn, 3], poses f64 [..., 3, 4], K f64 [3, 3] or [..., 3, 3] -> f64 [..., vn, 2]:
    u = (fx X + s Y) / Z + cx, v = fy Y / Z + cy in the camera frame, in float64 on the tensors' device."""
    X = points_3d @ poses[..., :3].transpose(-1, -2) + poses[..., None, :, 3]
    u = (K[..., None, 0, 0] * X[..., 0] + K[..., None, 0, 1] * X[..., 1]) / X[..., 2] + K[..., None, 0, 2]
    v = (K[..., None, 1, 1] * X[..., 1]) / X[..., 2] + K[..., None, 1, 2]
    return torch.stack([u, v], -1)


def render_ground_truth(table: MeshTable, points_3d, poses: torch.Tensor, model_id, K, H: int, W: int,
                        znear: float = 1e-3, dtype=torch.float32, layout: str = "bhwk2", label_dtype=torch.uint8):
    """What the network should have said about a frame: label map, vector field and keypoints.

    points_3d  [ncls, vn, 3]: each class's 3-D keypoints; class = model_id, label = class + 1
    poses      [b, n, 3, 4] device tensor; model_id int [b, n] or [n] with values in [0, ncls).
               A class appears at most once per frame; a class that is absent has keypoints 0
               and no pixel.

    Returns ``(label [b, H, W], vertex, keypoints_2d f64 [b, ncls, vn, 2])`` with vertex as
    :func:`vertex_field` lays it out: ``ransac_voting_layer_v3_multi(label, vertex, ncls, ...)``
    takes them as they are."""
    if not isinstance(poses, torch.Tensor) or poses.dim() != 4:
        raise RuntimeError("poses must be a [b, n, 3, 4] device tensor")
    pose, _, b, per, n, mid, lab = _instances(table, poses, model_id, None)
    dev = pose.device
    p3 = _on(points_3d, dev, torch.float64)
    if p3.dim() != 3 or p3.shape[2] != 3 or p3.shape[0] != table.nmodels:
        raise RuntimeError("points_3d must be [nmodels, vn, 3]")
    ncls, vn = int(p3.shape[0]), int(p3.shape[1])
    Kt, ks = _camera(K, b, dev)
    label = render_labels(table, poses, mid.reshape(b, per), lab.reshape(b, per), Kt, H, W, znear, want=("label",),
                          label_dtype=label_dtype)["label"]
    valid = (mid >= 0) & (mid < ncls)
    cls = mid.clamp(0, ncls - 1).to(torch.int64)
    Kb = Kt if ks == 0 else Kt[:, None].expand(b, per, 3, 3).reshape(n, 3, 3)
    kp_inst = project_keypoints(p3[cls], pose, Kb)                         # [n, vn, 2]
    img = torch.arange(b, device=dev).repeat_interleave(per)
    kp = torch.zeros((b, ncls, vn, 2), dtype=torch.float64, device=dev)
    kp.index_put_((img, cls), torch.where(valid[:, None, None], kp_inst, kp[img, cls]))
    vertex = vertex_field(label, kp, ncls, dtype=dtype, layout=layout)
    return label, vertex, kp


def mask_iou(label_a: torch.Tensor, label_b: torch.Tensor, class_num: int) -> torch.Tensor:
    """Intersection over union of each class's mask in two label maps [b, H, W] -> f64
    [b, class_num] on their device (NaN where neither map has the class)."""
    if not (isinstance(label_a, torch.Tensor) and isinstance(label_b, torch.Tensor)) or label_a.dim() != 3 \
            or label_a.shape != label_b.shape:
        raise RuntimeError("label_a and label_b must be [b, H, W] tensors of one shape")
    if label_a.device != label_b.device:
        raise RuntimeError("label_a and label_b must be on the same device")
    cls = torch.arange(1, int(class_num) + 1, device=label_a.device)[None, :, None, None]
    a, bb = label_a[:, None] == cls, label_b[:, None] == cls
    inter = (a & bb).sum((2, 3)).to(torch.float64)
    union = (a | bb).sum((2, 3)).to(torch.float64)
    return inter / union
