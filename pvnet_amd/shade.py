"""Colour frames from vertex-coloured meshes, on the device: the picture that goes with the labels.

* :class:`ColorMeshTable` holds triangle meshes with a colour (and optionally a normal) per vertex;
  ``with_smooth_normals()`` computes area-weighted vertex normals on the device (``pv_shade_normals``).
* :func:`default_lights` and :func:`random_lights` make the small [b, 9] light table.
* :func:`render_color` turns (meshes, poses, cameras, lights) into u8 RGB frames with Lambert
  shading, and the label / instance / depth / face maps of the same z-buffer (``pv_shade_render``,
  include/pvshade.h).  The maps equal ``render.render_labels``' bit for bit.
* :func:`render_bank` renders one object per frame and projects its keypoints: the first three
  arguments of ``compose.compose_ground_truth``.

No specular term, no texture, no anti-aliasing (``compose.finish`` blurs).  Nothing is read back and
nothing synchronises.  No CPU fallback: without libpvshade.so or a ROCm device the calls raise.
"""
from __future__ import annotations

import copy
import ctypes

import numpy as np
import torch

from . import _shade_lib
from .ransac_voting_gpu import VotingWorkspace
from .render import MeshTable, _camera, _instances, _on, project_keypoints

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own

_LABEL_KIND = {torch.int64: _shade_lib.PV_LABEL_I64, torch.uint8: _shade_lib.PV_LABEL_U8,
               torch.int32: _shade_lib.PV_LABEL_I32}
ALL_OUTPUTS = ("image", "label", "inst", "depth", "face", "won")
_MAP_DTYPE = {"inst": torch.int32, "depth": torch.float32, "face": torch.int32}
HEADLIGHT = (0.0, 0.0, -1.0, 0.3, 0.3, 0.3, 0.7, 0.7, 0.7)   # from the camera; ambient 0.3, diffuse 0.7
_default = {}                                # device -> the shared headlight, made once (a capture cannot upload)


class ColorMeshTable(MeshTable):
    """Triangle meshes with a colour per vertex.

    models  list of ``(vertices [pv, 3], faces [pf, 3], colors [pv, 3][, normals [pv, 3]])``: colours are
            integers 0..255 (r, g, b); normals, in the model frame, need not be unit length, and a
            zero normal means "use the face normal".  With normals on no model the table shades flat;
            with normals on some, the other models' are zero.
    device  where the table lives (default: the current ROCm device)

    MeshTable's tensors, colors u8 [total_v, 3] and normals f64 [total_v, 3] or None."""

    def __init__(self, models, device=None):
        super().__init__([(m[0], m[1]) for m in models], device)
        cs, ns, have = [], [], False
        for m, nv in zip(models, self.vert_counts):
            if len(m) not in (3, 4):
                raise ValueError("a model is (vertices, faces, colors) or (vertices, faces, colors, normals)")
            c = np.asarray(m[2])
            if c.size and not np.issubdtype(c.dtype, np.integer):
                raise ValueError("colors must be integers")
            c = c.astype(np.int64).reshape(-1, 3)
            if c.shape[0] != nv or (c.size and (c.min() < 0 or c.max() > 255)):
                raise ValueError("colors must be [vertices, 3] with values in 0..255")
            cs.append(c.astype(np.uint8))
            if len(m) == 4 and m[3] is not None:
                n = np.asarray(m[3], dtype=np.float64).reshape(-1, 3)
                if n.shape[0] != nv:
                    raise ValueError("normals must be [vertices, 3]")
                have = True
            else:
                n = np.zeros((nv, 3), np.float64)
            ns.append(n)
        self.colors = torch.from_numpy(np.ascontiguousarray(np.concatenate(cs))).to(self.device)
        self.normals = torch.from_numpy(np.ascontiguousarray(np.concatenate(ns))).to(self.device) if have else None

    def _meshes(self):
        return _shade_lib.ShadeMeshes(self.verts.data_ptr(), self.vert_off.data_ptr(), self.faces.data_ptr(),
                                      self.face_off.data_ptr(), self.colors.data_ptr(),
                                      None if self.normals is None else self.normals.data_ptr(), self.nmodels,
                                      self.total_v, self.total_f, self.max_verts, self.max_faces, 0)

    def with_smooth_normals(self) -> "ColorMeshTable":
        """A table sharing this one's tensors whose normals are the area-weighted sums of the faces
        around each vertex, normalised (``pv_shade_normals``); a vertex no face names gets zero."""
        if self.device.type != "cuda":
            raise RuntimeError("with_smooth_normals runs on the ROCm device (no CPU path)")
        t = copy.copy(self)
        t.normals = torch.empty((self.total_v, 3), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _shade_lib.check(_shade_lib.load().pv_shade_normals(ctypes.byref(self._meshes()), t.normals.data_ptr(),
                                                                torch.cuda.current_stream(self.device).cuda_stream),
                             "pv_shade_normals")
        return t


def default_lights(b: int = 1, device=None) -> torch.Tensor:
    """f64 [b, 9] on `device` (default: the host): a headlight, direction (0, 0, -1) towards the
    camera, ambient 0.3 and diffuse 0.7 on every channel."""
    return torch.tensor([HEADLIGHT] * int(b), dtype=torch.float64).reshape(int(b), 9).to(device or "cpu")


def random_lights(b: int, seed: int, ambient=(0.2, 0.5), diffuse=(0.4, 0.8), device=None) -> torch.Tensor:
    """f64 [b, 9] on `device` (default: the host), drawn with numpy's default_rng(seed) on the host:
    the direction uniform on the camera-side hemisphere (unit length, z <= 0: the camera looks along
    +z, so a surface it sees faces -z), the ambient and the diffuse level each one uniform draw from
    its range, the same on r, g and b."""
    b = int(b)
    for name, (lo, hi) in (("ambient", ambient), ("diffuse", diffuse)):
        if not (0.0 <= float(lo) <= float(hi)) or not np.isfinite(hi):
            raise RuntimeError(f"{name} must be a finite range 0 <= lo <= hi")
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(b, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    d[:, 2] = -np.abs(d[:, 2])
    a = rng.uniform(ambient[0], ambient[1], size=(b, 1))
    k = rng.uniform(diffuse[0], diffuse[1], size=(b, 1))
    out = np.concatenate([d, np.repeat(a, 3, 1), np.repeat(k, 3, 1)], 1)
    return torch.from_numpy(np.ascontiguousarray(out)).to(device or "cpu")


def _lights(lights, b, dev):
    if lights is None:
        if dev not in _default:
            _default[dev] = default_lights(1, dev)
        return _default[dev], 0
    lt = _on(lights, dev, torch.float64)
    if tuple(lt.shape) in ((9,), (1, 9)):
        return lt, 0
    if tuple(lt.shape) == (b, 9):
        return lt, 9
    raise RuntimeError("lights must be [9], [1, 9] (shared) or [b, 9]")


def _background(background, b, H, W, dev, desc):
    if background is None:
        return None
    if isinstance(background, torch.Tensor):
        bg = background
        if bg.dtype != torch.uint8 or bg.dim() not in (3, 4) or tuple(bg.shape[-3:]) != (H, W, 3) or \
                (bg.dim() == 4 and bg.shape[0] not in (1, b)):
            raise RuntimeError("background must be a uint8 [H, W, 3], [1, H, W, 3] or [b, H, W, 3] tensor, or three integers")
        if bg.device != dev:
            raise RuntimeError("background must be on the poses' device")
        if bg.dim() == 3:
            bg = bg[None]
        desc.background = bg.data_ptr()
        for i in range(4):
            desc.bg_strides[i] = bg.stride(i) if (i or bg.shape[0] == b) else 0
        return bg
    try:
        rgb = tuple(background)
        good = len(rgb) == 3 and all(v == int(v) and 0 <= v <= 255 for v in rgb)
    except TypeError:
        good = False
    if not good:
        raise RuntimeError("background must be a uint8 [H, W, 3], [1, H, W, 3] or [b, H, W, 3] tensor, or three integers")
    for i in range(3):
        desc.bg_color[i] = int(rgb[i])
    return None


def render_color(table: ColorMeshTable, poses, model_id, labels, K, H: int, W: int, lights=None, background=None,
                 znear: float = 1e-3, want=("image", "label"), out: dict | None = None, label_dtype=torch.uint8) -> dict:
    """Render a batch of colour frames on the device.

    table       :class:`ColorMeshTable`; its normals (if any) shade smooth, else each face is flat
    poses, model_id, labels, K, znear   as ``render.render_labels`` takes them, both instance forms
    lights      f64 [9] or [1, 9] (shared) or [b, 9]: direction towards the light in the camera frame,
                ambient rgb, diffuse rgb; None = :func:`default_lights`
    background  None (black), three integers 0..255, or a uint8 [H, W, 3] / [1, H, W, 3] (shared) /
                [b, H, W, 3] device tensor of any strides
    want        any of "image", "label", "inst", "depth", "face", "won" (at least one map)
    out         optional dict of tensors to write into: image uint8 [b, H, W, 3] of any strides (a
                [b, 3, H, W] tensor permuted is fine), the maps contiguous [b, H, W] (label: uint8 /
                int32 / int64, inst and face: int32, depth: float32), won int32 [total]

    Returns a dict of those wanted: label 0 / inst -1 / depth +inf / face -1 on the background, face
    the winning triangle's index within its model, won the pixels each instance owns.  The semantics
    are include/pvshade.h's."""
    if not isinstance(table, ColorMeshTable):
        raise RuntimeError("table must be a ColorMeshTable")
    pose, inst_off, b, per, n, mid, lab = _instances(table, poses, model_id, labels)
    dev = pose.device
    H, W = int(H), int(W)
    if not (1 <= H <= _shade_lib.PV_SHADE_MAX_DIM and 1 <= W <= _shade_lib.PV_SHADE_MAX_DIM):
        raise RuntimeError("H and W must be in 1..2^20")
    if not float(znear) > 0.0:
        raise RuntimeError("znear must be positive")
    want = tuple(want)
    if not want or any(w not in ALL_OUTPUTS for w in want) or want == ("won",):
        raise RuntimeError(f"want must name at least one map of {ALL_OUTPUTS}")
    if label_dtype not in _LABEL_KIND:
        raise RuntimeError("label_dtype must be uint8, int32 or int64")
    if n * table.max_faces >= 2 ** 32:
        raise RuntimeError("instances times the largest model's faces must stay below 2^32")
    Kt, ks = _camera(K, b, dev)
    lt, ls = _lights(lights, b, dev)
    L = _shade_lib.ShadeLights()
    L.lights, L.lights_stride = lt.data_ptr(), ls
    bg = _background(background, b, H, W, dev, L)          # kept alive until the call is enqueued
    res = {}
    for w in want:
        shape = (b, H, W, 3) if w == "image" else (n,) if w == "won" else (b, H, W)
        dt = torch.uint8 if w == "image" else torch.int32 if w == "won" else label_dtype if w == "label" else _MAP_DTYPE[w]
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=dev)
        elif not isinstance(t, torch.Tensor) or t.device != dev or tuple(t.shape) != shape or \
                (w != "image" and not t.is_contiguous()) or (t.dtype not in _LABEL_KIND if w == "label" else t.dtype != dt):
            raise RuntimeError(f"out[{w!r}] must be a {list(shape)} tensor of the output's dtype on the poses' device"
                               " (contiguous, but for the image)")
        res[w] = t
    if b == 0:
        return res

    def ptr(t):
        return None if t is None else t.data_ptr()

    lib = _shade_lib.load()
    need = int(lib.pv_shade_workspace_size(b, H, W, n * table.max_verts, n))
    ws = _ws.get(dev, need)
    m = table._meshes()
    label_t = res.get("label")
    bt = _shade_lib.ShadeBatch(b, H, W, per, n, _LABEL_KIND[label_t.dtype if label_t is not None else label_dtype],
                               ptr(inst_off), mid.data_ptr(), lab.data_ptr(), pose.data_ptr(), Kt.data_ptr(), ks, float(znear))
    ot = _shade_lib.ShadeOut()
    img = res.get("image")
    ot.image = ptr(img)
    if img is not None:
        for i in range(4):
            ot.image_strides[i] = img.stride(i)
    ot.label, ot.inst, ot.depth, ot.face, ot.won = ptr(label_t), ptr(res.get("inst")), ptr(res.get("depth")), \
        ptr(res.get("face")), ptr(res.get("won"))
    with torch.cuda.device(dev):
        _shade_lib.check(lib.pv_shade_render(ctypes.byref(m), ctypes.byref(bt), ctypes.byref(L), ctypes.byref(ot),
                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                         "pv_shade_render")
    del bg
    return res


def render_bank(table: ColorMeshTable, points_3d, poses: torch.Tensor, model_id, K, H: int, W: int, lights=None,
                background=None, znear: float = 1e-3, label_dtype=torch.uint8):
    """A bank of single-object frames for ``compose.compose_ground_truth``.

    points_3d  [nmodels, vn, 3]: each model's 3-D keypoints
    poses      [N, 3, 4] device tensor, one object per frame; model_id int [N]; the label is model_id + 1
    K          [3, 3] shared or [N, 3, 3]

    Returns ``(bank_image uint8 [N, H, W, 3], bank_label [N, H, W], bank_keypoints f64 [N, vn, 2])``."""
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise RuntimeError("poses must be a [N, 3, 4] device tensor")
    N = int(poses.shape[0])
    pose, _, _, _, _, mid, lab = _instances(table, poses[:, None], torch.as_tensor(model_id).reshape(N, 1), None)
    dev = pose.device
    p3 = _on(points_3d, dev, torch.float64)
    if p3.dim() != 3 or p3.shape[2] != 3 or p3.shape[0] != table.nmodels:
        raise RuntimeError("points_3d must be [nmodels, vn, 3]")
    Kt, _ = _camera(K, N, dev)
    r = render_color(table, poses[:, None], mid.reshape(N, 1), lab.reshape(N, 1), Kt, H, W, lights, background, znear,
                     want=("image", "label"), label_dtype=label_dtype)
    cls = mid.clamp(0, table.nmodels - 1).to(torch.int64)
    kp = project_keypoints(p3[cls], pose, Kt)
    return r["image"], r["label"], kp
