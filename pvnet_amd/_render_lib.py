"""ctypes binding of libpvrender.so (include/pvrender.h): label / instance / depth maps from
meshes and poses, and the unit vector field from a label map and keypoints.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVRENDER_LIB", os.path.join(HERE, "libpvrender.so"))

PV_LABEL_I64, PV_LABEL_U8, PV_LABEL_I32 = 0, 1, 2
PV_FIELD_F32, PV_FIELD_F16 = 0, 1
PV_KP_F64, PV_KP_F32 = 0, 1
PV_RENDER_SUBPIXEL_BITS = 8
PV_RENDER_MAX_SNAP = 1 << 29
PV_RENDER_MAX_DIM = 1 << 20
PV_RENDER_SNAP_INVALID = -(1 << 31)

c_i32, c_i64, c_vp, c_f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double


class RenderMeshes(ctypes.Structure):
    _fields_ = [("verts", c_vp), ("vert_off", c_vp), ("faces", c_vp), ("face_off", c_vp),
                ("nmodels", c_i32), ("total_v", c_i32), ("total_f", c_i32),
                ("max_verts", c_i32), ("max_faces", c_i32), ("reserved_", c_i32)]


class RenderBatch(ctypes.Structure):
    _fields_ = [("b", c_i32), ("H", c_i32), ("W", c_i32), ("ninst", c_i32), ("total_inst", c_i32),
                ("label_kind", c_i32), ("inst_off", c_vp), ("model_id", c_vp), ("label", c_vp), ("pose", c_vp),
                ("K", c_vp), ("K_stride", c_i64), ("znear", c_f64)]


class RenderOut(ctypes.Structure):
    _fields_ = [("label", c_vp), ("inst", c_vp), ("depth", c_vp), ("snap_xy", c_vp), ("snap_z", c_vp), ("won", c_vp)]


class FieldDesc(ctypes.Structure):
    _fields_ = [("label", c_vp), ("keypoints", c_vp), ("vertex", c_vp), ("label_strides", c_i64 * 3),
                ("vertex_strides", c_i64 * 5), ("label_kind", c_i32), ("kp_kind", c_i32), ("vertex_kind", c_i32),
                ("b", c_i32), ("H", c_i32), ("W", c_i32), ("ncls", c_i32), ("vn", c_i32)]


# (name, restype, argtypes) -- one entry per function declared in include/pvrender.h
SIGNATURES = [
    ("pv_render_workspace_size", ctypes.c_size_t, [c_i32, c_i32, c_i32, c_i64, c_i32]),
    ("pv_render_labels", ctypes.c_int, [ctypes.POINTER(RenderMeshes), ctypes.POINTER(RenderBatch),
                                        ctypes.POINTER(RenderOut), c_vp, ctypes.c_size_t, c_vp]),
    ("pv_vertex_field", ctypes.c_int, [ctypes.POINTER(FieldDesc), c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVRenderError(RuntimeError):
    pass


check = checker(PVRenderError)
