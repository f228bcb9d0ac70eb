"""ctypes binding of libpvshade.so (include/pvshade.h): u8 RGB frames with Lambert shading from
vertex-coloured meshes and poses, with the maps of the same z-buffer, and smooth vertex normals.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVSHADE_LIB", os.path.join(HERE, "libpvshade.so"))

PV_LABEL_I64, PV_LABEL_U8, PV_LABEL_I32 = 0, 1, 2
PV_SHADE_SUBPIXEL_BITS = 8
PV_SHADE_MAX_SNAP = 1 << 29
PV_SHADE_MAX_DIM = 1 << 20
PV_SHADE_LIGHT_DOUBLES = 9

c_i32, c_i64, c_vp, c_f64, c_u8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_uint8


class ShadeMeshes(ctypes.Structure):
    _fields_ = [("verts", c_vp), ("vert_off", c_vp), ("faces", c_vp), ("face_off", c_vp), ("colors", c_vp),
                ("normals", c_vp), ("nmodels", c_i32), ("total_v", c_i32), ("total_f", c_i32),
                ("max_verts", c_i32), ("max_faces", c_i32), ("reserved_", c_i32)]


class ShadeBatch(ctypes.Structure):
    _fields_ = [("b", c_i32), ("H", c_i32), ("W", c_i32), ("ninst", c_i32), ("total_inst", c_i32),
                ("label_kind", c_i32), ("inst_off", c_vp), ("model_id", c_vp), ("label", c_vp), ("pose", c_vp),
                ("K", c_vp), ("K_stride", c_i64), ("znear", c_f64)]


class ShadeLights(ctypes.Structure):
    _fields_ = [("lights", c_vp), ("lights_stride", c_i64), ("background", c_vp), ("bg_strides", c_i64 * 4),
                ("bg_color", c_u8 * 3), ("pad_", c_u8 * 5)]


class ShadeOut(ctypes.Structure):
    _fields_ = [("image", c_vp), ("image_strides", c_i64 * 4), ("label", c_vp), ("inst", c_vp), ("depth", c_vp),
                ("face", c_vp), ("won", c_vp)]


# (name, restype, argtypes) -- one entry per function declared in include/pvshade.h
SIGNATURES = [
    ("pv_shade_normals", ctypes.c_int, [ctypes.POINTER(ShadeMeshes), c_vp, c_vp]),
    ("pv_shade_workspace_size", ctypes.c_size_t, [c_i32, c_i32, c_i32, c_i64, c_i32]),
    ("pv_shade_render", ctypes.c_int, [ctypes.POINTER(ShadeMeshes), ctypes.POINTER(ShadeBatch), ctypes.POINTER(ShadeLights),
                                       ctypes.POINTER(ShadeOut), c_vp, ctypes.c_size_t, c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVShadeError(RuntimeError):
    pass


check = checker(PVShadeError)
