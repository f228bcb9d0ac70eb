"""ctypes binding of libpvcompose.so (include/pvcompose.h): multi-object frames pasted from a bank of
single-object frames, the draw of their placement, erasers, blur and noise, and the blur + noise finish.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVCOMPOSE_LIB", os.path.join(HERE, "libpvcompose.so"))

PV_CMP_LABEL_I64, PV_CMP_LABEL_U8, PV_CMP_LABEL_I32 = 0, 1, 2
PV_CMP_PIXELS = 8
PV_CMP_THREADS = 256
PV_CMP_TILE = 32
PV_CMP_HALO = 4
PV_CMP_MAX_SLOTS = 16
PV_CMP_MAX_ERASE = 8
PV_CMP_MAX_DIM = 2 ** 15
PV_CMP_MAX_CLASSES = 1024
PV_CMP_DRAW0 = 64

c_i32, c_i64, c_vp, c_f32, c_f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double


class CmpDesc(ctypes.Structure):
    _fields_ = [("image", c_vp), ("label", c_vp), ("pick", c_vp), ("shift", c_vp), ("erase", c_vp), ("background", c_vp),
                ("out_image", c_vp), ("out_label", c_vp), ("out_instance", c_vp), ("visible", c_vp),
                ("image_strides", c_i64 * 4), ("label_strides", c_i64 * 3), ("background_strides", c_i64 * 4),
                ("out_image_strides", c_i64 * 4), ("out_label_strides", c_i64 * 3), ("out_instance_strides", c_i64 * 3),
                ("label_kind", c_i32), ("N", c_i32), ("H", c_i32), ("W", c_i32), ("b", c_i32), ("Ho", c_i32), ("Wo", c_i32),
                ("S", c_i32), ("E", c_i32), ("ncls", c_i32), ("fill", c_i32 * 3), ("pad_", c_i32)]


class CmpRanges(ctypes.Structure):
    _fields_ = [("margin", c_f64), ("erase_frac", c_f64 * 2), ("p_blur", c_f64), ("noise", c_f64 * 2),
                ("b", c_i32), ("N", c_i32), ("H", c_i32), ("W", c_i32), ("Ho", c_i32), ("Wo", c_i32),
                ("S", c_i32), ("E", c_i32), ("ncls", c_i32), ("pad_", c_i32)]


class CmpFinish(ctypes.Structure):
    _fields_ = [("image", c_vp), ("out", c_vp), ("ksel", c_vp), ("amp", c_vp), ("state", c_vp),
                ("image_strides", c_i64 * 4), ("out_strides", c_i64 * 4), ("w", (c_f32 * 5) * 5),
                ("b", c_i32), ("H", c_i32), ("W", c_i32), ("pad_", c_i32)]


# (name, restype, argtypes) -- one entry per function declared in include/pvcompose.h
SIGNATURES = [
    ("pv_compose_apply", ctypes.c_int, [ctypes.POINTER(CmpDesc), c_vp]),
    ("pv_compose_params", ctypes.c_int, [ctypes.POINTER(CmpRanges), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("pv_compose_finish", ctypes.c_int, [ctypes.POINTER(CmpFinish), c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVComposeError(RuntimeError):
    pass


check = checker(PVComposeError)
