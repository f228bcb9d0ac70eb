"""ctypes binding of libpvaugment.so (include/pvaugment.h): the foreground statistics of a label map,
the draw of one affine map and one colour jitter per image, and the warp + background + photometric
chain + normalisation of a u8 batch.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVAUGMENT_LIB", os.path.join(HERE, "libpvaugment.so"))

PV_AUG_LABEL_I64, PV_AUG_LABEL_U8, PV_AUG_LABEL_I32 = 0, 1, 2
PV_AUG_F32, PV_AUG_F16 = 0, 1
PV_AUG_BRIGHTNESS, PV_AUG_CONTRAST, PV_AUG_SATURATION, PV_AUG_HUE = 1, 2, 4, 8
PV_AUG_ALL = 15
PV_AUG_PIXELS = 8
PV_AUG_THREADS = 256
PV_AUG_MAX_DIM = 2 ** 20
PV_AUG_MAX_CLASSES = 1024
PV_AUG_DRAWS = 8

c_i32, c_i64, c_vp, c_f32, c_f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double


class AugLabel(ctypes.Structure):
    _fields_ = [("label", c_vp), ("label_strides", c_i64 * 3), ("label_kind", c_i32),
                ("b", c_i32), ("H", c_i32), ("W", c_i32)]


class AugRanges(ctypes.Structure):
    _fields_ = [("rot_deg", c_f64 * 2), ("scale", c_f64 * 2), ("margin", c_f64), ("jitter", c_f64 * 4),
                ("b", c_i32), ("H", c_i32), ("W", c_i32), ("Ho", c_i32), ("Wo", c_i32), ("pad_", c_i32)]


class AugDesc(ctypes.Structure):
    _fields_ = [("image", c_vp), ("label", c_vp), ("inv", c_vp), ("color", c_vp), ("background", c_vp),
                ("out_image", c_vp), ("out_label", c_vp),
                ("image_strides", c_i64 * 4), ("label_strides", c_i64 * 3), ("background_strides", c_i64 * 4),
                ("out_image_strides", c_i64 * 4), ("out_label_strides", c_i64 * 3),
                ("fill", c_f32 * 3), ("mean", c_f32 * 3), ("std", c_f32 * 3),
                ("label_kind", c_i32), ("out_kind", c_i32), ("flags", c_i32),
                ("b", c_i32), ("H", c_i32), ("W", c_i32), ("Ho", c_i32), ("Wo", c_i32)]


# (name, restype, argtypes) -- one entry per function declared in include/pvaugment.h
SIGNATURES = [
    ("pv_augment_workspace_size", ctypes.c_size_t, [c_i32, c_i32, c_i32]),
    ("pv_label_stats", ctypes.c_int, [ctypes.POINTER(AugLabel), c_i32, c_vp, c_vp]),
    ("pv_augment_params", ctypes.c_int, [ctypes.POINTER(AugRanges), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("pv_augment_apply", ctypes.c_int, [ctypes.POINTER(AugDesc), c_vp, ctypes.c_size_t, c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVAugmentError(RuntimeError):
    pass


check = checker(PVAugmentError)
