"""ctypes binding of libpvloss.so (include/pvloss.h): the per-image cross-entropy, mask-weighted
smooth-L1, precision / recall counts and the gradients of the two predictions.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVLOSS_LIB", os.path.join(HERE, "libpvloss.so"))

PV_LOSS_LABEL_I64, PV_LOSS_LABEL_U8, PV_LOSS_LABEL_I32 = 0, 1, 2
PV_LOSS_F32, PV_LOSS_F16 = 0, 1
PV_LOSS_PIXELS = 8
PV_LOSS_THREADS = 256
PV_LOSS_MAX_DIM = 2 ** 20
PV_LOSS_MAX_CLASSES = 1024
PV_LOSS_MAX_CHUNKS = 8

c_i32, c_i64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


class LossDesc(ctypes.Structure):
    _fields_ = [("seg", c_vp), ("vertex", c_vp), ("target", c_vp), ("label", c_vp),
                ("seg_strides", c_i64 * 4), ("vertex_strides", c_i64 * 5), ("target_strides", c_i64 * 5),
                ("label_strides", c_i64 * 3),
                ("seg_kind", c_i32), ("vertex_kind", c_i32), ("target_kind", c_i32), ("label_kind", c_i32),
                ("b", c_i32), ("H", c_i32), ("W", c_i32), ("ncls", c_i32), ("vn", c_i32), ("sigma", ctypes.c_float)]


class LossOut(ctypes.Structure):
    _fields_ = [("loss_seg", c_vp), ("loss_vertex", c_vp), ("fg", c_vp), ("counts", c_vp)]


class LossGrad(ctypes.Structure):
    _fields_ = [("g_seg", c_vp), ("g_vertex", c_vp), ("fg", c_vp), ("grad_seg", c_vp), ("grad_vertex", c_vp),
                ("grad_seg_strides", c_i64 * 4), ("grad_vertex_strides", c_i64 * 5)]


# (name, restype, argtypes) -- one entry per function declared in include/pvloss.h
SIGNATURES = [
    ("pv_loss_workspace_size", ctypes.c_size_t, [c_i32, c_i32, c_i32, c_i32]),
    ("pv_loss_forward", ctypes.c_int, [ctypes.POINTER(LossDesc), ctypes.POINTER(LossOut), c_vp, ctypes.c_size_t, c_vp]),
    ("pv_loss_backward", ctypes.c_int, [ctypes.POINTER(LossDesc), ctypes.POINTER(LossGrad), c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVLossError(RuntimeError):
    pass


check = checker(PVLossError)
