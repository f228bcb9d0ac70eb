"""ctypes binding of libpvoptim.so (include/pvoptim.h): the mixed-precision optimiser step -- the
gradients' non-finite check and global norm, the decision on the device, and the Adam / AdamW / SGD
update with the f16 model copy and the zeroed gradients.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVOPTIM_LIB", os.path.join(HERE, "libpvoptim.so"))

PV_OPT_F32, PV_OPT_F16 = 0, 1
PV_OPT_ADAM, PV_OPT_ADAMW, PV_OPT_SGD = 0, 1, 2
PV_OPT_CHUNK = 8192
PV_OPT_THREADS = 256
PV_OPT_GROUP = 8

c_i32, c_i64, c_vp, c_f32, c_f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double


class OptTensor(ctypes.Structure):
    _fields_ = [("master", c_vp), ("model", c_vp), ("grad", c_vp), ("m", c_vp), ("v", c_vp), ("n", c_i64),
                ("grad_kind", c_i32), ("pad_", c_i32)]


class OptChunk(ctypes.Structure):
    _fields_ = [("first", c_i64), ("tensor", c_i32), ("pad_", c_i32)]


class OptState(ctypes.Structure):
    _fields_ = [("b1pow", c_f64), ("b2pow", c_f64), ("step", c_i64), ("lr", c_f32), ("scale", c_f32),
                ("growth_tracker", c_i32), ("grad_norm", c_f32), ("found_inf", c_i32), ("skipped", c_i32)]


class OptDesc(ctypes.Structure):
    _fields_ = [("algorithm", c_i32), ("beta1", c_f32), ("beta2", c_f32), ("eps", c_f32), ("weight_decay", c_f32),
                ("momentum", c_f32), ("max_norm", c_f32), ("growth_factor", c_f32), ("backoff_factor", c_f32),
                ("growth_interval", c_i32), ("zero_grads", c_i32), ("pad_", c_i32)]


# (name, restype, argtypes) -- one entry per function declared in include/pvoptim.h
SIGNATURES = [
    ("pv_optim_plan", c_i64, [ctypes.POINTER(OptTensor), c_i32, c_i32, ctypes.POINTER(OptChunk), c_i64]),
    ("pv_optim_workspace_size", ctypes.c_size_t, [c_i64]),
    ("pv_optim_step", ctypes.c_int, [ctypes.POINTER(OptDesc), c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, ctypes.c_size_t, c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVOptimError(RuntimeError):
    pass


check = checker(PVOptimError)
