"""ctypes binding of libpvpose.so (include/pvpose.h): batched EPnP.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVPOSE_LIB", os.path.join(HERE, "libpvpose.so"))

PV_EPNP_OK, PV_EPNP_DEGENERATE = 0, 1
PV_EPNP_MIN_POINTS, PV_EPNP_MAX_POINTS = 6, 64

c_i32, c_i64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


class EpnpBatch(ctypes.Structure):
    _fields_ = [("b", c_i32), ("pn", c_i32), ("pts2d", c_vp), ("pts2d64", c_vp), ("pts3d", c_vp), ("K", c_vp),
                ("pts3d_stride", c_i64), ("K_stride", c_i64)]


class EpnpDiag(ctypes.Structure):
    _fields_ = [("status", c_vp), ("n_used", c_vp), ("cand_err", c_vp)]


# (name, restype, argtypes) -- one entry per function declared in include/pvpose.h
SIGNATURES = [
    ("pv_epnp", ctypes.c_int, [ctypes.POINTER(EpnpBatch), c_vp, c_vp, ctypes.POINTER(EpnpDiag), c_vp]),
    ("pv_rt6_to_Rt", ctypes.c_int, [c_vp, c_vp, c_i32, c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVPoseError(RuntimeError):
    pass


check = checker(PVPoseError)
