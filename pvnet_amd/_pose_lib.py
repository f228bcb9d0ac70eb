"""ctypes binding of libpvpose.so (include/pvpose.h): batched EPnP.

As with ``_lib`` and ``_eval_lib``: no CPU fallback.  If the library is missing, or the
tensors are not on a ROCm device, calls raise.  ``python -m pvnet_amd.build`` (or
``__graft_entry__.build()``) builds it next to libpvvote.so.
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVPOSE_LIB", os.path.join(HERE, "libpvpose.so"))

PV_EINVAL, PV_EWORKSPACE, PV_EALIGN = -1, -2, -3
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

_lib = None
_lock = threading.Lock()


def load():
    """Load libpvpose.so once (raises if it is absent: no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(f"libpvpose.so not found at {LIB_PATH}; build it with `python -m pvnet_amd.build`")
            L = ctypes.CDLL(LIB_PATH)
            for name, res, args in SIGNATURES:
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


class PVPoseError(RuntimeError):
    pass


_ERR = {PV_EINVAL: "invalid argument", PV_EWORKSPACE: "workspace missing or too small",
        PV_EALIGN: "pointer not aligned as documented"}


def check(code: int, what: str):
    if code != 0:
        raise PVPoseError(f"{what} failed: {_ERR.get(code, 'HIP error')} (code {code})")
