"""ctypes binding of libpvmodel.so (include/pvmodel.h): the bounding box, centroid, farthest-point
keypoints and diameter of every model of a table.

As with ``_lib``, ``_eval_lib``, ``_pose_lib`` and ``_render_lib``: no CPU fallback.  If the library is
missing, or the tensors are not on a ROCm device, calls raise.  ``python -m pvnet_amd.build`` (or
``__graft_entry__.build()``) builds it next to libpvvote.so.
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVMODEL_LIB", os.path.join(HERE, "libpvmodel.so"))

PV_EINVAL, PV_EWORKSPACE, PV_EALIGN = -1, -2, -3
PV_MODEL_SUM_LANES = 256
PV_MODEL_MAX_K = 1024
PV_MODEL_BLOCK_MAX_PN = 12288
PV_MODEL_CHUNK = 8192
PV_MODEL_TILE = 256
PV_FPS_START_CENTROID, PV_FPS_START_CENTROID_KEPT, PV_FPS_START_INDEX = 0, 1, 2

c_i32, c_vp = ctypes.c_int32, ctypes.c_void_p


class ModelPoints(ctypes.Structure):
    _fields_ = [("points", c_vp), ("off", c_vp), ("nmodels", c_i32), ("total", c_i32), ("max_pn", c_i32),
                ("reserved_", c_i32)]


# (name, restype, argtypes) -- one entry per function declared in include/pvmodel.h
SIGNATURES = [
    ("pv_model_workspace_size", ctypes.c_size_t, [c_i32, c_i32, c_i32]),
    ("pv_model_extent", ctypes.c_int, [ctypes.POINTER(ModelPoints), c_vp, c_vp, c_vp, c_vp]),
    ("pv_farthest_points", ctypes.c_int, [ctypes.POINTER(ModelPoints), c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          ctypes.c_size_t, c_vp]),
    ("pv_model_diameter", ctypes.c_int, [ctypes.POINTER(ModelPoints), c_vp, c_vp, ctypes.c_size_t, c_vp]),
]

_lib = None
_lock = threading.Lock()


def load():
    """Load libpvmodel.so once (raises if it is absent: no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(f"libpvmodel.so not found at {LIB_PATH}; build it with `python -m pvnet_amd.build`")
            L = ctypes.CDLL(LIB_PATH)
            for name, res, args in SIGNATURES:
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


class PVModelError(RuntimeError):
    pass


_ERR = {PV_EINVAL: "invalid argument", PV_EWORKSPACE: "workspace missing or too small",
        PV_EALIGN: "pointer not aligned as documented"}


def check(code: int, what: str):
    if code != 0:
        raise PVModelError(f"{what} failed: {_ERR.get(code, 'HIP error')} (code {code})")
