"""ctypes binding of libpvmodel.so (include/pvmodel.h): the bounding box, centroid, farthest-point
keypoints and diameter of every model of a table.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVMODEL_LIB", os.path.join(HERE, "libpvmodel.so"))

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

load = loader(LIB_PATH, SIGNATURES)


class PVModelError(RuntimeError):
    pass


check = checker(PVModelError)
