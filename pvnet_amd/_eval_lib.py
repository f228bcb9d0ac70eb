"""ctypes binding of libpveval.so (include/pveval.h): batched pose evaluation.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVEVAL_LIB", os.path.join(HERE, "libpveval.so"))

PV_EVAL_ADD, PV_EVAL_ADDS, PV_EVAL_PROJ, PV_EVAL_PROJ_SYM, PV_EVAL_CMDEG = 1, 2, 4, 8, 16
PV_EVAL_ALL = 31
# metric name -> (request bit, columns of out [b][PV_EVAL_NCOL] it fills)
COLUMNS = ("add", "adds", "proj", "proj_sym", "trans_cm", "rot_deg")
METRICS = {"add": (PV_EVAL_ADD, (0,)), "adds": (PV_EVAL_ADDS, (1,)), "proj": (PV_EVAL_PROJ, (2,)),
           "proj_sym": (PV_EVAL_PROJ_SYM, (3,)), "cmdeg": (PV_EVAL_CMDEG, (4, 5))}
PV_EVAL_NCOL = 6

c_i32, c_i64, c_u32, c_size, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p


class EvalBatch(ctypes.Structure):
    _fields_ = [("b", c_i32), ("total", c_i32), ("pose_pred", c_vp), ("pose_gt", c_vp), ("model", c_vp),
                ("model_off", c_vp), ("model_id", c_vp), ("nmodels", c_i32), ("max_pn", c_i32), ("K", c_vp),
                ("K_stride", c_i64), ("metrics", c_u32)]


# (name, restype, argtypes) -- one entry per function declared in include/pveval.h
SIGNATURES = [
    ("pv_nearest_point_idx", ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    ("pv_eval_workspace_size", c_size, [c_i32, c_i32]),
    ("pv_pose_metrics", ctypes.c_int, [ctypes.POINTER(EvalBatch), c_vp, c_vp, c_size, c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVEvalError(RuntimeError):
    pass


check = checker(PVEvalError)
