"""ctypes binding of libpveval.so (include/pveval.h): batched pose evaluation.

As with ``_lib``: no CPU fallback.  If the library is missing, or the tensors
are not on a ROCm device, calls raise.  ``python -m pvnet_amd.build`` (or
``__graft_entry__.build()``) builds it next to libpvvote.so.
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVEVAL_LIB", os.path.join(HERE, "libpveval.so"))

PV_EINVAL, PV_EWORKSPACE, PV_EALIGN = -1, -2, -3
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

_lib = None
_lock = threading.Lock()


def load():
    """Load libpveval.so once (raises if it is absent: no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(f"libpveval.so not found at {LIB_PATH}; build it with `python -m pvnet_amd.build`")
            L = ctypes.CDLL(LIB_PATH)
            for name, res, args in SIGNATURES:
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


class PVEvalError(RuntimeError):
    pass


_ERR = {PV_EINVAL: "invalid argument", PV_EWORKSPACE: "workspace missing or too small",
        PV_EALIGN: "pointer not aligned as documented"}


def check(code: int, what: str):
    if code != 0:
        raise PVEvalError(f"{what} failed: {_ERR.get(code, 'HIP error')} (code {code})")
