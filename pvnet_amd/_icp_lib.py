"""ctypes binding of libpvicp.so (include/pvicp.h): one Gauss-Newton step of a projective
point-to-plane ICP for a batch of poses, from rendered and sensor depth maps.

No CPU fallback: if the library is missing, or the tensors are not on a ROCm device, calls raise
(``_cdll`` loads it; ``python -m pvnet_amd.build`` builds it).
"""
from __future__ import annotations

import ctypes
import os

from ._cdll import PV_EALIGN, PV_EINVAL, PV_EWORKSPACE, checker, loader  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVICP_LIB", os.path.join(HERE, "libpvicp.so"))

PV_ICP_RUNNING, PV_ICP_CONVERGED, PV_ICP_FEW, PV_ICP_NOT_PD, PV_ICP_BAD_INPUT = 0, 1, 2, 3, 4
PV_ICP_NSUM = 28
PV_ICP_RUN, PV_ICP_LANES, PV_ICP_BLOCK = 4, 256, 1024
PV_ICP_MAX_DIM = 1 << 20
PV_ICP_STAT_RMS, PV_ICP_STAT_ROT, PV_ICP_STAT_TRANS, PV_ICP_NSTAT = 0, 1, 2, 3
STATUS = {PV_ICP_RUNNING: "running", PV_ICP_CONVERGED: "converged", PV_ICP_FEW: "too few pixels",
          PV_ICP_NOT_PD: "not positive definite", PV_ICP_BAD_INPUT: "bad input"}

c_i32, c_i64, c_vp, c_f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double


class IcpBatch(ctypes.Structure):
    _fields_ = [("b", c_i32), ("n_img", c_i32), ("H", c_i32), ("W", c_i32), ("min_count", c_i32), ("reserved_", c_i32),
                ("depth_test", c_vp), ("img_id", c_vp), ("depth_est", c_vp), ("K", c_vp), ("K_stride", c_i64),
                ("dist_max", c_f64), ("edge_max", c_f64), ("lambda_", c_f64), ("max_rot", c_f64), ("max_trans", c_f64),
                ("eps_rot", c_f64), ("eps_trans", c_f64)]


class IcpState(ctypes.Structure):
    _fields_ = [("pose", c_vp), ("status", c_vp), ("iters", c_vp), ("cnt", c_vp), ("stats", c_vp), ("neq", c_vp)]


# (name, restype, argtypes) -- one entry per function declared in include/pvicp.h
SIGNATURES = [
    ("pv_icp_workspace_size", ctypes.c_size_t, [c_i32, c_i32, c_i32]),
    ("pv_icp_iterate", ctypes.c_int, [ctypes.POINTER(IcpBatch), ctypes.POINTER(IcpState), c_vp, ctypes.c_size_t, c_vp]),
]

load = loader(LIB_PATH, SIGNATURES)


class PVIcpError(RuntimeError):
    pass


check = checker(PVIcpError)
