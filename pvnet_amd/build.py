"""Build libpvvote.so, libpveval.so, libpvpose.so, libpvrender.so, libpvmodel.so, libpvloss.so and
libpvaugment.so (the HIP C-ABI libraries) in-tree for gfx950.

    python -m pvnet_amd.build            # or __graft_entry__.build()

hipcc cross-compiles without a GPU.  The libraries land next to this file so they
travel to the GPU box with the repository snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
# the translation units (csrc/pvvote.hip's head comment maps the vote library's)
SRCS = [os.path.join(CSRC, n) for n in (
    "pvvote.hip", "pvapi.hip", "pvpipeline.hip", "pvcompact.hip", "pvrefine.hip", "pvevd.hip", "pvpnp.hip",
    "pvdecoder.hip", "pvconv.hip")]
HDR = os.path.join(REPO, "include", "pvvote.h")
OUT = os.path.join(HERE, "libpvvote.so")
# the pose-evaluation library (include/pveval.h): a library of its own, so libpvvote.so's
# export list and translation-unit count hold still
EVAL_SRCS = [os.path.join(CSRC, "pveval.hip")]
EVAL_HDR = os.path.join(REPO, "include", "pveval.h")
EVAL_OUT = os.path.join(HERE, "libpveval.so")
# the plain-PnP library (include/pvpose.h), a third library for the same reason; pvepnp_core.h is
# its kernel's body and belongs to it alone
POSE_SRCS = [os.path.join(CSRC, "pvepnp.hip")]
POSE_HDR = os.path.join(REPO, "include", "pvpose.h")
POSE_OUT = os.path.join(HERE, "libpvpose.so")
POSE_DEPS = (*POSE_SRCS, os.path.join(CSRC, "pvepnp_core.h"), POSE_HDR)
# the render library (include/pvrender.h), a fourth for the same reason; its one translation unit
# includes no other file of csrc/
RENDER_SRCS = [os.path.join(CSRC, "pvrender.hip")]
RENDER_HDR = os.path.join(REPO, "include", "pvrender.h")
RENDER_OUT = os.path.join(HERE, "libpvrender.so")
RENDER_DEPS = (*RENDER_SRCS, RENDER_HDR)
# the model-preparation library (include/pvmodel.h), a fifth; like the render library its one
# translation unit includes no other file of csrc/
MODEL_SRCS = [os.path.join(CSRC, "pvmodel.hip")]
MODEL_HDR = os.path.join(REPO, "include", "pvmodel.h")
MODEL_OUT = os.path.join(HERE, "libpvmodel.so")
MODEL_DEPS = (*MODEL_SRCS, MODEL_HDR)
# the training-loss library (include/pvloss.h), a sixth; again one translation unit that includes no
# other file of csrc/
LOSS_SRCS = [os.path.join(CSRC, "pvloss.hip")]
LOSS_HDR = os.path.join(REPO, "include", "pvloss.h")
LOSS_OUT = os.path.join(HERE, "libpvloss.so")
LOSS_DEPS = (*LOSS_SRCS, LOSS_HDR)
# the training-augmentation library (include/pvaugment.h), a seventh; one translation unit that
# includes no other file of csrc/
AUG_SRCS = [os.path.join(CSRC, "pvaugment.hip")]
AUG_HDR = os.path.join(REPO, "include", "pvaugment.h")
AUG_OUT = os.path.join(HERE, "libpvaugment.so")
AUG_DEPS = (*AUG_SRCS, AUG_HDR)
ARCH = os.environ.get("PVVOTE_ARCH", "gfx950")

HIPCC_FLAGS = [
    f"--offload-arch={ARCH}",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-shared",
    # every expression restating reference arithmetic rounds after each op;
    # the approximate test's FMAs are explicit fmaf() calls
    "-ffp-contract=off",
    "-fhip-fp32-correctly-rounded-divide-sqrt",
    # packed f32 (v_pk_*) has no throughput advantage on gfx950 and costs
    # the abs/neg source modifiers the vote test relies on
    "-fno-slp-vectorize",
    "-fno-gpu-rdc",
    # MFMA results straight into VGPRs (gfx950's unified register file): the
    # vote kernel's VALU reads them without v_accvgpr_read copies
    "-mllvm", "-amdgpu-mfma-vgpr-form=1",
    "-Wall",
]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (ROCm install required to build libpvvote.so)")


def stale(out: str) -> bool:
    """Is `out` missing, or older than any source under csrc/, a public header or this file?
    For each library the other six's translation units and public headers do not count, and
    libpvrender.so, libpvmodel.so, libpvloss.so and libpvaugment.so, which include nothing else of
    csrc/, depend on their own sources alone."""
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    own = {RENDER_OUT: RENDER_DEPS, MODEL_OUT: MODEL_DEPS, LOSS_OUT: LOSS_DEPS, AUG_OUT: AUG_DEPS}.get(out)
    if own is not None:
        return any(os.path.getmtime(p) > t for p in (*own, __file__))
    other = {OUT: (*EVAL_SRCS, EVAL_HDR, *POSE_DEPS, *RENDER_DEPS, *MODEL_DEPS, *LOSS_DEPS, *AUG_DEPS),
             EVAL_OUT: (*SRCS, *POSE_DEPS, *RENDER_DEPS, *MODEL_DEPS, *LOSS_DEPS, *AUG_DEPS),
             POSE_OUT: (*SRCS, *EVAL_SRCS, EVAL_HDR, *RENDER_DEPS, *MODEL_DEPS, *LOSS_DEPS, *AUG_DEPS)}.get(out, ())
    deps = [os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith((".hip", ".h"))]
    return any(os.path.getmtime(p) > t for p in (*deps, HDR, EVAL_HDR, POSE_HDR, RENDER_HDR, __file__)
               if p not in other)


def needs_build() -> bool:
    return any(stale(o) for o in (OUT, EVAL_OUT, POSE_OUT, RENDER_OUT, MODEL_OUT, LOSS_OUT, AUG_OUT))


def _link(out: str, srcs, extra=()) -> None:
    cmd = [hipcc(), *HIPCC_FLAGS, *extra, "-o", out + ".tmp", *srcs]
    subprocess.check_call(cmd)
    # every reference resolved (an unresolved kernel stub only shows at load time)
    import ctypes
    ctypes.CDLL(os.path.abspath(out + ".tmp"), mode=ctypes.RTLD_LOCAL | os.RTLD_NOW)
    os.replace(out + ".tmp", out)


def build(force: bool = False, extra=()) -> str:
    """Build libpvvote.so, libpveval.so, libpvpose.so, libpvrender.so, libpvmodel.so, libpvloss.so and
    libpvaugment.so (each when stale); returns libpvvote.so's path."""
    if force or stale(OUT):
        _link(OUT, SRCS, extra)
    if force or stale(EVAL_OUT):
        _link(EVAL_OUT, EVAL_SRCS, extra)
    if force or stale(POSE_OUT):
        _link(POSE_OUT, POSE_SRCS, extra)
    if force or stale(RENDER_OUT):
        _link(RENDER_OUT, RENDER_SRCS, extra)
    if force or stale(MODEL_OUT):
        _link(MODEL_OUT, MODEL_SRCS, extra)
    if force or stale(LOSS_OUT):
        _link(LOSS_OUT, LOSS_SRCS, extra)
    if force or stale(AUG_OUT):
        _link(AUG_OUT, AUG_SRCS, extra)
    return OUT


def asm(tu: str = "pvvote.hip", path: str | None = None, extra=()) -> str:
    """Device assembly of one translation unit (csrc/TU, or a path) for
    inspection (kernel resource usage, v_cmp/s_bcnt1 loops); default output
    csrc/<TU's base name>.gfx950.s."""
    src = tu if os.path.isabs(tu) else os.path.join(CSRC, tu)
    path = path or os.path.join(CSRC, os.path.splitext(os.path.basename(src))[0] + ".gfx950.s")
    cmd = [hipcc(), *[f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC", "-Wall")], *extra,
           "--cuda-device-only", "-S", "-o", path, src]
    subprocess.check_call(cmd)
    return path


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
