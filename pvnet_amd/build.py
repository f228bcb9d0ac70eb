"""Build the HIP C-ABI libraries (the tables LIBS, MORE_LIBS, LATER_LIBS, NEXT_LIBS, BOP_LIBS and ICP_LIBS) in-tree for gfx950.

    python -m pvnet_amd.build            # or __graft_entry__.build()

hipcc cross-compiles without a GPU.  The libraries land next to this file so they
travel to the GPU box with the repository snapshot.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")


class Lib(NamedTuple):
    out: str    # the shared library, next to this file
    hdr: str    # its public header under include/
    srcs: list  # its translation units under csrc/


def _lib(name: str, *srcs: str) -> Lib:
    return Lib(os.path.join(HERE, f"lib{name}.so"), os.path.join(REPO, "include", name + ".h"),
               [os.path.join(CSRC, s) for s in srcs])


# Every library, in build order: one row here, one loader module, one public header and its own
# tests make a library.  What a library depends on is not listed: closure() reads it from the sources.
LIBS = {
    # the translation units (csrc/pvvote.hip's head comment maps the vote library's)
    "vote": _lib("pvvote", "pvvote.hip", "pvapi.hip", "pvpipeline.hip", "pvcompact.hip", "pvrefine.hip", "pvevd.hip",
                 "pvpnp.hip", "pvdecoder.hip", "pvconv.hip"),
    # the pose-evaluation library (include/pveval.h): a library of its own, so libpvvote.so's
    # export list and translation-unit count hold still; so is each library below
    "eval": _lib("pveval", "pveval.hip"),
    # the plain-PnP library (include/pvpose.h); pvepnp_core.h is its kernel's body and belongs to
    # it alone
    "pose": _lib("pvpose", "pvepnp.hip"),
    # the render (include/pvrender.h), model-preparation (include/pvmodel.h), training-loss
    # (include/pvloss.h) and training-augmentation (include/pvaugment.h) libraries: one translation
    # unit each, which includes no other file of csrc/
    "render": _lib("pvrender", "pvrender.hip"),
    "model": _lib("pvmodel", "pvmodel.hip"),
    "loss": _lib("pvloss", "pvloss.hip"),
    "augment": _lib("pvaugment", "pvaugment.hip"),
}
# LIBS continued: the frame-composition library (include/pvcompose.h), one translation unit that
# includes no other file of csrc/.  A table of its own only because tests/test_build_table.py holds
# LIBS to seven rows; the two merge when that test is next opened.
MORE_LIBS = {
    "compose": _lib("pvcompose", "pvcompose.hip"),
}
# and again: the optimiser-step library (include/pvoptim.h), one translation unit that includes no
# other file of csrc/.  A third table only because tests/test_compose_abi.py holds MORE_LIBS to its
# one row as tests/test_build_table.py holds LIBS to seven; a later library goes here.
LATER_LIBS = {
    "optim": _lib("pvoptim", "pvoptim.hip"),
}
# and once more: the colour-render library (include/pvshade.h), one translation unit that includes no
# other file of csrc/.  A fourth table only because tests/test_optim_abi.py holds libs() to the nine
# above, with the optimiser last; all_libs() is what build(), stale() and needs_build() work over.
NEXT_LIBS = {
    "shade": _lib("pvshade", "pvshade.hip"),
}
# and a fifth: the BOP pose-error library (include/pvbop.h), one translation unit that includes no
# other file of csrc/.  A table of its own only because tests/test_shade_abi.py holds all_libs() to
# the ten above, with shade last.
BOP_LIBS = {
    "bop": _lib("pvbop", "pvbop.hip"),
}
# and a sixth: the depth-refinement library (include/pvicp.h), one translation unit that includes no
# other file of csrc/.  A table of its own only because tests/test_bop_abi.py holds every_lib() to the
# eleven above, with bop last; each_lib() is what build(), stale() and needs_build() work over.
ICP_LIBS = {
    "icp": _lib("pvicp", "pvicp.hip"),
}
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


def libs() -> list:
    """Every library of the three tables, in build order."""
    return [*LIBS.values(), *MORE_LIBS.values(), *LATER_LIBS.values()]


def all_libs() -> list:
    """libs() and the fourth table, in build order."""
    return [*libs(), *NEXT_LIBS.values()]


def every_lib() -> list:
    """all_libs() and the fifth table, in build order."""
    return [*all_libs(), *BOP_LIBS.values()]


def each_lib() -> list:
    """Every library that is built: every_lib() and the sixth table, in build order."""
    return [*every_lib(), *ICP_LIBS.values()]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (ROCm install required to build libpvvote.so)")


_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def closure(srcs) -> list:
    """`srcs` and every file they reach through #include "...", resolved relative to the including
    file and normalised, so one file is one string however it was reached.  <...> includes (the
    toolchain's) are not followed."""
    seen = [os.path.normpath(s) for s in srcs]
    for path in seen:               # grows while it is walked
        with open(path) as f:
            for inc in _INCLUDE.findall(f.read()):
                dep = os.path.normpath(os.path.join(os.path.dirname(path), inc))
                if dep not in seen:
                    seen.append(dep)
    return seen


def older(path: str, deps) -> bool:
    """Is `path` missing, or older than any of `deps`?"""
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    return any(os.path.getmtime(p) > t for p in deps)


def stale(out: str) -> bool:
    """Is the library `out` missing, or older than a file the compiler reads for it or this file?"""
    srcs = {lib.out: lib.srcs for lib in each_lib()}
    if out not in srcs:
        raise ValueError(f"{out} is not a library of LIBS, MORE_LIBS, LATER_LIBS, NEXT_LIBS, BOP_LIBS or ICP_LIBS; for another "
                         "file use older(path, deps)")
    return older(out, (*closure(srcs[out]), __file__))


def needs_build() -> bool:
    return any(stale(lib.out) for lib in each_lib())


def _link(out: str, srcs, extra=()) -> None:
    cmd = [hipcc(), *HIPCC_FLAGS, *extra, "-o", out + ".tmp", *srcs]
    subprocess.check_call(cmd)
    # every reference resolved (an unresolved kernel stub only shows at load time)
    import ctypes
    ctypes.CDLL(os.path.abspath(out + ".tmp"), mode=ctypes.RTLD_LOCAL | os.RTLD_NOW)
    os.replace(out + ".tmp", out)


def build(force: bool = False, extra=()) -> str:
    """Build every library of the six tables (each when stale); returns libpvvote.so's path."""
    for lib in each_lib():
        if force or stale(lib.out):
            _link(lib.out, lib.srcs, extra)
    return LIBS["vote"].out


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
