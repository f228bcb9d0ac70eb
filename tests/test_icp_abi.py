"""CPU-side checks of libpvicp.so (include/pvicp.h): it builds for gfx950 from the sixth table of
pvnet_amd/build.py, exports exactly its header, stands apart from the other eleven libraries and
rejects bad arguments on the host."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.test_build_table import HEADERS, exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_icp_iterate", "pv_icp_workspace_size"]
ELEVEN = [*HEADERS, "pvcompose.h", "pvoptim.h", "pvshade.h", "pvbop.h"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _icp_lib
    build.build()
    return _icp_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    assert list(build.ICP_LIBS) == ["icp"] and list(build.BOP_LIBS) == ["bop"] and len(build.LIBS) == 7
    eleven = [lib_.out for lib_ in build.every_lib()]
    icp = build.ICP_LIBS["icp"]
    assert len(set(eleven)) == 11 and [lib_.out for lib_ in build.each_lib()] == [*eleven, icp.out] and icp.out not in eleven
    assert isinstance(icp, build.Lib)
    assert icp.out == os.path.join(REPO, "pvnet_amd", "libpvicp.so")
    assert icp.hdr == os.path.join(REPO, "include", "pvicp.h")
    assert [os.path.basename(s) for s in icp.srcs] == ["pvicp.hip"]
    assert b"gfx950" in open(icp.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    assert all(os.path.exists(lib_.out) for lib_ in build.each_lib())
    src = open(icp.srcs[0]).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../../include/pvicp.h"]
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    # no fast-math form, no fused multiply-add, no matrix instruction, no atomic of any kind, no inline assembly,
    # no transcendental
    assert not re.search(r"__fdividef|__fsqrt|__frsqrt|rsqrtf?\s*\(|\bfmaf?\s*\(|mfma_|\batomic\w*\s*\(|\basm\b", src)
    assert not re.search(r"\b(sin|cos|tan|atan2?|acos|asin|exp|log|pow)f?\s*\(", src)
    assert src.count("<<<") == 2                                        # two launches a call
    hdr = open(icp.hdr).read()
    for name in ("pvbop.h", "pvrender.h", "tests/icp_ref.py", "hipGraph", "bit for bit", "Cayley", "increasing k",
                 "exactly two launches"):
        assert name in hdr, name
    assert '#include "' not in hdr


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _icp_lib
    assert header_functions("pvicp.h") == NAMES
    assert exported(build.ICP_LIBS["icp"].out) == set(NAMES)
    assert {n for n, _, _ in _icp_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_icp_lib.py"
    # the library whose depth maps this one reads gained nothing
    assert exported(build.BOP_LIBS["bop"].out) == {"pv_bop_sym_errors", "pv_bop_vsd", "pv_bop_workspace_size"}


def test_closure_and_staleness(lib, monkeypatch):
    from pvnet_amd import build
    icp = build.ICP_LIBS["icp"]
    got = build.closure(icp.srcs)
    assert set(got) == {*icp.srcs, icp.hdr} and len(got) == 2
    mm = subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "--cuda-host-only", "-MM", *icp.srcs],
                        capture_output=True, text=True, check=True).stdout
    read = {os.path.realpath(w) for w in mm.replace("\\\n", " ").split() if not w.endswith(":")}
    root = os.path.realpath(REPO) + os.sep
    assert {p for p in read if p.startswith(root)} == {os.path.realpath(p) for p in got}
    eleven = [set(build.closure(lib_.srcs)) for lib_ in build.every_lib()]
    assert len(eleven) == 11
    for lib_, files in zip(build.every_lib(), eleven):
        assert not files & set(got), lib_.out
    # which edit makes which library stale: modification times simulated, no file touched
    outs = [lib_.out for lib_ in build.each_lib()]
    assert outs[-1] == icp.out and len(outs) == 12
    real = os.path.getmtime
    newest = max(real(p) for p in outs) + 10

    def stale_after(paths):
        monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p in paths else real(p))
        return tuple(build.stale(o) for o in outs)

    F, T = False, True
    assert stale_after(set()) == (F,) * 12
    assert stale_after({icp.hdr}) == stale_after(set(icp.srcs)) == stale_after(set(got)) == (F,) * 11 + (T,)
    assert stale_after({build.__file__}) == (T,) * 12
    assert stale_after(set().union(*eleven)) == (T,) * 11 + (F,)
    bop = build.BOP_LIBS["bop"]
    assert stale_after({bop.hdr, *bop.srcs}) == tuple(o == bop.out for o in outs)
    for name in ("_icp_lib.py", "icp.py", "evaluation_utils.py", "__init__.py"):
        assert stale_after({os.path.join(REPO, "pvnet_amd", name)}) == (F,) * 12
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p == icp.hdr else real(p))
    assert build.needs_build()
    monkeypatch.undo()
    assert not build.needs_build()
    with pytest.raises(ValueError, match="ICP_LIBS"):
        build.stale(os.path.join(REPO, "pvnet_amd", "libpvnothing.so"))


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_first_and_last_among_the_twelve(tmp_path, lang):
    from pvnet_amd import build
    if lang == "c":
        cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c"]) + ["-std=c99", "-pedantic-errors"]
    else:
        cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c++"]) + ["-std=c++17"]
    assert len(ELEVEN) == 11 and all(os.path.exists(os.path.join(REPO, "include", h)) for h in ELEVEN)
    assert sorted(os.listdir(os.path.join(REPO, "include"))) == sorted([*ELEVEN, "pvicp.h"])
    orders = [["pvicp.h"], ["pvicp.h", *ELEVEN], [*ELEVEN, "pvicp.h"], ["pvicp.h", *ELEVEN[::-1]], [*ELEVEN[::-1], "pvicp.h"]]
    for i, order in enumerate(orders):
        src = tmp_path / f"order{i}.{'c' if lang == 'c' else 'cpp'}"
        src.write_text("".join(f'#include "{h}"\n' for h in order) +
                       "int pv_order_probe(pv_stream_t s, const pv_icp_batch *m, const pv_icp_state *v);\n"
                       "int pv_order_probe(pv_stream_t s, const pv_icp_batch *m, const pv_icp_state *v) "
                       "{ return s ? PV_OK : PV_EINVAL + PV_EWORKSPACE + PV_EALIGN + m->min_count + (v->neq != 0) + "
                       "PV_ICP_BAD_INPUT + PV_ICP_NSUM + PV_ICP_NSTAT; }\n")
        r = subprocess.run([*cc, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (order, r.stderr)


def test_header_constants_and_structures_match_binding():
    from pvnet_amd import _icp_lib as P
    from tests import icp_ref as R
    src = open(os.path.join(REPO, "include", "pvicp.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)u?\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    names = ("PV_ICP_RUNNING", "PV_ICP_CONVERGED", "PV_ICP_FEW", "PV_ICP_NOT_PD", "PV_ICP_BAD_INPUT", "PV_ICP_NSUM",
             "PV_ICP_RUN", "PV_ICP_LANES", "PV_ICP_BLOCK", "PV_ICP_MAX_DIM", "PV_ICP_STAT_RMS", "PV_ICP_STAT_ROT",
             "PV_ICP_STAT_TRANS", "PV_ICP_NSTAT")
    assert {k for k in defs if k.startswith("PV_ICP_")} == set(names)
    for name in names:
        assert defs[name] == getattr(P, name), name
    assert defs["PV_ICP_BLOCK"] == defs["PV_ICP_RUN"] * defs["PV_ICP_LANES"]
    assert (R.RUNNING, R.CONVERGED, R.FEW, R.NOT_PD, R.BAD_INPUT) == (0, 1, 2, 3, 4) == tuple(sorted(P.STATUS))
    assert (R.NSUM, R.RUN, R.LANES, R.BLOCK) == (P.PV_ICP_NSUM, P.PV_ICP_RUN, P.PV_ICP_LANES, P.PV_ICP_BLOCK)
    B, S = P.IcpBatch, P.IcpState
    assert ctypes.sizeof(B) == 6 * 4 + 5 * 8 + 7 * 8 == 120
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112]
    assert ctypes.sizeof(S) == 6 * 8 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32, 40]
    for struct, cls in (("pv_icp_batch", B), ("pv_icp_state", S)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\b([A-Za-z_0-9]+)\s*(?:,|$)", decl.strip())]
        assert names == [f.rstrip("_") if f == "lambda_" else f for f, _ in cls._fields_], struct


def test_workspace_size(lib):
    f = lib.pv_icp_workspace_size
    assert f(0, 8, 8) == 0 and f(1, 0, 8) == 0 and f(1, 8, 0) == 0 and f(-1, 8, 8) == 0
    assert f(1, 1, 1) == 256                                             # one block: 28 f64 and one i32, to 256 bytes
    for b, H, W in ((1, 32, 32), (3, 25, 41), (256, 480, 640), (1000, 1080, 1920)):
        got = f(b, H, W)
        nblk = -(-H * W // 1024)
        assert got % 256 == 0 and 0 <= got - b * nblk * (28 * 8 + 4) < 256


def test_argument_errors_without_device(lib):
    from pvnet_amd import _icp_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    nan, inf = float("nan"), float("inf")
    E, EW, EA = P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN
    need = lib.pv_icp_workspace_size(2, 16, 16)

    def go(null=False, nullst=False, ws=p, nbytes=need, st=None, **kw):
        bt = dict(b=2, n_img=2, H=16, W=16, min_count=6, reserved_=0, depth_test=p, img_id=None, depth_est=p, K=p, K_stride=0,
                  dist_max=0.02, edge_max=0.01, lambda_=1e-6, max_rot=0.2, max_trans=0.05, eps_rot=1e-5, eps_trans=1e-5)
        bt.update(kw)
        so = dict(pose=p, status=p, iters=p, cnt=p, stats=p, neq=p)
        so.update(st or {})
        B, S = P.IcpBatch(**bt), P.IcpState(**so)
        return lib.pv_icp_iterate(None if null else ctypes.byref(B), None if nullst else ctypes.byref(S), ws, nbytes, None)

    # a complete call is only stopped by its workspace, so no pointer is touched in any of this
    assert go(ws=None) == EW and go(nbytes=need - 1) == EW and go(nbytes=0) == EW
    assert go(null=True) == E and go(nullst=True) == E
    for kw in (dict(b=-1), dict(n_img=-1), dict(min_count=-1), dict(K_stride=-1), dict(H=0), dict(W=0), dict(H=2 ** 20 + 1),
               dict(W=2 ** 20 + 1), dict(dist_max=-1.0), dict(dist_max=nan), dict(edge_max=-1.0), dict(edge_max=nan),
               dict(eps_rot=-1.0), dict(eps_rot=nan), dict(eps_trans=-1.0), dict(eps_trans=nan), dict(lambda_=-1.0),
               dict(lambda_=nan), dict(lambda_=inf), dict(max_rot=0.0), dict(max_rot=-1.0), dict(max_rot=nan),
               dict(max_trans=0.0), dict(max_trans=nan), dict(depth_est=None), dict(K=None), dict(depth_test=None),
               dict(b=2 ** 22, H=2 ** 20, W=2 ** 20)):
        assert go(ws=None, **kw) == E, kw
    for k in ("pose", "status", "iters", "cnt", "stats"):
        assert go(ws=None, st={k: None}) == E, k
    # what may be NULL or infinite: neq, img_id, depth_test without images, the limits and the gates
    assert go(ws=None, st=dict(neq=None)) == EW and go(ws=None, img_id=p) == EW
    assert go(ws=None, depth_test=None, n_img=0) == EW
    assert go(ws=None, dist_max=inf, edge_max=inf, max_rot=inf, max_trans=inf, eps_rot=inf, eps_trans=inf, lambda_=0.0,
              min_count=0) == EW
    for kw in (dict(K=260), dict(depth_test=258), dict(depth_est=257), dict(img_id=258)):
        assert go(**kw) == EA, kw
    for k, v in (("pose", 260), ("stats", 260), ("neq", 260), ("status", 258), ("iters", 258), ("cnt", 257)):
        assert go(st={k: v}) == EA, k
    assert go(ws=260) == EA
    # nothing to do: success, whatever the pointers
    assert go(b=0, ws=None, nbytes=0, depth_est=None, K=None, st=dict(pose=None, status=None, iters=None, cnt=None, stats=None)) == 0


def test_python_layer_rejects_before_any_call():
    import numpy as np
    import torch
    import pvnet_amd
    from pvnet_amd import icp
    from pvnet_amd.evaluation_utils import Evaluator, ModelTable
    assert pvnet_amd.refine_depth is icp.refine_depth and "refine_depth" in pvnet_amd.__all__
    poses = torch.zeros((2, 3, 4), dtype=torch.float64)
    depth = torch.zeros((2, 4, 4))
    with pytest.raises(RuntimeError, match="device"):
        icp.refine_depth(None, poses, None, depth, np.eye(3))             # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="device"):
        icp.linearise(None, poses, None, depth, np.eye(3))
    with pytest.raises(RuntimeError, match="device"):
        icp.new_state(poses)
    with pytest.raises(RuntimeError, match="device"):
        icp.iterate(dict(pose=poses), depth, depth, np.eye(3))
    with pytest.raises(TypeError, match="unknown ICP parameter"):
        icp.refine_depth(None, poses, None, depth, np.eye(3), huber=1.0)
    table = ModelTable([(np.zeros((4, 3)), 0.1, False)], device="cpu")
    with pytest.raises(RuntimeError, match="device"):
        Evaluator(table, np.zeros((1, 9, 3))).refine_depth(poses, None, depth, np.eye(3), None)
    assert set(icp.DEFAULTS) == {"dist_max", "edge_max", "lam", "min_count", "max_rot", "max_trans", "eps_rot", "eps_trans"}
    assert "metres" in icp.__doc__ and "radians" in icp.__doc__
