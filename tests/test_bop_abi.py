"""CPU-side checks of libpvbop.so (include/pvbop.h): it builds for gfx950 from the fifth table of
pvnet_amd/build.py, exports exactly its header, stands apart from the other ten libraries and rejects
bad arguments on the host."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.test_build_table import HEADERS, exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_bop_sym_errors", "pv_bop_vsd", "pv_bop_workspace_size"]
TEN = [*HEADERS, "pvcompose.h", "pvoptim.h", "pvshade.h"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _bop_lib
    build.build()
    return _bop_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    assert list(build.BOP_LIBS) == ["bop"] and list(build.NEXT_LIBS) == ["shade"] and len(build.LIBS) == 7
    ten = [lib_.out for lib_ in build.all_libs()]
    bop = build.BOP_LIBS["bop"]
    assert len(set(ten)) == 10 and [lib_.out for lib_ in build.every_lib()] == [*ten, bop.out] and bop.out not in ten
    assert isinstance(bop, build.Lib)
    assert bop.out == os.path.join(REPO, "pvnet_amd", "libpvbop.so")
    assert bop.hdr == os.path.join(REPO, "include", "pvbop.h")
    assert [os.path.basename(s) for s in bop.srcs] == ["pvbop.hip"]
    assert b"gfx950" in open(bop.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    assert all(os.path.exists(lib_.out) for lib_ in build.every_lib())
    src = open(bop.srcs[0]).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../../include/pvbop.h"]
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    # no fast-math form, no fused multiply-add, no matrix instruction, no floating-point atomic, no inline assembly
    assert not re.search(r"__fdividef|__fsqrt|__frsqrt|rsqrtf?\s*\(|\bfmaf?\s*\(|mfma_|atomic\w*\(\s*\(?(float|double)|\basm\b", src)
    assert set(re.findall(r"\batomic\w+", src)) == {"atomicAdd"} and src.count("atomicAdd(") == 1
    assert "atomicAdd((unsigned long long *)(a.counts" in src                        # the one integer count
    hdr = open(bop.hdr).read()
    for name in ("pveval.h", "pvrender.h", "tests/bop_ref.py", "hipGraph", "MSSD", "MSPD", "VSD", "bit for bit", "lowest s"):
        assert name in hdr, name
    assert '#include "' not in hdr


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _bop_lib
    assert header_functions("pvbop.h") == NAMES
    assert exported(build.BOP_LIBS["bop"].out) == set(NAMES)
    assert {n for n, _, _ in _bop_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_bop_lib.py"
    # the pinned library of the 2018 protocol gained nothing
    assert exported(build.LIBS["eval"].out) == {"pv_nearest_point_idx", "pv_eval_workspace_size", "pv_pose_metrics"}


def test_closure_and_staleness(lib, monkeypatch):
    from pvnet_amd import build
    bop = build.BOP_LIBS["bop"]
    got = build.closure(bop.srcs)
    assert set(got) == {*bop.srcs, bop.hdr} and len(got) == 2
    mm = subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "--cuda-host-only", "-MM", *bop.srcs],
                        capture_output=True, text=True, check=True).stdout
    read = {os.path.realpath(w) for w in mm.replace("\\\n", " ").split() if not w.endswith(":")}
    root = os.path.realpath(REPO) + os.sep
    assert {p for p in read if p.startswith(root)} == {os.path.realpath(p) for p in got}
    ten = [set(build.closure(lib_.srcs)) for lib_ in build.all_libs()]
    assert len(ten) == 10
    for lib_, files in zip(build.all_libs(), ten):
        assert not files & set(got), lib_.out
    # which edit makes which library stale: modification times simulated, no file touched
    outs = [lib_.out for lib_ in build.every_lib()]
    assert outs[-1] == bop.out and len(outs) == 11
    real = os.path.getmtime
    newest = max(real(p) for p in outs) + 10

    def stale_after(paths):
        monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p in paths else real(p))
        return tuple(build.stale(o) for o in outs)

    F, T = False, True
    assert stale_after(set()) == (F,) * 11
    assert stale_after({bop.hdr}) == stale_after(set(bop.srcs)) == stale_after(set(got)) == (F,) * 10 + (T,)
    assert stale_after({build.__file__}) == (T,) * 11
    assert stale_after(set().union(*ten)) == (T,) * 10 + (F,)
    ev = build.LIBS["eval"]
    assert stale_after({ev.hdr, *ev.srcs}) == tuple(o == ev.out for o in outs)
    for name in ("_bop_lib.py", "bop.py", "evaluation_utils.py", "__init__.py"):
        assert stale_after({os.path.join(REPO, "pvnet_amd", name)}) == (F,) * 11
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p == bop.hdr else real(p))
    assert build.needs_build()
    monkeypatch.undo()
    assert not build.needs_build()
    with pytest.raises(ValueError, match="BOP_LIBS"):
        build.stale(os.path.join(REPO, "pvnet_amd", "libpvnothing.so"))


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_first_and_last_among_the_eleven(tmp_path, lang):
    from pvnet_amd import build
    if lang == "c":
        cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c"]) + ["-std=c99", "-pedantic-errors"]
    else:
        cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c++"]) + ["-std=c++17"]
    assert len(TEN) == 10 and all(os.path.exists(os.path.join(REPO, "include", h)) for h in TEN)
    orders = [["pvbop.h"], ["pvbop.h", *TEN], [*TEN, "pvbop.h"], ["pvbop.h", *TEN[::-1]], [*TEN[::-1], "pvbop.h"]]
    for i, order in enumerate(orders):
        src = tmp_path / f"order{i}.{'c' if lang == 'c' else 'cpp'}"
        src.write_text("".join(f'#include "{h}"\n' for h in order) +
                       "int pv_order_probe(pv_stream_t s, const pv_bop_batch *m, const pv_bop_vsd_batch *v);\n"
                       "int pv_order_probe(pv_stream_t s, const pv_bop_batch *m, const pv_bop_vsd_batch *v) "
                       "{ return s ? PV_OK : PV_EINVAL + PV_EWORKSPACE + PV_EALIGN + m->nmodels + v->ntau + "
                       "(int)PV_BOP_ALL + PV_BOP_NCOL + PV_BOP_MAX_TAUS; }\n")
        r = subprocess.run([*cc, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (order, r.stderr)


def test_header_constants_and_structures_match_binding():
    from pvnet_amd import _bop_lib as P
    src = open(os.path.join(REPO, "include", "pvbop.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)u?\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    for name in ("PV_BOP_MSSD", "PV_BOP_MSPD", "PV_BOP_ALL", "PV_BOP_COL_MSSD", "PV_BOP_COL_MSPD", "PV_BOP_NCOL",
                 "PV_BOP_MAX_ENTRY_EXP", "PV_BOP_MAX_TAUS", "PV_BOP_MAX_DIM"):
        assert defs[name] == getattr(P, name), name
    assert P.METRICS == {"mssd": (1, 0), "mspd": (2, 1)}
    B, V = P.BopBatch, P.VsdBatch
    assert ctypes.sizeof(B) == 8 * 4 + 9 * 8 == 104
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96]
    assert ctypes.sizeof(V) == 6 * 4 + 8 * 8 == 88
    assert [getattr(V, f).offset for f, _ in V._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80]
    for struct, cls in (("pv_bop_batch", B), ("pv_bop_vsd_batch", V)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\b([A-Za-z_0-9]+)\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in cls._fields_], struct


def test_workspace_size(lib):
    f = lib.pv_bop_workspace_size
    assert f(0, 8, 1) == 0 and f(1, 0, 1) == 0 and f(1, 8, 0) == 0 and f(-1, 8, 1) == 0
    assert f(1, 1, 1) == 256                                             # one chunk, one symmetry, two columns
    for b, pn, ns in ((1, 1024, 1), (3, 1025, 33), (256, 8192, 315), (1000, 10000, 315)):
        got = f(b, pn, ns)
        chunks = -(-pn // 1024)
        assert got % 256 == 0 and 0 <= got - b * chunks * ns * 16 < 256


def test_argument_errors_without_device(lib):
    from pvnet_amd import _bop_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    nan, inf = float("nan"), float("inf")
    E, EW, EA = P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN
    need = lib.pv_bop_workspace_size(2, 100, 3)

    def sym(null=False, err=p, best=p, ws=p, nbytes=need, **kw):
        bt = dict(b=2, total=100, total_s=3, nmodels=1, max_pn=100, max_ns=3, metrics=P.PV_BOP_ALL, reserved_=0,
                  pose_est=p, pose_gt=p, model=p, model_off=p, model_id=None, syms=p, sym_off=p, K=p, K_stride=0)
        bt.update(kw)
        B = P.BopBatch(**bt)
        return lib.pv_bop_sym_errors(None if null else ctypes.byref(B), err, best, ws, nbytes, None)

    # a complete call is only stopped by its workspace, so no pointer is touched in any of this
    assert sym(ws=None) == EW and sym(nbytes=need - 1) == EW and sym(nbytes=0) == EW
    assert sym(null=True) == E
    for kw in (dict(b=-1), dict(total=-1), dict(total_s=-1), dict(max_pn=-1), dict(max_ns=-1), dict(K_stride=-1),
               dict(nmodels=0), dict(nmodels=-1), dict(metrics=4), dict(metrics=7), dict(metrics=2 ** 31),
               dict(pose_est=None), dict(pose_gt=None), dict(model_off=None), dict(sym_off=None), dict(model=None),
               dict(syms=None), dict(K=None), dict(b=2 ** 31 - 1, max_pn=2 ** 31 - 1)):
        assert sym(ws=None, **kw) == E, kw
    assert sym(err=None, ws=None) == E and sym(best=None, ws=None) == E
    # what is not read may be NULL: K without MSPD, the tables when they have no rows
    assert sym(K=None, metrics=P.PV_BOP_MSSD, ws=None) == EW
    assert sym(model=None, total=0, ws=None) == EW and sym(syms=None, total_s=0, ws=None) == EW
    assert sym(model_id=p, ws=None) == EW
    for kw in (dict(pose_est=260), dict(pose_gt=260), dict(syms=260), dict(K=260)):
        assert sym(**kw) == EA, kw
    assert sym(err=260) == EA and sym(ws=260) == EA and sym(best=258) == EA
    # nothing to do: success, whatever the pointers
    assert sym(b=0, err=None, best=None, ws=None, nbytes=0, pose_est=None) == 0
    assert sym(metrics=0, err=None, best=None, ws=None, nbytes=0, pose_est=None) == 0

    def vsd(null=False, counts=p, err=p, **kw):
        bt = dict(b=2, n_img=2, H=16, W=16, ntau=10, reserved_=0, depth_test=p, img_id=None, depth_est=p, depth_gt=p, K=p,
                  K_stride=0, delta=15.0, taus=p)
        bt.update(kw)
        V = P.VsdBatch(**bt)
        return lib.pv_bop_vsd(None if null else ctypes.byref(V), counts, err, None)

    # a complete call has no workspace to stop it: a misaligned pointer is the last check, after every other
    assert vsd(taus=260) == EA
    assert vsd(null=True) == E
    for kw in (dict(b=-1), dict(n_img=-1), dict(K_stride=-1), dict(H=0), dict(W=0), dict(H=2 ** 20 + 1), dict(W=2 ** 20 + 1),
               dict(ntau=0), dict(ntau=33), dict(ntau=-1), dict(delta=-1.0), dict(delta=nan), dict(delta=inf),
               dict(depth_est=None), dict(depth_gt=None), dict(K=None), dict(taus=None), dict(depth_test=None),
               dict(b=2 ** 22, H=2 ** 20, W=2 ** 20)):
        assert vsd(counts=260, **kw) == E, kw
    assert vsd(counts=None, taus=260) == E and vsd(err=None, taus=260) == E
    assert vsd(depth_test=None, n_img=0, taus=260) == EA                     # no images: no map to read
    for kw in (dict(K=260), dict(depth_test=258), dict(depth_est=257), dict(depth_gt=258), dict(img_id=258)):
        assert vsd(**kw) == EA, kw
    assert vsd(counts=260) == EA and vsd(err=260) == EA
    assert vsd(b=0, counts=None, err=None, depth_est=None, taus=None) == 0


def test_python_layer_rejects_before_any_call():
    import numpy as np
    import torch
    import pvnet_amd
    from pvnet_amd import bop
    from pvnet_amd.evaluation_utils import Evaluator, ModelTable
    assert pvnet_amd.SymmetryTable is bop.SymmetryTable and pvnet_amd.sym_errors is bop.sym_errors
    assert pvnet_amd.vsd is bop.vsd and pvnet_amd.average_recall is bop.average_recall
    assert {"SymmetryTable", "sym_errors", "vsd", "average_recall"} <= set(pvnet_amd.__all__)
    table = ModelTable([(np.zeros((4, 3)), 0.1, False)], device="cpu")
    syms = bop.SymmetryTable.identity(1, device="cpu")
    poses = torch.zeros((2, 3, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device"):
        bop.sym_errors(poses, poses, table, syms, np.eye(3))                  # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="device"):
        bop.vsd(torch.zeros((2, 4, 4)), poses, poses, None, np.eye(3), None, 0.1)
    with pytest.raises(RuntimeError, match="device"):
        bop.vsd_maps(torch.zeros((2, 4, 4)), torch.zeros((2, 4, 4)), torch.zeros((2, 4, 4)), np.eye(3), torch.zeros((2, 1)), 15.0)
    with pytest.raises(RuntimeError, match="device"):
        Evaluator(table, np.zeros((1, 9, 3))).bop_errors(poses, poses, syms, np.eye(3))
    assert len(bop.FRACTIONS) == 10 and abs(bop.FRACTIONS[-1] - 0.5) < 1e-15 and bop.MSPD_PIXELS[0] == 5.0
    # recall and average_recall are plain torch: NaN is a miss, thresholds are strict
    err = torch.tensor([0.04, 0.05, float("nan"), 0.6], dtype=torch.float64)
    assert float(bop.recall(err, [0.05, 0.5])) == (1 + 2 + 0 + 0) / 8
    assert float(bop.recall(err, torch.tensor([[0.05], [0.06], [1.0], [0.6]], dtype=torch.float64))) == 2 / 4
    ar = bop.average_recall(torch.tensor([0.004, 0.2]), torch.tensor([4.0, float("nan")]),
                            torch.tensor([[0.0, 0.31], [1.0, 1.0]]), torch.tensor([0.1, 0.1]), 640)
    assert ar["ar_mssd"] == 10 / 20 and ar["ar_mspd"] == 10 / 20 and ar["ar_vsd"] == (10 + 4) / 40
    assert ar["ar"] == (ar["ar_vsd"] + ar["ar_mssd"] + ar["ar_mspd"]) / 3
    assert bop.average_recall(torch.tensor([0.004]), torch.tensor([9.0]), torch.zeros((1, 1)), [0.1], 1280)["ar_mspd"] == 1.0
