"""CPU-side checks of libpvoptim.so (include/pvoptim.h): it builds for gfx950 from the third table of
pvnet_amd/build.py, exports exactly its header, stands apart from the other eight libraries, plans its
chunks on the host and rejects bad arguments there."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.test_build_table import HEADERS, exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_optim_plan", "pv_optim_step", "pv_optim_workspace_size"]
EIGHT = [*HEADERS, "pvcompose.h"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _optim_lib
    build.build()
    return _optim_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    assert list(build.LATER_LIBS) == ["optim"] and len(build.LIBS) == 7 and list(build.MORE_LIBS) == ["compose"]
    assert [lib_.out for lib_ in build.libs()] == [lib_.out for t in (build.LIBS, build.MORE_LIBS, build.LATER_LIBS) for lib_ in t.values()]
    assert len({lib_.out for lib_ in build.libs()}) == 9
    opt = build.LATER_LIBS["optim"]
    assert isinstance(opt, build.Lib)
    assert opt.out == os.path.join(REPO, "pvnet_amd", "libpvoptim.so")
    assert opt.hdr == os.path.join(REPO, "include", "pvoptim.h")
    assert [os.path.basename(s) for s in opt.srcs] == ["pvoptim.hip"]
    assert b"gfx950" in open(opt.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    src = open(opt.srcs[0]).read()
    assert [i for i in re.findall(r'#include "([^"]+)"', src)] == ["../../include/pvoptim.h"]
    for flag in ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"):
        assert flag in build.HIPCC_FLAGS
    # no fast-math form, no fused multiply-add, no floating-point atomic
    assert not re.search(r"__fdividef|__fsqrt|__frsqrt|rsqrtf?\s*\(|\bfmaf?\s*\(|atomicAdd\(\s*\(?(float|double)", src)
    hdr = open(opt.hdr).read()
    for name in ("clip_grad_norm_", "_amp_update_scale_", "torch.optim.Adam", "AdamW", "SGD", "tests/optim_ref.py", "hipGraph"):
        assert name in hdr, name
    # pvloss.h sends the caller of an f16 gradient to loss scaling: this library is that
    assert "scales the loss" in open(os.path.join(REPO, "include", "pvloss.h")).read()


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _optim_lib
    assert header_functions("pvoptim.h") == NAMES
    assert exported(build.LATER_LIBS["optim"].out) == set(NAMES)
    assert {n for n, _, _ in _optim_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_optim_lib.py"


def test_closure_and_staleness(lib, monkeypatch):
    from pvnet_amd import build
    opt = build.LATER_LIBS["optim"]
    got = build.closure(opt.srcs)
    assert set(got) == {*opt.srcs, opt.hdr} and len(got) == 2
    mm = subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "--cuda-host-only", "-MM", *opt.srcs],
                        capture_output=True, text=True, check=True).stdout
    read = {os.path.realpath(w) for w in mm.replace("\\\n", " ").split() if not w.endswith(":")}
    root = os.path.realpath(REPO) + os.sep
    assert {p for p in read if p.startswith(root)} == {os.path.realpath(p) for p in got}
    eight = {k: set(build.closure(lib_.srcs)) for k, lib_ in (*build.LIBS.items(), *build.MORE_LIBS.items())}
    for k, files in eight.items():
        assert not files & set(got), k
    # which edit makes which library stale: modification times simulated, no file touched
    outs = [lib_.out for lib_ in build.libs()]
    assert outs[-1] == opt.out
    real = os.path.getmtime
    newest = max(real(p) for p in outs) + 10

    def stale_after(paths):
        monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p in paths else real(p))
        return tuple(build.stale(o) for o in outs)

    F, T = False, True
    assert stale_after(set()) == (F,) * 9
    assert stale_after({opt.hdr}) == stale_after(set(opt.srcs)) == stale_after(set(got)) == (F,) * 8 + (T,)
    assert stale_after({build.__file__}) == (T,) * 9
    assert stale_after(set().union(*eight.values())) == (T,) * 8 + (F,)
    for name in ("_optim_lib.py", "optim.py", "__init__.py"):
        assert stale_after({os.path.join(REPO, "pvnet_amd", name)}) == (F,) * 9
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p == opt.hdr else real(p))
    assert build.needs_build()
    monkeypatch.undo()
    assert not build.needs_build()
    with pytest.raises(ValueError, match="LIBS"):
        build.stale(os.path.join(REPO, "pvnet_amd", "libpvnothing.so"))


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_in_every_order_with_the_eight(tmp_path, lang):
    from pvnet_amd import build
    if lang == "c":
        cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c"]) + ["-std=c99", "-pedantic-errors"]
    else:
        cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c++"]) + ["-std=c++17"]
    # alone, and at every position among the other eight, which also come in reverse
    orders = [["pvoptim.h"]]
    for base in (EIGHT, EIGHT[::-1]):
        orders += [[*base[:i], "pvoptim.h", *base[i:]] for i in range(len(base) + 1)]
    assert len(orders) == 19
    for i, order in enumerate(orders):
        src = tmp_path / f"order{i}.{'c' if lang == 'c' else 'cpp'}"
        src.write_text("".join(f'#include "{h}"\n' for h in order) +
                       "int pv_order_probe(pv_stream_t s, const pv_optim_desc *d, const pv_optim_tensor *t);\n"
                       "int pv_order_probe(pv_stream_t s, const pv_optim_desc *d, const pv_optim_tensor *t) "
                       "{ return s ? PV_OK : PV_EINVAL + PV_EWORKSPACE + PV_EALIGN + d->algorithm + (int)t->n + PV_OPT_CHUNK; }\n")
        r = subprocess.run([*cc, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (order, r.stderr)


def test_header_constants_match_binding():
    from pvnet_amd import _optim_lib as P, _loss_lib
    from tests import optim_ref as R
    src = open(os.path.join(REPO, "include", "pvoptim.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    assert (defs["PV_OPT_F32"], defs["PV_OPT_F16"]) == (P.PV_OPT_F32, P.PV_OPT_F16) == (_loss_lib.PV_LOSS_F32, _loss_lib.PV_LOSS_F16)
    assert (defs["PV_OPT_ADAM"], defs["PV_OPT_ADAMW"], defs["PV_OPT_SGD"]) == (P.PV_OPT_ADAM, P.PV_OPT_ADAMW, P.PV_OPT_SGD) == \
        (R.ADAM, R.ADAMW, R.SGD) == (0, 1, 2)
    assert defs["PV_OPT_CHUNK"] == P.PV_OPT_CHUNK == R.CHUNK == 8192 and R.CHUNK & (R.CHUNK - 1) == 0
    assert defs["PV_OPT_THREADS"] == P.PV_OPT_THREADS == R.THREADS == 256
    assert defs["PV_OPT_GROUP"] == P.PV_OPT_GROUP == R.GROUP == 8 and R.CHUNK % (R.THREADS * R.GROUP) == 0
    # the structures are the header's
    T, C, S, D = P.OptTensor, P.OptChunk, P.OptState, P.OptDesc
    assert ctypes.sizeof(T) == 5 * 8 + 8 + 2 * 4 == 56
    assert [getattr(T, f).offset for f in ("master", "model", "grad", "m", "v", "n", "grad_kind", "pad_")] == [0, 8, 16, 24, 32, 40, 48, 52]
    assert ctypes.sizeof(C) == 16 and [getattr(C, f).offset for f in ("first", "tensor", "pad_")] == [0, 8, 12]
    assert ctypes.sizeof(S) == 48
    assert [getattr(S, f).offset for f in ("b1pow", "b2pow", "step", "lr", "scale", "growth_tracker", "grad_norm", "found_inf",
                                           "skipped")] == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    assert ctypes.sizeof(D) == 48
    assert [getattr(D, f).offset for f in ("algorithm", "beta1", "beta2", "eps", "weight_decay", "momentum", "max_norm",
                                           "growth_factor", "backoff_factor", "growth_interval", "zero_grads", "pad_")] == \
        list(range(0, 48, 4))
    # each field of each structure is in the header, in this order
    for struct, cls in (("pv_optim_tensor", T), ("pv_optim_chunk", C), ("pv_optim_state", S), ("pv_optim_desc", D)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\b([A-Za-z_0-9]+)\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in cls._fields_], struct


def test_plan(lib):
    from pvnet_amd import _optim_lib as P
    from tests import optim_ref as R
    C = P.PV_OPT_CHUNK

    def tensors(ns, **kw):
        tab = (P.OptTensor * max(len(ns), 1))()
        for i, n in enumerate(ns):
            d = dict(master=256, model=512, grad=1024, m=2048, v=4096, n=n, grad_kind=P.PV_OPT_F16)
            d.update({k: v for k, v in kw.items() if not isinstance(v, dict)})
            d.update(kw.get(f"t{i}", {}))
            tab[i] = P.OptTensor(**d)
        return tab

    def plan(ns, alg=P.PV_OPT_ADAM, cap=None, **kw):
        tab = tensors(ns, **kw)
        n = lib.pv_optim_plan(tab, len(ns), alg, None, 0)
        if n < 0:
            return n
        cap = n if cap is None else cap
        out = (P.OptChunk * (max(cap, 0) + 2))()
        for c in out:
            c.first, c.tensor, c.pad_ = -7, -7, -7
        assert lib.pv_optim_plan(tab, len(ns), alg, out, cap) == n
        got = [(c.tensor, c.first) for c in out]
        assert got[min(cap, n):] == [(-7, -7)] * (len(out) - min(cap, n))          # nothing past the capacity or the count
        assert all(c.pad_ == 0 for c in out[:min(cap, n)])
        return got[:min(cap, n)]

    sizes = [0, 1, C - 1, C, C + 1, 0, 3 * C + 5, 7, 2 * C]
    assert plan(sizes) == R.plan(sizes) and len(R.plan(sizes)) == 12
    assert plan(sizes, cap=5) == R.plan(sizes)[:5] and plan(sizes, cap=0) == []
    for ns in ([], [0], [0, 0], [1], [C - 1], [C], [C + 1], [2 ** 40 // 1024]):
        assert plan(ns) == R.plan(ns), ns
    # the order is a function of the n's alone: pointers, kinds and the algorithm do not enter
    assert plan(sizes, alg=P.PV_OPT_SGD, v=None, model=None, grad_kind=P.PV_OPT_F32, master=4) == R.plan(sizes)
    # bad tensors
    E = P.PV_EINVAL
    assert lib.pv_optim_plan(None, 1, 0, None, 0) == E and lib.pv_optim_plan(tensors([1]), -1, 0, None, 0) == E
    assert lib.pv_optim_plan(tensors([1]), 1, 3, None, 0) == E and lib.pv_optim_plan(tensors([1]), 1, -1, None, 0) == E
    assert lib.pv_optim_plan(tensors([1]), 1, 0, None, 1) == E and lib.pv_optim_plan(tensors([1]), 1, 0, None, -1) == E
    assert lib.pv_optim_plan(None, 0, 0, None, 0) == 0
    assert plan([5, -1]) == E and plan([5, 5], t1=dict(grad_kind=2)) == E and plan([5], grad_kind=-1) == E
    for name in ("master", "grad", "m", "v"):
        assert plan([5, 5, 5], t2={name: None}) == E, name
        assert plan([0, 5], t0={name: None}) == [(1, 0)], name         # a tensor without elements may have no address
    assert plan([5], alg=P.PV_OPT_SGD, v=None) == [(0, 0)] and plan([5], alg=P.PV_OPT_ADAMW, v=None) == E
    assert plan([5], model=None) == [(0, 0)]
    for kw in (dict(master=258), dict(m=257), dict(v=4098), dict(model=513), dict(grad=1025),
               dict(grad=1026, grad_kind=P.PV_OPT_F32)):
        assert plan([5], **kw) == P.PV_EALIGN, kw
    assert plan([5], grad=1026) == [(0, 0)]                            # an f16 gradient at an even address
    # more chunks than a grid holds
    assert plan([C * (2 ** 31 - 1)], cap=0) == [] and lib.pv_optim_plan(tensors([C * (2 ** 31 - 1)]), 1, 0, None, 0) == 2 ** 31 - 1
    assert plan([C * (2 ** 31 - 1), 1]) == E and plan([2 ** 62]) == E


def test_workspace_size(lib):
    f = lib.pv_optim_workspace_size
    assert f(-1) == 0 and f(2 ** 31) == 0 and f(2 ** 40) == 0
    assert f(0) == 256                                                  # the decision record alone
    assert f(1) == 3 * 256 and f(32) == 3 * 256 and f(33) == 4 * 256 and f(64) == 4 * 256 and f(65) == 6 * 256
    assert all(f(n) % 256 == 0 and f(n) >= 12 * n + 24 for n in (1, 100, 1601, 2 ** 20, 2 ** 31 - 1))
    assert f(2000) < 32 * 1024                                          # a 13 M parameter network: a few KiB


def test_argument_errors_without_device(lib):
    from pvnet_amd import _optim_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    nan, inf = float("nan"), float("inf")
    need = lib.pv_optim_workspace_size(5)

    def desc(**kw):
        d = dict(algorithm=P.PV_OPT_ADAM, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, momentum=0.9, max_norm=1.0,
                 growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, zero_grads=1)
        d.update(kw)
        return P.OptDesc(**d)

    def step(d=None, null=False, table=p, n_tensors=3, chunks=p, n_chunks=5, state=p, ws=p, nbytes=need):
        d = d or desc()
        return lib.pv_optim_step(None if null else ctypes.byref(d), table, n_tensors, chunks, n_chunks, state, ws, nbytes, None)

    assert step(null=True) == P.PV_EINVAL
    for kw in (dict(algorithm=3), dict(algorithm=-1),
               dict(beta1=-0.1), dict(beta1=1.0), dict(beta1=1.5), dict(beta1=nan), dict(beta1=inf),
               dict(beta2=-0.1), dict(beta2=1.0), dict(beta2=nan), dict(beta2=-inf),
               dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf),
               dict(weight_decay=-0.1), dict(weight_decay=nan), dict(weight_decay=inf),
               dict(momentum=-0.5), dict(momentum=nan), dict(momentum=inf),
               dict(max_norm=nan), dict(max_norm=-inf),
               dict(growth_factor=0.5), dict(growth_factor=nan), dict(growth_factor=inf),
               dict(backoff_factor=0.0), dict(backoff_factor=-0.5), dict(backoff_factor=1.5), dict(backoff_factor=nan),
               dict(growth_interval=-1), dict(zero_grads=2), dict(zero_grads=-1)):
        for alg in (P.PV_OPT_ADAM, P.PV_OPT_ADAMW, P.PV_OPT_SGD):
            assert step(desc(**{"algorithm": alg, **kw})) == P.PV_EINVAL, (alg, kw)
        assert step(desc(**kw), n_chunks=0) == P.PV_EINVAL, kw          # an empty table does not excuse them
    # values at the edges that are allowed: rejected for the workspace, so no pointer is touched
    for kw in (dict(beta1=0.0, beta2=0.0), dict(weight_decay=0.0, momentum=0.0), dict(max_norm=0.0), dict(max_norm=-1.0),
               dict(max_norm=inf), dict(growth_factor=1.0, backoff_factor=1.0), dict(growth_interval=0), dict(zero_grads=0)):
        assert step(desc(**kw), ws=None) == P.PV_EWORKSPACE, kw
    # counts and pointers
    assert step(n_tensors=-1) == P.PV_EINVAL and step(n_chunks=-1) == P.PV_EINVAL and step(n_chunks=2 ** 31) == P.PV_EINVAL
    assert step(table=None) == P.PV_EINVAL and step(chunks=None) == P.PV_EINVAL and step(state=None) == P.PV_EINVAL
    # the workspace: missing, short by one byte, misaligned
    assert step(ws=None) == P.PV_EWORKSPACE and step(nbytes=need - 1) == P.PV_EWORKSPACE and step(nbytes=0) == P.PV_EWORKSPACE
    assert step(ws=264) == P.PV_EALIGN
    # a misaligned table, chunk list or state
    assert step(table=260) == P.PV_EALIGN and step(chunks=258) == P.PV_EALIGN and step(state=260) == P.PV_EALIGN
    # nothing to do: success, no launch, whatever the pointers
    assert step(n_tensors=0) == 0 and step(n_chunks=0) == 0
    assert step(n_tensors=0, n_chunks=0, table=None, chunks=None, state=None, ws=None, nbytes=0) == 0
    assert step(n_chunks=0, table=None, chunks=None, state=None, ws=None, nbytes=0) == 0


def test_python_layer_rejects_before_any_call():
    import torch
    import pvnet_amd
    from pvnet_amd import optim as O
    assert pvnet_amd.Optimizer is O.Optimizer and "Optimizer" in pvnet_amd.__all__
    w = torch.nn.Parameter(torch.zeros(4, 3))
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="device"):
        O.Optimizer([w])
    with pytest.raises(RuntimeError, match="device"):
        O.Optimizer([("conv.weight", w)], "sgd", lr=0.1, momentum=0.9)
    # wrong arguments, before the device is looked at
    with pytest.raises(RuntimeError, match="algorithm"):
        O.Optimizer([w], "adagrad")
    with pytest.raises(RuntimeError, match="empty"):
        O.Optimizer([])
    assert set(O.ALGORITHMS) == {"adam", "adamw", "sgd"}
    for name in ("scale_loss", "step", "zero_grad", "set_lr", "stats", "state_dict", "load_state_dict"):
        assert callable(getattr(O.Optimizer, name)), name
