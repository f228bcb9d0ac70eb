"""What is about all seven HIP libraries at once (CPU only): the table pvnet_amd/build.py builds from,
the dependency list it derives from the sources, which edit makes which library stale, that the
public headers can be included together in any order, and the loader every binding shares."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pvnet_amd", "csrc")
# key -> (library, public header, translation units), in build order
TABLE = {
    "vote": ("libpvvote.so", "pvvote.h", ["pvvote.hip", "pvapi.hip", "pvpipeline.hip", "pvcompact.hip", "pvrefine.hip",
                                          "pvevd.hip", "pvpnp.hip", "pvdecoder.hip", "pvconv.hip"]),
    "eval": ("libpveval.so", "pveval.h", ["pveval.hip"]),
    "pose": ("libpvpose.so", "pvpose.h", ["pvepnp.hip"]),
    "render": ("libpvrender.so", "pvrender.h", ["pvrender.hip"]),
    "model": ("libpvmodel.so", "pvmodel.h", ["pvmodel.hip"]),
    "loss": ("libpvloss.so", "pvloss.h", ["pvloss.hip"]),
    "augment": ("libpvaugment.so", "pvaugment.h", ["pvaugment.hip"]),
}
# the headers pveval.hip shares with the vote library's translation units
SHARED = {os.path.join(REPO, "include", "pvvote.h"),
          *(os.path.join(CSRC, n) for n in ("pv_common.h", "pv_host.h", "pv_tunables.h", "pv_rng.h", "pv_hypclass.h"))}


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pv_[A-Za-z0-9_]+)\s*\(", src)))


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    return {n for n in names if not re.fullmatch(r"__hip_cuid_[0-9a-f]+", n)}


@pytest.fixture(scope="module")
def build():
    from pvnet_amd import build
    build.build()
    return build


@pytest.fixture(scope="module")
def deps(build):
    return {k: set(build.closure(lib.srcs)) for k, lib in build.LIBS.items()}


def test_table():
    from pvnet_amd import build
    assert list(build.LIBS) == list(TABLE)
    for key, (out, hdr, srcs) in TABLE.items():
        lib = build.LIBS[key]
        assert lib.out == os.path.join(REPO, "pvnet_amd", out)
        assert lib.hdr == os.path.join(REPO, "include", hdr)
        assert list(lib.srcs) == [os.path.join(CSRC, s) for s in srcs]
    for name in ("SRCS", "HDR", "OUT", "EVAL_OUT", "POSE_DEPS", "AUG_SRCS"):      # no alias layer
        assert not hasattr(build, name)
    pose = build.LIBS["pose"]
    assert set(build.closure(pose.srcs)) == {*pose.srcs, os.path.join(CSRC, "pvepnp_core.h"), pose.hdr}


@pytest.mark.parametrize("key", list(TABLE))
def test_closure_is_what_the_compiler_reads(build, key):
    lib = build.LIBS[key]
    mm = subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "--cuda-host-only", "-MM", *lib.srcs],
                        capture_output=True, text=True, check=True).stdout
    # make rules, "target: dep dep \<newline> dep": everything but the targets and the continuations
    read = {os.path.realpath(w) for w in mm.replace("\\\n", " ").split() if not w.endswith(":")}
    root = os.path.realpath(REPO) + os.sep
    assert {p for p in read if p.startswith(root)} == {os.path.realpath(p) for p in build.closure(lib.srcs)}
    # one file is one string: normalised, absolute, no duplicates, and the library's own header among them
    got = build.closure(lib.srcs)
    assert got == [os.path.normpath(p) for p in got] and all(os.path.isabs(p) for p in got)
    assert len(set(got)) == len(got) and lib.hdr in got


def test_staleness_matrix(build, deps, monkeypatch):
    """Which edit makes which library stale.  An edit is simulated by the modification times stale()
    sees; no file is touched."""
    L = build.LIBS
    outs = [lib.out for lib in L.values()]
    real = os.path.getmtime
    newest = max(real(p) for p in outs) + 10

    def stale_after(paths):
        monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p in paths else real(p))
        return tuple(build.stale(o) for o in outs)

    F, T = False, True
    # the files each library calls its own: the vote and the eval library share headers of csrc/
    own = {**deps, "vote": {*L["vote"].srcs, L["vote"].hdr}, "eval": {*L["eval"].srcs, L["eval"].hdr}}
    for i, k in list(enumerate(L))[2:]:
        assert stale_after({L[k].hdr}) == stale_after(set(L[k].srcs)) == tuple(j == i for j in range(7)), k
        # every library before this one edited: this one and the later ones stay
        assert stale_after(set().union(*(own[j] for j in list(L)[:i]))) == tuple(j < i for j in range(7)), k
    assert stale_after(set().union(*(own[k] for k in L if k != "augment"))) == (T, T, T, T, T, T, F)
    assert stale_after(deps["augment"]) == (F, F, F, F, F, F, T)
    assert stale_after(deps["loss"]) == (F, F, F, F, F, T, F)
    assert stale_after(deps["model"]) == (F, F, F, F, T, F, F)
    assert stale_after(deps["render"]) == (F, F, F, T, F, F, F)
    assert stale_after(deps["pose"]) == (F, F, T, F, F, F, F)
    assert stale_after({os.path.join(CSRC, "pvepnp_core.h")}) == (F, F, T, F, F, F, F)
    assert stale_after(own["eval"]) == (F, T, F, F, F, F, F)
    assert stale_after(set(L["vote"].srcs)) == (T, F, F, F, F, F, F)
    assert stale_after({*L["vote"].srcs, *own["eval"]}) == (T, T, F, F, F, F, F)
    # the headers the vote library's translation units and pveval.hip share
    assert stale_after({os.path.join(CSRC, "pv_common.h"), os.path.join(CSRC, "pv_host.h")}) == (T, T, F, F, F, F, F)
    assert stale_after({L["vote"].hdr}) == (T, T, F, F, F, F, F)
    assert stale_after({build.__file__}) == (T, T, T, T, T, T, T)
    monkeypatch.undo()
    # a path that is no library's has no rule: stale() does not guess one
    with pytest.raises(ValueError, match="LIBS"):
        build.stale(os.path.join(CSRC, "pvvote.gfx950.s"))
    assert build.older(os.path.join(CSRC, "no_such.gfx950.s"), ()) and not build.older(outs[0], ())
    assert not build.needs_build()


def test_libraries_share_no_translation_unit(build, deps):
    for a, b in itertools.combinations(build.LIBS, 2):
        assert not set(build.LIBS[a].srcs) & set(build.LIBS[b].srcs)
        assert deps[a] & deps[b] == (SHARED if (a, b) == ("vote", "eval") else set()), (a, b)
    assert SHARED == deps["eval"] - {*build.LIBS["eval"].srcs, build.LIBS["eval"].hdr}


HEADERS = [hdr for _, hdr, _ in TABLE.values()]
ORDERS = [HEADERS, HEADERS[::-1], *([h] + [o for o in HEADERS if o != h] for h in HEADERS)]


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_headers_compile_together_in_any_order(tmp_path, lang):
    """Forward, reverse and each header first: one definition of pv_stream_t and the status codes,
    whichever header comes first."""
    from pvnet_amd import build
    if lang == "c":
        cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c"]) + ["-std=c99", "-pedantic-errors"]
    else:
        cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c++"]) + ["-std=c++17"]      # hipcc's clang compiles plain C++ too
    assert len(ORDERS) == 9 and all(sorted(o) == sorted(HEADERS) for o in ORDERS)
    for i, order in enumerate(ORDERS):
        src = tmp_path / f"order{i}.{'c' if lang == 'c' else 'cpp'}"
        src.write_text("".join(f'#include "{h}"\n' for h in order) +
                       "int pv_order_probe(pv_stream_t s);\n"
                       "int pv_order_probe(pv_stream_t s) { return s ? PV_OK : PV_EINVAL + PV_EWORKSPACE + PV_EALIGN + 6; }\n")
        r = subprocess.run([*cc, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (order, r.stderr)


def test_loader_names_a_missing_library(tmp_path):
    from pvnet_amd import _cdll
    path = str(tmp_path / "libpvnothing.so")
    load = _cdll.loader(path, [])
    for _ in range(2):      # and does not remember the failure as a library
        with pytest.raises(RuntimeError) as e:
            load()
        assert path in str(e.value) and "python -m pvnet_amd.build" in str(e.value)


def test_loader_loads_once_under_threads(build):
    from pvnet_amd import _cdll, _model_lib
    load = _cdll.loader(_model_lib.LIB_PATH, _model_lib.SIGNATURES)      # a fresh one: the first call is contended
    gate = threading.Barrier(8, timeout=60)

    def run(_):
        gate.wait()
        return load(), _model_lib.load()
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(run, range(8)))
    assert all(g[0] is got[0][0] and g[1] is got[0][1] for g in got)
    assert isinstance(got[0][0], ctypes.CDLL) and got[0][0].pv_model_workspace_size.restype is ctypes.c_size_t
    assert _model_lib.load() is got[0][1]


def test_status_check_raises_the_given_class():
    from pvnet_amd import _loss_lib as P
    assert P.check(0, "step") is None and (P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN) == (-1, -2, -3)
    for code, text in ((P.PV_EINVAL, "invalid argument"), (P.PV_EWORKSPACE, "workspace missing or too small"),
                       (P.PV_EALIGN, "pointer not aligned as documented"), (700, "HIP error")):
        with pytest.raises(P.PVLossError, match=re.escape(f"step failed: {text} (code {code})")):
            P.check(code, "step")
