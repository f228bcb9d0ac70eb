"""CPU-side checks of libpvshade.so (include/pvshade.h): it builds for gfx950 from the fourth table of
pvnet_amd/build.py, exports exactly its header, stands apart from the other nine libraries and rejects
bad arguments on the host."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.test_build_table import HEADERS, exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_shade_normals", "pv_shade_render", "pv_shade_workspace_size"]
NINE = [*HEADERS, "pvcompose.h", "pvoptim.h"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _shade_lib
    build.build()
    return _shade_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    assert list(build.NEXT_LIBS) == ["shade"] and list(build.LATER_LIBS) == ["optim"] and len(build.LIBS) == 7
    nine = [lib_.out for t in (build.LIBS, build.MORE_LIBS, build.LATER_LIBS) for lib_ in t.values()]
    assert [lib_.out for lib_ in build.libs()] == nine and len(set(nine)) == 9
    sh = build.NEXT_LIBS["shade"]
    assert [lib_.out for lib_ in build.all_libs()] == [*nine, sh.out] and len({*nine, sh.out}) == 10
    assert isinstance(sh, build.Lib)
    assert sh.out == os.path.join(REPO, "pvnet_amd", "libpvshade.so")
    assert sh.hdr == os.path.join(REPO, "include", "pvshade.h")
    assert [os.path.basename(s) for s in sh.srcs] == ["pvshade.hip"]
    assert b"gfx950" in open(sh.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    assert all(os.path.exists(lib_.out) for lib_ in build.all_libs())
    src = open(sh.srcs[0]).read()
    assert [i for i in re.findall(r'#include "([^"]+)"', src)] == ["../../include/pvshade.h"]
    for flag in ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"):
        assert flag in build.HIPCC_FLAGS
    # no fast-math form, no fused multiply-add, no floating-point atomic, no inline assembly
    assert not re.search(r"__fdividef|__fsqrt|__frsqrt|rsqrtf?\s*\(|\bfmaf?\s*\(|atomic\w*\(\s*\(?(float|double)|\basm\b", src)
    assert set(re.findall(r"\batomic\w+", src)) == {"atomicMin", "atomicAdd"}
    assert "atomicAdd(a.out.won" in src and src.count("atomicAdd(") == 1          # the one integer count
    hdr = open(sh.hdr).read()
    for name in ("pvrender.h", "tests/shade_ref.py", "hipGraph", "OUT OF SCOPE", "top-left", "Lambert", "pv_render_labels"):
        assert name in hdr, name
    assert '#include "' not in hdr


def test_rules_are_the_label_renderer_s_word_for_word():
    def rules(name, nums):
        src = open(os.path.join(REPO, "include", name)).read()
        out = {}
        for n in nums:
            m = re.search(r"\n \*  %d\. (.*?)(?=\n \*  \d\. |\*/)" % n, src, re.S)
            out[n] = " ".join(m.group(1).replace("\n *", " ").split())
        return out
    want = rules("pvrender.h", (1, 2, 3, 4, 5, 7))
    got = rules("pvshade.h", (1, 2, 3, 4, 5, 7))
    assert got == want and all(len(v) > 60 for v in want.values())


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _shade_lib
    assert header_functions("pvshade.h") == NAMES
    assert exported(build.NEXT_LIBS["shade"].out) == set(NAMES)
    assert {n for n, _, _ in _shade_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_shade_lib.py"


def test_closure_and_staleness(lib, monkeypatch):
    from pvnet_amd import build
    sh = build.NEXT_LIBS["shade"]
    got = build.closure(sh.srcs)
    assert set(got) == {*sh.srcs, sh.hdr} and len(got) == 2
    mm = subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "--cuda-host-only", "-MM", *sh.srcs],
                        capture_output=True, text=True, check=True).stdout
    read = {os.path.realpath(w) for w in mm.replace("\\\n", " ").split() if not w.endswith(":")}
    root = os.path.realpath(REPO) + os.sep
    assert {p for p in read if p.startswith(root)} == {os.path.realpath(p) for p in got}
    nine = {k: set(build.closure(lib_.srcs))
            for k, lib_ in (*build.LIBS.items(), *build.MORE_LIBS.items(), *build.LATER_LIBS.items())}
    assert len(nine) == 9
    for k, files in nine.items():
        assert not files & set(got), k
    # which edit makes which library stale: modification times simulated, no file touched
    outs = [lib_.out for lib_ in build.all_libs()]
    assert outs[-1] == sh.out and len(outs) == 10
    real = os.path.getmtime
    newest = max(real(p) for p in outs) + 10

    def stale_after(paths):
        monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p in paths else real(p))
        return tuple(build.stale(o) for o in outs)

    F, T = False, True
    assert stale_after(set()) == (F,) * 10
    assert stale_after({sh.hdr}) == stale_after(set(sh.srcs)) == stale_after(set(got)) == (F,) * 9 + (T,)
    assert stale_after({build.__file__}) == (T,) * 10
    assert stale_after(set().union(*nine.values())) == (T,) * 9 + (F,)
    render = build.LIBS["render"]
    assert stale_after({render.hdr, *render.srcs}) == tuple(o == render.out for o in outs)
    for name in ("_shade_lib.py", "shade.py", "render.py", "__init__.py"):
        assert stale_after({os.path.join(REPO, "pvnet_amd", name)}) == (F,) * 10
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p == sh.hdr else real(p))
    assert build.needs_build()
    monkeypatch.undo()
    assert not build.needs_build()
    with pytest.raises(ValueError, match="LIBS"):
        build.stale(os.path.join(REPO, "pvnet_amd", "libpvnothing.so"))


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_in_every_order_with_the_nine(tmp_path, lang):
    from pvnet_amd import build
    if lang == "c":
        cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c"]) + ["-std=c99", "-pedantic-errors"]
    else:
        cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c++"]) + ["-std=c++17"]
    # alone, and at every position among the other nine, which also come in reverse
    orders = [["pvshade.h"]]
    for base in (NINE, NINE[::-1]):
        orders += [[*base[:i], "pvshade.h", *base[i:]] for i in range(len(base) + 1)]
    assert len(orders) == 21
    for i, order in enumerate(orders):
        src = tmp_path / f"order{i}.{'c' if lang == 'c' else 'cpp'}"
        src.write_text("".join(f'#include "{h}"\n' for h in order) +
                       "int pv_order_probe(pv_stream_t s, const pv_shade_meshes *m, const pv_shade_lights *l);\n"
                       "int pv_order_probe(pv_stream_t s, const pv_shade_meshes *m, const pv_shade_lights *l) "
                       "{ return s ? PV_OK : PV_EINVAL + PV_EWORKSPACE + PV_EALIGN + m->nmodels + (int)l->bg_color[2] + "
                       "PV_LABEL_I32 + PV_SHADE_LIGHT_DOUBLES; }\n")
        r = subprocess.run([*cc, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (order, r.stderr)


def test_header_constants_and_structures_match_binding():
    from pvnet_amd import _render_lib, _shade_lib as P
    src = open(os.path.join(REPO, "include", "pvshade.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    assert (defs["PV_LABEL_I64"], defs["PV_LABEL_U8"], defs["PV_LABEL_I32"]) == (P.PV_LABEL_I64, P.PV_LABEL_U8, P.PV_LABEL_I32) == \
        (_render_lib.PV_LABEL_I64, _render_lib.PV_LABEL_U8, _render_lib.PV_LABEL_I32)
    assert defs["PV_SHADE_SUBPIXEL_BITS"] == P.PV_SHADE_SUBPIXEL_BITS == _render_lib.PV_RENDER_SUBPIXEL_BITS
    assert defs["PV_SHADE_MAX_SNAP"] == P.PV_SHADE_MAX_SNAP == _render_lib.PV_RENDER_MAX_SNAP
    assert defs["PV_SHADE_MAX_DIM"] == P.PV_SHADE_MAX_DIM == _render_lib.PV_RENDER_MAX_DIM
    assert defs["PV_SHADE_LIGHT_DOUBLES"] == P.PV_SHADE_LIGHT_DOUBLES == 9
    M, B, L, O = P.ShadeMeshes, P.ShadeBatch, P.ShadeLights, P.ShadeOut
    assert ctypes.sizeof(M) == 6 * 8 + 6 * 4 == 72
    assert [getattr(M, f).offset for f, _ in M._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68]
    assert ctypes.sizeof(B) == ctypes.sizeof(_render_lib.RenderBatch) == 80
    assert [(f, getattr(B, f).offset) for f, _ in B._fields_] == \
        [(f, getattr(_render_lib.RenderBatch, f).offset) for f, _ in _render_lib.RenderBatch._fields_]
    assert ctypes.sizeof(L) == 64
    assert [getattr(L, f).offset for f, _ in L._fields_] == [0, 8, 16, 24, 56, 59]
    assert ctypes.sizeof(O) == 80
    assert [getattr(O, f).offset for f, _ in O._fields_] == [0, 8, 40, 48, 56, 64, 72]
    # the meshes are pv_render_meshes' fields with colors and normals after the four tables
    assert [f for f, _ in M._fields_ if f not in ("colors", "normals")] == [f for f, _ in _render_lib.RenderMeshes._fields_]
    # each field of each structure is in the header, in this order
    for struct, cls in (("pv_shade_meshes", M), ("pv_shade_batch", B), ("pv_shade_lights", L), ("pv_shade_out", O)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\b([A-Za-z_0-9]+)\s*(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in cls._fields_], struct


def test_workspace_size(lib):
    from pvnet_amd import _render_lib
    f = lib.pv_shade_workspace_size
    assert f(0, 4, 4, 0, 0) == 0 and f(1, 0, 4, 0, 0) == 0 and f(1, 4, 2 ** 20 + 1, 0, 0) == 0
    assert f(1, 4, 4, -1, 0) == 0 and f(1, 4, 4, 0, -1) == 0 and f(1, 4, 4, 2 ** 40 + 1, 0) == 0
    assert f(1, 1, 1, 0, 0) == 2 * 256                                   # one key and one image base
    for b, H, W, iv, n in ((1, 1, 1, 1, 1), (3, 37, 53, 3 * 642, 3), (32, 480, 640, 256 * 10242, 256)):
        got = f(b, H, W, iv, n)
        assert got % 256 == 0 and got >= b * H * W * 8 + iv * 32 + n * 32 + b * 4
        # the label renderer's, and camera-frame X and Y per projected vertex
        assert got - _render_lib.load().pv_render_workspace_size(b, H, W, iv, n) == -(-iv * 16 // 256) * 256


def test_argument_errors_without_device(lib):
    from pvnet_amd import _shade_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    nan = float("nan")
    need = lib.pv_shade_workspace_size(2, 16, 16, 2 * 8, 2)
    E, EW, EA = P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN

    def render(null=(), ws=p, nbytes=need, **kw):
        m = dict(verts=p, vert_off=p, faces=p, face_off=p, colors=p, normals=None, nmodels=1, total_v=8, total_f=12,
                 max_verts=8, max_faces=12, reserved_=0)
        bt = dict(b=2, H=16, W=16, ninst=1, total_inst=2, label_kind=P.PV_LABEL_U8, inst_off=None, model_id=p, label=p,
                  pose=p, K=p, K_stride=0, znear=1e-3)
        lt = dict(lights=p, lights_stride=0, background=None)
        ot = dict(image=p, label=p, inst=p, depth=p, face=p, won=p)
        arrays = {}
        for k, v in kw.items():
            if k in ("bg_strides", "image_strides", "bg_color"):
                arrays[k] = v
            elif k == "inst_label":                                    # the batch's per-instance labels; `label` is the map
                bt["label"] = v
            else:
                next(d for d in (m, lt, ot, bt) if k in d)[k] = v
        M, B, L, O = P.ShadeMeshes(**m), P.ShadeBatch(**bt), P.ShadeLights(**lt), P.ShadeOut(**ot)
        for i, s in enumerate(arrays.get("image_strides", (768, 48, 3, 1))):
            O.image_strides[i] = s
        for i, s in enumerate(arrays.get("bg_strides", (0, 0, 0, 0))):
            L.bg_strides[i] = s
        args = [None if n in null else ctypes.byref(s) for n, s in (("m", M), ("bt", B), ("lt", L), ("ot", O))]
        return lib.pv_shade_render(*args, ws, nbytes, None)

    # a complete call is only stopped by its workspace, so no pointer is touched in any of this
    assert render(ws=None) == EW and render(nbytes=need - 1) == EW and render(nbytes=0) == EW
    assert render(ws=264) == EA
    for n in ("m", "bt", "lt", "ot"):
        assert render(null=(n,)) == E, n
    for kw in (dict(b=-1), dict(ninst=-1), dict(total_inst=-1), dict(K_stride=-1), dict(H=0), dict(W=0), dict(H=2 ** 20 + 1),
               dict(W=2 ** 20 + 1), dict(nmodels=-1), dict(total_v=-1), dict(total_f=-1), dict(max_verts=-1), dict(max_faces=-1),
               dict(znear=0.0), dict(znear=-1.0), dict(znear=nan), dict(label_kind=3), dict(label_kind=-1),
               dict(ninst=2), dict(total_inst=3),                                   # b * ninst != total_inst without inst_off
               dict(lights_stride=-9), dict(bg_strides=(0, -1, 0, 0)), dict(bg_strides=(0, 0, 0, -1)),
               dict(image_strides=(-1, 48, 3, 1)), dict(image_strides=(768, 48, -3, 1)),
               dict(image=None, label=None, inst=None, depth=None, face=None),       # won alone is no output
               dict(lights=None), dict(model_id=None), dict(inst_label=None), dict(pose=None), dict(K=None),
               dict(nmodels=0), dict(vert_off=None), dict(face_off=None), dict(verts=None), dict(faces=None), dict(colors=None)):
        assert render(**kw) == E, kw
    # the z-buffer's slot: total_inst * max_faces must stay below 2^32
    big = dict(inst_off=p, total_inst=65536, ninst=0)
    assert render(max_faces=65536, ws=None, **big) == E
    assert render(max_faces=65535, ws=None, **big) == EW
    assert render(max_faces=2 ** 31 - 1, total_inst=2, ws=None) == EW and render(max_faces=2 ** 31 - 1, total_inst=3, ninst=0, inst_off=p) == E
    # any single output is enough; the rest may be NULL
    for keep in ("image", "label", "inst", "depth", "face"):
        outs = {k: (p if k == keep else None) for k in ("image", "label", "inst", "depth", "face", "won")}
        assert render(ws=None, **outs) == EW, keep
    # misaligned pointers
    for kw in (dict(pose=260), dict(K=1028), dict(lights=260), dict(normals=260), dict(inst=258), dict(depth=257), dict(face=258),
               dict(won=1026), dict(label=260, label_kind=P.PV_LABEL_I64), dict(label=258, label_kind=P.PV_LABEL_I32)):
        assert render(**kw) == EA, kw
    assert render(label=257, ws=None) == EW and render(image=257, ws=None) == EW       # u8: any address
    # nothing to do: success, whatever the pointers; zero instances still need their outputs and lights
    assert render(b=0, total_inst=0, ninst=0, ws=None, nbytes=0, lights=None, image=None, label=None, inst=None, depth=None,
                  face=None) == 0
    assert render(total_inst=0, ninst=0, lights=None) == E
    assert render(total_inst=0, ninst=0, ws=None, model_id=None, pose=None, K=None, colors=None, nmodels=0) == EW

    def normals(null=False, out=p, **kw):
        m = dict(verts=p, vert_off=p, faces=p, face_off=p, colors=None, normals=None, nmodels=1, total_v=8, total_f=12,
                 max_verts=8, max_faces=12, reserved_=0)
        m.update(kw)
        M = P.ShadeMeshes(**m)
        return lib.pv_shade_normals(None if null else ctypes.byref(M), out, None)

    assert normals(null=True) == E and normals(out=None) == E and normals(out=260) == EA
    for kw in (dict(nmodels=-1), dict(total_v=-1), dict(total_f=-1), dict(max_verts=-1), dict(max_faces=-1), dict(vert_off=None),
               dict(face_off=None), dict(verts=None), dict(faces=None)):
        assert normals(**kw) == E, kw
    # nothing to do: success without a launch
    assert normals(nmodels=0, out=None) == 0 and normals(total_v=0, out=None, verts=None) == 0 and normals(max_verts=0) == 0


def test_python_layer_rejects_before_any_call():
    import numpy as np
    import torch
    from pvnet_amd import shade as S
    from tests import render_ref as R
    v, f = R.box()
    col = np.full((8, 3), 128, np.uint8)
    table = S.ColorMeshTable([(v, f, col)], device="cpu")
    assert table.normals is None and table.colors.dtype == torch.uint8 and tuple(table.colors.shape) == (8, 3)
    both = S.ColorMeshTable([(v, f, col), (v, f, col, np.ones((8, 3)))], device="cpu")
    assert tuple(both.normals.shape) == (16, 3) and (both.normals[:8] == 0).all() and (both.normals[8:] == 1).all()
    for bad in ([(v, f)], [(v, f, col[:7])], [(v, f, col.astype(np.float32))], [(v, f, col.astype(np.int32) + 200)],
                [(v, f, col, np.ones((7, 3)))]):
        with pytest.raises(ValueError):
            S.ColorMeshTable(bad, device="cpu")
    poses = torch.zeros((2, 1, 3, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device"):
        S.render_color(table, poses, [0], None, np.eye(3), 16, 16)            # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="ColorMeshTable"):
        S.render_color(object(), poses, [0], None, np.eye(3), 16, 16)
    with pytest.raises(RuntimeError, match="device"):
        table.with_smooth_normals()
    with pytest.raises(RuntimeError, match="poses"):
        S.render_bank(table, np.zeros((1, 9, 3)), poses, [0, 0], np.eye(3), 16, 16)
    d = S.default_lights(3)
    assert d.dtype == torch.float64 and tuple(d.shape) == (3, 9) and d[1].tolist() == [0, 0, -1, 0.3, 0.3, 0.3, 0.7, 0.7, 0.7]
    a, b2 = S.random_lights(64, 7), S.random_lights(64, 7)
    assert a.dtype == torch.float64 and tuple(a.shape) == (64, 9) and torch.equal(a, b2) and not torch.equal(a, S.random_lights(64, 8))
    assert (a[:, 2] <= 0).all() and torch.allclose(a[:, :3].norm(dim=1), torch.ones(64, dtype=torch.float64))
    assert ((a[:, 3:6] >= 0.2) & (a[:, 3:6] <= 0.5)).all() and ((a[:, 6:] >= 0.4) & (a[:, 6:] <= 0.8)).all()
    assert (a[:, 3] == a[:, 5]).all() and (a[:, 6] == a[:, 8]).all()
    c = S.random_lights(8, 1, ambient=(0.1, 0.1), diffuse=(0.9, 0.9))
    assert (c[:, 3:6] == 0.1).all() and (c[:, 6:] == 0.9).all()
    with pytest.raises(RuntimeError, match="ambient"):
        S.random_lights(2, 0, ambient=(0.5, 0.2))
