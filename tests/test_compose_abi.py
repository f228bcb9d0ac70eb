"""CPU-side checks of libpvcompose.so (include/pvcompose.h): it builds for gfx950 from the second table of
pvnet_amd/build.py, exports exactly its header, stands apart from the seven libraries of LIBS, and
rejects bad arguments on the host."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.test_build_table import HEADERS, exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_compose_apply", "pv_compose_finish", "pv_compose_params"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _compose_lib
    build.build()
    return _compose_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    assert list(build.MORE_LIBS) == ["compose"] and len(build.LIBS) == 7 and not set(build.MORE_LIBS) & set(build.LIBS)
    cmp_ = build.MORE_LIBS["compose"]
    assert isinstance(cmp_, build.Lib)
    assert cmp_.out == os.path.join(REPO, "pvnet_amd", "libpvcompose.so")
    assert cmp_.hdr == os.path.join(REPO, "include", "pvcompose.h")
    assert [os.path.basename(s) for s in cmp_.srcs] == ["pvcompose.hip"]
    assert b"gfx950" in open(cmp_.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    src = open(cmp_.srcs[0]).read()
    assert [i for i in re.findall(r'#include "([^"]+)"', src)] == ["../../include/pvcompose.h"]
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    # no transcendental, no fast-math form, no floating-point atomic
    assert not re.search(r"\b(?:exp|exp2|sin|cos|tan|pow|log|sincos)[fl]?\s*\(", src)
    assert not re.search(r"__expf|__fdividef|__sinf|__cosf|__powf|__logf|atomicAdd\(\s*\(?(float|double)", src)
    hdr = open(cmp_.hdr).read()
    for name in ("fuse", "NOT A REPLAY", "blur", "noise", "Flips", "erasing", "reflect-101", "tests/compose_ref.py"):
        assert name in hdr, name
    # pvaugment.h and augment.py point here for what they leave out
    assert "pvcompose.h" in open(os.path.join(REPO, "include", "pvaugment.h")).read()
    assert "compose" in open(os.path.join(REPO, "pvnet_amd", "augment.py")).read()


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _compose_lib
    assert header_functions("pvcompose.h") == NAMES
    assert exported(build.MORE_LIBS["compose"].out) == set(NAMES)
    assert {n for n, _, _ in _compose_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_compose_lib.py"


def test_closure_and_staleness(lib, monkeypatch):
    from pvnet_amd import build
    cmp_ = build.MORE_LIBS["compose"]
    got = build.closure(cmp_.srcs)
    assert set(got) == {*cmp_.srcs, cmp_.hdr} and len(got) == 2
    mm = subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", "-std=c++17", "--cuda-host-only", "-MM", *cmp_.srcs],
                        capture_output=True, text=True, check=True).stdout
    read = {os.path.realpath(w) for w in mm.replace("\\\n", " ").split() if not w.endswith(":")}
    root = os.path.realpath(REPO) + os.sep
    assert {p for p in read if p.startswith(root)} == {os.path.realpath(p) for p in got}
    seven = {k: set(build.closure(lib_.srcs)) for k, lib_ in build.LIBS.items()}
    for k, files in seven.items():
        assert not files & set(got), k
    # which edit makes which library stale: modification times simulated, no file touched
    outs = [lib_.out for lib_ in build.LIBS.values()] + [cmp_.out]
    real = os.path.getmtime
    newest = max(real(p) for p in outs) + 10

    def stale_after(paths):
        monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p in paths else real(p))
        return tuple(build.stale(o) for o in outs)

    F, T = False, True
    assert stale_after(set()) == (F,) * 8
    assert stale_after({cmp_.hdr}) == stale_after(set(cmp_.srcs)) == stale_after(set(got)) == (F,) * 7 + (T,)
    assert stale_after({build.__file__}) == (T,) * 8
    assert stale_after(set().union(*seven.values())) == (T,) * 7 + (F,)
    for name in ("_compose_lib.py", "compose.py", "__init__.py"):
        assert stale_after({os.path.join(REPO, "pvnet_amd", name)}) == (F,) * 8
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: newest if p == cmp_.hdr else real(p))
    assert build.needs_build()
    monkeypatch.undo()
    assert not build.needs_build()
    with pytest.raises(ValueError, match="LIBS"):
        build.stale(os.path.join(REPO, "pvnet_amd", "libpvnothing.so"))


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_before_and_after_the_seven(tmp_path, lang):
    from pvnet_amd import build
    if lang == "c":
        cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c"]) + ["-std=c99", "-pedantic-errors"]
    else:
        cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        cc = ([cc] if cc else [build.hipcc(), "-x", "c++"]) + ["-std=c++17"]
    for i, order in enumerate((["pvcompose.h"], ["pvcompose.h", *HEADERS], [*HEADERS, "pvcompose.h"])):
        src = tmp_path / f"order{i}.{'c' if lang == 'c' else 'cpp'}"
        src.write_text("".join(f'#include "{h}"\n' for h in order) +
                       "int pv_order_probe(pv_stream_t s, const pv_cmp_desc *d);\n"
                       "int pv_order_probe(pv_stream_t s, const pv_cmp_desc *d) "
                       "{ return s ? PV_OK : PV_EINVAL + PV_EWORKSPACE + PV_EALIGN + d->S + PV_CMP_TILE; }\n")
        r = subprocess.run([*cc, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (order, r.stderr)


def test_header_constants_match_binding():
    from pvnet_amd import _compose_lib as P, _augment_lib as A
    from tests import compose_ref as R
    src = open(os.path.join(REPO, "include", "pvcompose.h")).read()
    hip = open(os.path.join(REPO, "pvnet_amd", "csrc", "pvcompose.hip")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    assert (defs["PV_CMP_LABEL_I64"], defs["PV_CMP_LABEL_U8"], defs["PV_CMP_LABEL_I32"]) == \
        (P.PV_CMP_LABEL_I64, P.PV_CMP_LABEL_U8, P.PV_CMP_LABEL_I32) == \
        (A.PV_AUG_LABEL_I64, A.PV_AUG_LABEL_U8, A.PV_AUG_LABEL_I32)
    assert defs["PV_CMP_PIXELS"] == P.PV_CMP_PIXELS == A.PV_AUG_PIXELS == 8
    assert defs["PV_CMP_THREADS"] == P.PV_CMP_THREADS == A.PV_AUG_THREADS == 256
    assert defs["PV_CMP_TILE"] == P.PV_CMP_TILE == R.TILE == 32 and defs["PV_CMP_HALO"] == P.PV_CMP_HALO == 4
    assert defs["PV_CMP_MAX_SLOTS"] == P.PV_CMP_MAX_SLOTS == R.MAX_SLOTS == 16
    assert defs["PV_CMP_MAX_ERASE"] == P.PV_CMP_MAX_ERASE == R.MAX_ERASE == 8
    assert defs["PV_CMP_MAX_DIM"] == P.PV_CMP_MAX_DIM == R.MAX_DIM == 2 ** 15
    assert defs["PV_CMP_MAX_CLASSES"] == P.PV_CMP_MAX_CLASSES == 1024
    assert defs["PV_CMP_DRAW0"] == P.PV_CMP_DRAW0 == R.DRAW0 == 64 >= A.PV_AUG_DRAWS
    # a tile's LDS (the u8 tile with its halo, the f32 horizontal pass) lets several blocks share a CU's 160 KiB
    T, h = P.PV_CMP_TILE, P.PV_CMP_HALO
    assert 4 * ((T + 2 * h) ** 2 * 3 + (T + 2 * h) * T * 3 * 4) <= 160 * 1024
    # the generator's constants are pvaugment.h's, in the source and in the restatement
    aug = open(os.path.join(REPO, "include", "pvaugment.h")).read()
    for c in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15"):
        assert c in aug and c in hip
    assert int(R.G) == 0x9E3779B97F4A7C15 and "131070" in hip and "131070" in src
    # the structures are the header's
    assert ctypes.sizeof(P.CmpDesc) == 10 * 8 + 21 * 8 + 14 * 4 == 304
    assert P.CmpDesc.visible.offset == 72 and P.CmpDesc.image_strides.offset == 80 and P.CmpDesc.label_strides.offset == 112
    assert P.CmpDesc.background_strides.offset == 136 and P.CmpDesc.out_image_strides.offset == 168
    assert P.CmpDesc.out_label_strides.offset == 200 and P.CmpDesc.out_instance_strides.offset == 224
    assert P.CmpDesc.label_kind.offset == 248 and P.CmpDesc.b.offset == 264 and P.CmpDesc.S.offset == 276
    assert P.CmpDesc.ncls.offset == 284 and P.CmpDesc.fill.offset == 288 and P.CmpDesc.pad_.offset == 300
    assert ctypes.sizeof(P.CmpRanges) == 6 * 8 + 10 * 4 == 88
    assert P.CmpRanges.erase_frac.offset == 8 and P.CmpRanges.p_blur.offset == 24 and P.CmpRanges.noise.offset == 32
    assert P.CmpRanges.b.offset == 48 and P.CmpRanges.ncls.offset == 80
    assert ctypes.sizeof(P.CmpFinish) == 224
    assert P.CmpFinish.state.offset == 32 and P.CmpFinish.image_strides.offset == 40 and P.CmpFinish.out_strides.offset == 72
    assert P.CmpFinish.w.offset == 104 and P.CmpFinish.b.offset == 204 and P.CmpFinish.W.offset == 212


def test_argument_errors_without_device(lib):
    from pvnet_amd import _compose_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    N, H, W, Ho, Wo, S, E = 3, 48, 64, 40, 56, 4, 2
    nan, inf = float("nan"), float("inf")

    # ---- pv_compose_apply
    def desc(strides=None, fill=(0, 0, 0), **kw):
        d = dict(image=p, label=p, pick=p, shift=p, erase=p, background=p, out_image=p, out_label=p, out_instance=p, visible=p,
                 label_kind=P.PV_CMP_LABEL_U8, N=N, H=H, W=W, b=2, Ho=Ho, Wo=Wo, S=S, E=E, ncls=2)
        d.update(kw)
        t = P.CmpDesc(**d)
        s = dict(image_strides=(H * W * 3, W * 3, 3, 1), label_strides=(H * W, W, 1), background_strides=(0, Wo * 3, 3, 1),
                 out_image_strides=(Ho * Wo * 3, Wo * 3, 3, 1), out_label_strides=(Ho * Wo, Wo, 1),
                 out_instance_strides=(Ho * Wo, Wo, 1))
        s.update(strides or {})
        for k, v in s.items():
            getattr(t, k)[:] = v
        t.fill[:] = fill
        return t

    def apply(d=None, null=False):
        d = d or desc()
        return lib.pv_compose_apply(None if null else ctypes.byref(d), None)

    assert apply(null=True) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=0), dict(H=-1), dict(W=2 ** 15 + 1), dict(Ho=2 ** 15 + 1),
               dict(N=0), dict(N=-1), dict(S=0), dict(S=17), dict(E=-1), dict(E=9), dict(ncls=0), dict(ncls=1025),
               dict(ncls=256), dict(label_kind=3), dict(label_kind=-1), dict(fill=(-1, 0, 0)), dict(fill=(0, 256, 0)),
               dict(image=None), dict(label=None), dict(pick=None), dict(shift=None), dict(erase=None), dict(out_image=None),
               dict(out_label=None), dict(visible=None)):
        assert apply(desc(**kw)) == P.PV_EINVAL, kw
    for name, n in (("image_strides", 4), ("label_strides", 3), ("background_strides", 4), ("out_image_strides", 4),
                    ("out_label_strides", 3), ("out_instance_strides", 3)):
        for i in range(n):
            s = [7] * n
            s[i] = -1
            assert apply(desc(strides={name: s})) == P.PV_EINVAL, (name, i)
    # one frame of any operand spans at most 2^31 - 1 elements
    assert apply(desc(strides=dict(image_strides=(0, 2 ** 31 // (H - 1) + 1, 3, 1)))) == P.PV_EINVAL
    assert apply(desc(strides=dict(label_strides=(0, 1, 2 ** 31 // (W - 1) + 1)))) == P.PV_EINVAL
    assert apply(desc(strides=dict(background_strides=(0, 1, 1, 2 ** 30)))) == P.PV_EINVAL
    assert apply(desc(strides=dict(out_image_strides=(0, 1, 1, 2 ** 30)))) == P.PV_EINVAL
    assert apply(desc(strides=dict(out_label_strides=(0, 2 ** 31 // (Ho - 1) + 1, 1)))) == P.PV_EINVAL
    assert apply(desc(strides=dict(out_instance_strides=(0, 2 ** 31 // (Ho - 1) + 1, 1)))) == P.PV_EINVAL
    # a batch whose launch would reach 2^32 threads
    assert apply(desc(b=2 ** 24, Ho=8, Wo=256)) == P.PV_EINVAL
    # alignment to the element
    for name in ("pick", "shift", "erase", "visible"):
        assert apply(desc(**{name: 258})) == P.PV_EALIGN, name
    assert apply(desc(label=258, label_kind=P.PV_CMP_LABEL_I32)) == P.PV_EALIGN
    assert apply(desc(out_label=260, label_kind=P.PV_CMP_LABEL_I64)) == P.PV_EALIGN
    assert apply(desc(out_instance=260, label_kind=P.PV_CMP_LABEL_I64)) == P.PV_EALIGN
    # nothing to do: success, no launch, whatever the pointers
    assert apply(desc(b=0)) == 0
    assert apply(desc(b=0, image=None, label=None, pick=None, shift=None, erase=None, background=None, out_image=None,
                      out_label=None, out_instance=None, visible=None)) == 0
    assert apply(desc(b=0, S=0)) == P.PV_EINVAL and apply(desc(b=0, fill=(0, 0, 300))) == P.PV_EINVAL

    # ---- pv_compose_params
    def ranges(frac=(0.1, 0.4), noise=(0.0, 8.0), **kw):
        d = dict(margin=0.25, p_blur=0.5, b=2, N=N, H=H, W=W, Ho=Ho, Wo=Wo, S=S, E=E, ncls=2)
        d.update(kw)
        t = P.CmpRanges(**d)
        t.erase_frac[:], t.noise[:] = frac, noise
        return t

    def params(r=None, ptrs=None, null=False):
        r = r or ranges()
        q = dict(pick=p, state=p, shift=p, erase=p, ksel=p, amp=p)
        q.update(ptrs or {})
        return lib.pv_compose_params(None if null else ctypes.byref(r), q["pick"], q["state"], q["shift"], q["erase"],
                                     q["ksel"], q["amp"], None)

    assert params(null=True) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=-3), dict(Wo=2 ** 15 + 1), dict(N=0), dict(S=0), dict(S=17),
               dict(E=-1), dict(E=9), dict(ncls=0), dict(ncls=1025),
               dict(margin=-0.01), dict(margin=0.51), dict(margin=nan),
               dict(frac=(0.0, 0.5)), dict(frac=(-0.1, 0.5)), dict(frac=(0.5, 0.4)), dict(frac=(0.5, 1.01)), dict(frac=(nan, 0.5)),
               dict(frac=(0.5, nan)), dict(p_blur=-0.1), dict(p_blur=1.1), dict(p_blur=nan),
               dict(noise=(-1.0, 2.0)), dict(noise=(3.0, 2.0)), dict(noise=(0.0, inf)), dict(noise=(nan, 1.0)), dict(noise=(0.0, nan))):
        assert params(ranges(**kw)) == P.PV_EINVAL, kw
    for name in ("pick", "state", "shift", "erase", "ksel", "amp"):
        assert params(ptrs={name: None}) == P.PV_EINVAL, name
        assert params(ptrs={name: 258}) == P.PV_EALIGN, name
    assert params(ptrs=dict(state=260)) == P.PV_EALIGN
    assert params(ranges(b=0)) == 0
    assert params(ranges(b=0), ptrs=dict(pick=None, state=None, shift=None, erase=None, ksel=None, amp=None)) == 0
    assert params(ranges(b=0, margin=0.6)) == P.PV_EINVAL

    # ---- pv_compose_finish
    def fin(w=None, strides=None, **kw):
        d = dict(image=p, out=512, ksel=p, amp=p, state=p, b=2, H=H, W=W)
        d.update(kw)
        t = P.CmpFinish(**d)
        s = dict(image_strides=(H * W * 3, W * 3, 3, 1), out_strides=(H * W * 3, W * 3, 3, 1))
        s.update(strides or {})
        for k, v in s.items():
            getattr(t, k)[:] = v
        for j in range(5):
            for k in range(5):
                t.w[j][k] = 0.1 if w is None else w(j, k)
        return t

    def finish(d=None, null=False):
        d = d or fin()
        return lib.pv_compose_finish(None if null else ctypes.byref(d), None)

    assert finish(null=True) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(H=2 ** 15 + 1), dict(W=-1), dict(image=None), dict(out=None), dict(ksel=None),
               dict(amp=None), dict(state=None), dict(out=p)):                 # the output at the input's address
        assert finish(fin(**kw)) == P.PV_EINVAL, kw
    for bad in (nan, inf, -0.5):
        assert finish(fin(w=lambda j, k: bad if (j, k) == (3, 2) else 0.1)) == P.PV_EINVAL
        assert finish(fin(b=0, w=lambda j, k: bad if (j, k) == (2, 3) else 0.1)) == 0       # past t = j: not read
    for name in ("image_strides", "out_strides"):
        for i in range(4):
            s = [7] * 4
            s[i] = -1
            assert finish(fin(strides={name: s})) == P.PV_EINVAL, (name, i)
        assert finish(fin(strides={name: (0, 1, 1, 2 ** 30)})) == P.PV_EINVAL
    assert finish(fin(b=2 ** 24, H=32, W=32)) == P.PV_EINVAL                     # a launch of 2^32 threads
    assert finish(fin(ksel=258)) == P.PV_EALIGN and finish(fin(amp=258)) == P.PV_EALIGN and finish(fin(state=260)) == P.PV_EALIGN
    assert finish(fin(b=0)) == 0
    assert finish(fin(b=0, image=None, out=None, ksel=None, amp=None, state=None)) == 0
    assert finish(fin(b=0, H=0)) == P.PV_EINVAL


def test_python_layer_rejects_before_any_call():
    import torch
    import pvnet_amd
    from pvnet_amd import compose as C
    for name in ("Placement", "make_picks", "random_placement", "shift_keypoints", "shift_camera", "visible_fraction",
                 "compose_ground_truth"):
        assert getattr(pvnet_amd, name) is getattr(C, name) and name in pvnet_amd.__all__
    assert callable(pvnet_amd.compose.compose) and callable(pvnet_amd.compose.finish)
    N, H, W, b, S = 3, 6, 8, 2, 2
    img = torch.zeros(N, H, W, 3, dtype=torch.uint8)
    lab = torch.zeros(N, H, W, dtype=torch.uint8)
    state = torch.zeros(2, dtype=torch.int64)
    src = torch.tensor([[0, 1], [2, 5]])
    pick = C.make_picks(src, torch.tensor([1, 2]))
    assert pick.dtype == torch.int32 and pick.tolist()[1][1] == [5, 1, 2, 0, 0, 2 ** 15 - 1, 2 ** 15 - 1, 0]
    stats = torch.tensor([[4, 0, 0, 1, 2, 3, 4, 0], [0, 0, 0, W, H, -1, -1, 0], [1, 0, 0, 5, 5, 5, 5, 0]])
    pick = C.make_picks(src, torch.tensor([1, 2]), stats, src_label=7)
    assert pick[0].tolist() == [[0, 7, 1, 1, 2, 3, 4, 0], [1, 7, 2, W, H, -1, -1, 0]] and pick[1, 1, 0] == 5
    shift = torch.zeros(b, S, 2, dtype=torch.int32)
    kp = torch.zeros(N, 9, 2)
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="device"):
        C.random_placement(pick, (N, H, W), (H, W), state)
    with pytest.raises(RuntimeError, match="device"):
        C.compose(img, lab, pick, shift, 2, (H, W))
    with pytest.raises(RuntimeError, match="device"):
        C.finish(img, torch.zeros(N, dtype=torch.int32), torch.zeros(N), state)
    with pytest.raises(RuntimeError, match="device"):
        C.compose_ground_truth(img, lab, kp, pick, 2, (H, W), state)
    # wrong shapes and kinds, before the device is looked at
    with pytest.raises(RuntimeError, match="src"):
        C.make_picks(src.float(), 1)
    with pytest.raises(RuntimeError, match="src"):
        C.make_picks(torch.zeros(2, 17, dtype=torch.int64), 1)
    with pytest.raises(RuntimeError, match="cls"):
        C.make_picks(src, torch.tensor([1, 2, 3]))
    with pytest.raises(RuntimeError, match="bank_stats"):
        C.make_picks(src, 1, stats[:, :7])
    with pytest.raises(RuntimeError, match="pick"):
        C.random_placement(pick.long(), (N, H, W), (H, W), state)
    with pytest.raises(RuntimeError, match="pick"):
        C.random_placement(pick[..., :7], (N, H, W), (H, W), state)
    with pytest.raises(RuntimeError, match="bank_size"):
        C.random_placement(pick, (N, H), (H, W), state)
    with pytest.raises(RuntimeError, match="bank_size"):
        C.random_placement(pick, (0, H, W), (H, W), state)
    with pytest.raises(RuntimeError, match="out_size"):
        C.random_placement(pick, (N, H, W), (0, W), state)
    with pytest.raises(RuntimeError, match="out_size"):
        C.random_placement(pick, (N, H, W), 5, state)
    with pytest.raises(RuntimeError, match="state"):
        C.random_placement(pick, (N, H, W), (H, W), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="state"):
        C.random_placement(pick, (N, H, W), (H, W), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="margin"):
        C.random_placement(pick, (N, H, W), (H, W), state, margin=0.7)
    with pytest.raises(RuntimeError, match="erasers"):
        C.random_placement(pick, (N, H, W), (H, W), state, erasers=9)
    with pytest.raises(RuntimeError, match="erase_frac"):
        C.random_placement(pick, (N, H, W), (H, W), state, erase_frac=(0.0, 0.5))
    with pytest.raises(RuntimeError, match="erase_frac"):
        C.random_placement(pick, (N, H, W), (H, W), state, erase_frac=(0.5,))
    with pytest.raises(RuntimeError, match="blur_p"):
        C.random_placement(pick, (N, H, W), (H, W), state, blur_p=1.5)
    with pytest.raises(RuntimeError, match="noise"):
        C.random_placement(pick, (N, H, W), (H, W), state, noise=(2.0, 1.0))
    with pytest.raises(RuntimeError, match="noise"):
        C.random_placement(pick, (N, H, W), (H, W), state, noise=(0.0, float("inf")))
    with pytest.raises(RuntimeError, match="class_num"):
        C.random_placement(pick, (N, H, W), (H, W), state, class_num=0)
    with pytest.raises(RuntimeError, match="bank_image"):
        C.compose(img.permute(0, 3, 1, 2), lab, pick, shift, 2, (H, W))
    with pytest.raises(RuntimeError, match="bank_image"):
        C.compose(img.float(), lab, pick, shift, 2, (H, W))
    with pytest.raises(RuntimeError, match="bank_image"):
        C.compose(img[:, :, :4], lab, pick, shift, 2, (H, W))
    with pytest.raises(RuntimeError, match="bank_label"):
        C.compose(img, lab.float(), pick, shift, 2, (H, W))
    with pytest.raises(RuntimeError, match="shift"):
        C.compose(img, lab, pick, shift[:, :1], 2, (H, W))
    with pytest.raises(RuntimeError, match="shift"):
        C.compose(img, lab, pick, shift.long(), 2, (H, W))
    with pytest.raises(RuntimeError, match="class_num"):
        C.compose(img, lab, pick, shift, 0, (H, W))
    with pytest.raises(RuntimeError, match="class_num"):
        C.compose(img, lab, pick, shift, 256, (H, W))
    with pytest.raises(RuntimeError, match="out_size"):
        C.compose(img, lab, pick, shift, 2, (H, 2 ** 15 + 1))
    with pytest.raises(RuntimeError, match="background"):
        C.compose(img, lab, pick, shift, 2, (H, W), background=torch.zeros(b, H, W + 1, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="background"):
        C.compose(img, lab, pick, shift, 2, (H, W), background=torch.zeros(b, H, W, 3))
    with pytest.raises(RuntimeError, match="fill"):
        C.compose(img, lab, pick, shift, 2, (H, W), fill=300)
    with pytest.raises(RuntimeError, match="fill"):
        C.compose(img, lab, pick, shift, 2, (H, W), fill=(1, 2))
    with pytest.raises(RuntimeError, match="erase"):
        C.compose(img, lab, pick, shift, 2, (H, W), erase=torch.zeros(b, 9, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="erase"):
        C.compose(img, lab, pick, shift, 2, (H, W), erase=torch.zeros(b, 2, 4))
    with pytest.raises(RuntimeError, match="out must"):
        C.compose(img, lab, pick, shift, 2, (H, W), out=(torch.zeros(b, H, W, 3), torch.zeros(b, H, W, dtype=torch.uint8)))
    with pytest.raises(RuntimeError, match="image"):
        C.finish(img.float(), torch.zeros(N, dtype=torch.int32), torch.zeros(N), state)
    with pytest.raises(RuntimeError, match="ksel"):
        C.finish(img, torch.zeros(N, dtype=torch.int64), torch.zeros(N), state)
    with pytest.raises(RuntimeError, match="amp"):
        C.finish(img, torch.zeros(N, dtype=torch.int32), torch.zeros(N + 1), state)
    with pytest.raises(RuntimeError, match="state"):
        C.finish(img, torch.zeros(N, dtype=torch.int32), torch.zeros(N), state[:1])
    with pytest.raises(RuntimeError, match="alias"):
        C.finish(img, torch.zeros(N, dtype=torch.int32), torch.zeros(N), state, out=img)
    with pytest.raises(RuntimeError, match="bank_keypoints"):
        C.compose_ground_truth(img, lab, kp[:2], pick, 2, (H, W), state)
    with pytest.raises(RuntimeError, match="bank_keypoints"):
        C.shift_keypoints(torch.zeros(N, 9, 3), pick, shift, 2)
    with pytest.raises(RuntimeError, match="K must"):
        C.shift_camera(torch.zeros(3, 4), shift)
    with pytest.raises(RuntimeError, match="visible"):
        C.visible_fraction(torch.zeros(2, 3), torch.zeros(2, 2))
    # the ground-truth helpers are plain torch
    kp = torch.arange(N * 2 * 2, dtype=torch.float32).reshape(N, 2, 2)
    pk = C.make_picks(torch.tensor([[0, 2, 1, 7]]), torch.tensor([[2, 1, 2, 1]]))
    sh = torch.tensor([[[1, -1], [10, 20], [-3, 4], [9, 9]]], dtype=torch.int32)
    out, present = C.shift_keypoints(kp, pk, sh, 3)
    assert out.dtype == torch.float64 and tuple(out.shape) == (1, 3, 2, 2) and present.tolist() == [[True, True, False]]
    assert out[0, 0].tolist() == (kp[2].double() + torch.tensor([10.0, 20.0])).tolist()       # slot 3's src is outside the bank
    assert out[0, 1].tolist() == (kp[1].double() + torch.tensor([-3.0, 4.0])).tolist()        # the last live slot of class 2 wins
    assert (out[0, 2] == 0).all()
    K = torch.tensor([[100.0, 0.0, 30.0], [0.0, 110.0, 20.0], [0.0, 0.0, 1.0]])
    Ks = C.shift_camera(K, sh)
    assert tuple(Ks.shape) == (1, 4, 3, 3) and Ks[0, 2].tolist() == [[100.0, 0.0, 27.0], [0.0, 110.0, 24.0], [0.0, 0.0, 1.0]]
    frac = C.visible_fraction(torch.tensor([[5, 0, 3]], dtype=torch.int32), torch.tensor([[10, 0, 3]]))
    assert frac.tolist() == [[0.5, 0.0, 1.0]]
