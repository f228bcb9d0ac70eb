"""CPU-side checks of libpvaugment.so (include/pvaugment.h): it builds for gfx950, exports exactly its
header, and rejects bad arguments on the host."""
import ctypes
import os
import re

import pytest

from tests.test_build_table import exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_augment_apply", "pv_augment_params", "pv_augment_workspace_size", "pv_label_stats"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _augment_lib
    build.build()
    return _augment_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    aug = build.LIBS["augment"]
    assert aug.out == os.path.join(REPO, "pvnet_amd", "libpvaugment.so")
    assert aug.hdr == os.path.join(REPO, "include", "pvaugment.h")
    assert [os.path.basename(s) for s in aug.srcs] == ["pvaugment.hip"]
    assert set(build.closure(aug.srcs)) == {*aug.srcs, aug.hdr}
    assert b"gfx950" in open(aug.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    # the translation unit includes nothing else of csrc/, no floating-point atomic, no fast-math form
    src = open(aug.srcs[0]).read()
    assert [i for i in re.findall(r'#include "([^"]+)"', src)] == ["../../include/pvaugment.h"]
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    assert not re.search(r"__expf|__fdividef|__sinf|__cosf|atomicAdd\(\s*\(?(float|double)", src)
    # per-pixel trigonometry has no place in the sampler: cos and sin appear in k_params alone
    assert len(re.findall(r"\b(?:cos|sin)f?\(", src)) == 2
    # the reference functions the header replaces are named in it, and what is out of scope
    hdr = open(aug.hdr).read()
    for name in ("LineModDatasetRealAug", "rotate_instance", "crop_resize_instance_v1", "crop_or_padding_to_fixed_size",
                 "ColorJitter", "compute_vertex", "NOT A REPLAY", "blur", "noise", "flips", "occlusion"):
        assert name in hdr, name


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _augment_lib
    assert header_functions("pvaugment.h") == NAMES
    assert exported(build.LIBS["augment"].out) == set(NAMES)
    assert {n for n, _, _ in _augment_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_augment_lib.py"


def test_header_constants_match_binding():
    from pvnet_amd import _augment_lib as P, _render_lib
    src = open(os.path.join(REPO, "include", "pvaugment.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    assert (defs["PV_AUG_LABEL_I64"], defs["PV_AUG_LABEL_U8"], defs["PV_AUG_LABEL_I32"]) == \
        (P.PV_AUG_LABEL_I64, P.PV_AUG_LABEL_U8, P.PV_AUG_LABEL_I32) == \
        (_render_lib.PV_LABEL_I64, _render_lib.PV_LABEL_U8, _render_lib.PV_LABEL_I32)
    assert (defs["PV_AUG_F32"], defs["PV_AUG_F16"]) == (P.PV_AUG_F32, P.PV_AUG_F16) == \
        (_render_lib.PV_FIELD_F32, _render_lib.PV_FIELD_F16)
    assert (defs["PV_AUG_BRIGHTNESS"], defs["PV_AUG_CONTRAST"], defs["PV_AUG_SATURATION"], defs["PV_AUG_HUE"]) == \
        (P.PV_AUG_BRIGHTNESS, P.PV_AUG_CONTRAST, P.PV_AUG_SATURATION, P.PV_AUG_HUE) == (1, 2, 4, 8)
    assert P.PV_AUG_ALL == 15
    assert defs["PV_AUG_PIXELS"] == P.PV_AUG_PIXELS == 8
    assert defs["PV_AUG_THREADS"] == P.PV_AUG_THREADS == 256
    assert defs["PV_AUG_MAX_DIM"] == P.PV_AUG_MAX_DIM == 2 ** 20
    assert defs["PV_AUG_MAX_CLASSES"] == P.PV_AUG_MAX_CLASSES == 1024
    assert defs["PV_AUG_DRAWS"] == P.PV_AUG_DRAWS == 8
    # the generator's constants are the header's, and the numpy restatement's
    from tests import augment_ref as R
    for c in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15"):
        assert c in src and c in open(os.path.join(REPO, "pvnet_amd", "csrc", "pvaugment.hip")).read()
    assert int(R.G) == 0x9E3779B97F4A7C15 and R.DRAWS == P.PV_AUG_DRAWS
    assert (R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE) == (1, 2, 4, 8)
    # the structures are the header's
    assert ctypes.sizeof(P.AugLabel) == 8 + 3 * 8 + 4 * 4 == 48
    assert P.AugLabel.label_kind.offset == 32 and P.AugLabel.W.offset == 44
    assert ctypes.sizeof(P.AugRanges) == 9 * 8 + 6 * 4 == 96
    assert P.AugRanges.margin.offset == 32 and P.AugRanges.jitter.offset == 40 and P.AugRanges.b.offset == 72
    assert ctypes.sizeof(P.AugDesc) == 272
    assert P.AugDesc.image_strides.offset == 56 and P.AugDesc.label_strides.offset == 88
    assert P.AugDesc.background_strides.offset == 112 and P.AugDesc.out_image_strides.offset == 144
    assert P.AugDesc.out_label_strides.offset == 176 and P.AugDesc.fill.offset == 200 and P.AugDesc.mean.offset == 212
    assert P.AugDesc.std.offset == 224 and P.AugDesc.label_kind.offset == 236 and P.AugDesc.Wo.offset == 264


def test_workspace_size(lib):
    f = lib.pv_augment_workspace_size
    assert f(-1, 8, 8) == 0 and f(1, 0, 8) == 0 and f(1, 8, 0) == 0 and f(1, -8, 8) == 0 and f(1, 8, 2 ** 20 + 1) == 0
    assert f(2 ** 31 - 1, 2 ** 20, 2 ** 20) == 0                      # more blocks than a grid holds
    # a launch stays below 2^32 threads: at most 2^24 - 1 blocks of 256 lanes (2,048 pixels a block)
    assert f(2 ** 24 - 1, 8, 256) > 0 and f(2 ** 24, 8, 256) == 0 and f(1, 2 ** 20, 2 ** 20) == 0
    assert f(1, 2 ** 15, 2 ** 20) == 0 and f(1, 2 ** 15 - 1, 2 ** 20) > 0
    base = f(1, 1, 1)
    assert base > 0 and base % 256 == 0 and f(0, 8, 8) > 0
    # one f64 partial per block of 256 lanes x 8 pixels
    assert f(32, 480, 640) >= 32 * (480 * 640 // 2048) * 8
    assert f(1, 480, 640) < f(2, 480, 640) < f(2, 960, 640) < f(2, 960, 1280)
    assert f(32, 480, 640) < 1 << 16                                  # and stays small


def test_argument_errors_without_device(lib):
    from pvnet_amd import _augment_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    big = 1 << 30
    H, W, Ho, Wo = 48, 64, 40, 56
    nan, inf = float("nan"), float("inf")

    # ---- pv_label_stats
    def lab(ls=None, **kw):
        d = dict(label=p, label_kind=P.PV_AUG_LABEL_U8, b=2, H=H, W=W)
        d.update(kw)
        t = P.AugLabel(**d)
        t.label_strides[:] = ls or (H * W, W, 1)
        return t

    def stats(d=None, ncls=1, out=p, null=False):
        d = d or lab()
        return lib.pv_label_stats(None if null else ctypes.byref(d), ncls, out, None)

    assert stats(null=True) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(H=-1), dict(W=2 ** 20 + 1), dict(label_kind=3), dict(label_kind=-1),
               dict(label=None)):
        assert stats(lab(**kw)) == P.PV_EINVAL, kw
    for n in (0, -1, P.PV_AUG_MAX_CLASSES + 1):
        assert stats(ncls=n) == P.PV_EINVAL
    for i in range(3):
        ls = [H * W, W, 1]
        ls[i] = -1
        assert stats(lab(ls=ls)) == P.PV_EINVAL
    assert stats(out=None) == P.PV_EINVAL
    assert stats(out=260) == P.PV_EALIGN and stats(lab(label=258, label_kind=P.PV_AUG_LABEL_I32)) == P.PV_EALIGN
    assert stats(lab(label=260, label_kind=P.PV_AUG_LABEL_I64)) == P.PV_EALIGN
    assert stats(lab(b=0)) == 0 and stats(lab(b=0, label=None), out=None) == 0 and stats(lab(b=0), ncls=0) == P.PV_EINVAL

    # ---- pv_augment_params
    def ranges(rot=(-30.0, 30.0), scale=(0.8, 1.2), jitter=(0.1, 0.1, 0.05, 0.05), **kw):
        d = dict(margin=0.25, b=2, H=H, W=W, Ho=Ho, Wo=Wo)
        d.update(kw)
        t = P.AugRanges(**d)
        t.rot_deg[:], t.scale[:], t.jitter[:] = rot, scale, jitter
        return t

    def params(r=None, ptrs=None, null=False):
        r = r or ranges()
        q = dict(stats=p, state=p, fwd=p, inv=p, color=p)
        q.update(ptrs or {})
        return lib.pv_augment_params(None if null else ctypes.byref(r), q["stats"], q["state"], q["fwd"], q["inv"],
                                     q["color"], None)

    assert params(null=True) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=0), dict(Ho=-3), dict(Wo=2 ** 20 + 1),
               dict(margin=-0.01), dict(margin=0.51), dict(margin=nan),
               dict(rot=(30.0, -30.0)), dict(rot=(nan, 1.0)), dict(rot=(0.0, inf)), dict(rot=(-inf, 0.0)),
               dict(scale=(0.0, 1.0)), dict(scale=(-1.0, 1.0)), dict(scale=(1.2, 0.8)), dict(scale=(nan, 1.0)),
               dict(scale=(1.0, inf)), dict(scale=(1.0, nan)),
               dict(jitter=(-0.1, 0, 0, 0)), dict(jitter=(0, 1.1, 0, 0)), dict(jitter=(0, 0, nan, 0)),
               dict(jitter=(0, 0, 0, 0.6)), dict(jitter=(0, 0, 0, -0.1)), dict(jitter=(inf, 0, 0, 0))):
        assert params(ranges(**kw)) == P.PV_EINVAL, kw
    for name in ("stats", "state", "fwd", "inv", "color"):
        assert params(ptrs={name: None}) == P.PV_EINVAL, name
        assert params(ptrs={name: 258}) == P.PV_EALIGN, name
    assert params(ranges(b=0)) == 0
    assert params(ranges(b=0), ptrs=dict(stats=None, state=None, fwd=None, inv=None, color=None)) == 0
    assert params(ranges(b=0, margin=0.6)) == P.PV_EINVAL

    # ---- pv_augment_apply
    def desc(strides=None, fill=(0, 0, 0), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), **kw):
        d = dict(image=p, label=p, inv=p, color=p, background=p, out_image=p, out_label=p, label_kind=P.PV_AUG_LABEL_U8,
                 out_kind=P.PV_AUG_F16, flags=P.PV_AUG_ALL, b=2, H=H, W=W, Ho=Ho, Wo=Wo)
        d.update(kw)
        t = P.AugDesc(**d)
        s = dict(image_strides=(H * W * 3, W * 3, 3, 1), label_strides=(H * W, W, 1), background_strides=(0, Wo * 3, 3, 1),
                 out_image_strides=(3 * Ho * Wo, Ho * Wo, Wo, 1), out_label_strides=(Ho * Wo, Wo, 1))
        s.update(strides or {})
        for k, v in s.items():
            getattr(t, k)[:] = v
        t.fill[:], t.mean[:], t.std[:] = fill, mean, std
        return t

    def apply(d=None, ws=p, nbytes=big, null=False):
        d = d or desc()
        return lib.pv_augment_apply(None if null else ctypes.byref(d), ws, nbytes, None)

    assert apply(null=True) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=0), dict(H=-1), dict(W=2 ** 20 + 1), dict(Ho=2 ** 20 + 1),
               dict(label_kind=3), dict(label_kind=-1), dict(out_kind=2), dict(out_kind=-1), dict(flags=16), dict(flags=-1),
               dict(image=None), dict(label=None), dict(inv=None), dict(color=None), dict(out_image=None), dict(out_label=None),
               dict(fill=(-1, 0, 0)), dict(fill=(0, 256, 0)), dict(fill=(0, 0, nan)), dict(mean=(nan, 0, 0)), dict(mean=(0, inf, 0)),
               dict(std=(0, 1, 1)), dict(std=(1, -1, 1)), dict(std=(1, 1, nan)), dict(std=(inf, 1, 1))):
        assert apply(desc(**kw)) == P.PV_EINVAL, kw
    for name, n in (("image_strides", 4), ("label_strides", 3), ("background_strides", 4), ("out_image_strides", 4),
                    ("out_label_strides", 3)):
        for i in range(n):
            s = [7] * n
            s[i] = -1
            assert apply(desc(strides={name: s})) == P.PV_EINVAL, (name, i)
    # one image of the source, the label map or the background spans at most 2^31 - 1 elements
    assert apply(desc(strides=dict(image_strides=(0, 2 ** 31 // (H - 1) + 1, 3, 1)))) == P.PV_EINVAL
    assert apply(desc(strides=dict(label_strides=(0, 1, 2 ** 31 // (W - 1) + 1)))) == P.PV_EINVAL
    assert apply(desc(strides=dict(background_strides=(0, 1, 1, 2 ** 30)))) == P.PV_EINVAL
    # a batch whose launch would reach 2^32 threads
    assert apply(desc(b=2 ** 24, Ho=8, Wo=256, strides=dict(out_image_strides=(0, 0, 0, 1), out_label_strides=(0, 0, 1),
                                                            background_strides=(0, 0, 0, 1)))) == P.PV_EINVAL
    assert stats(lab(b=2 ** 24, H=64, W=128, ls=(0, 128, 1))) == P.PV_EINVAL
    # the workspace: needed with contrast only
    need = lib.pv_augment_workspace_size(2, Ho, Wo)
    assert need > 0
    assert apply(ws=None) == P.PV_EWORKSPACE and apply(nbytes=need - 1) == P.PV_EWORKSPACE and apply(nbytes=0) == P.PV_EWORKSPACE
    assert apply(ws=264) == P.PV_EALIGN
    # alignment to the element
    assert apply(desc(inv=260)) == P.PV_EALIGN and apply(desc(color=258)) == P.PV_EALIGN
    assert apply(desc(out_image=257)) == P.PV_EALIGN and apply(desc(out_image=258, out_kind=P.PV_AUG_F32)) == P.PV_EALIGN
    assert apply(desc(label=258, label_kind=P.PV_AUG_LABEL_I32)) == P.PV_EALIGN
    assert apply(desc(out_label=260, label_kind=P.PV_AUG_LABEL_I64)) == P.PV_EALIGN
    # nothing to do: success, no launch, whatever the pointers
    assert apply(desc(b=0)) == 0
    assert apply(desc(b=0, image=None, label=None, inv=None, color=None, background=None, out_image=None, out_label=None),
                 ws=None, nbytes=0) == 0
    assert apply(desc(b=0, flags=99)) == P.PV_EINVAL and apply(desc(b=0, std=(0, 1, 1))) == P.PV_EINVAL


def test_python_layer_rejects_before_any_call():
    import torch
    import pvnet_amd
    from pvnet_amd import augment as A
    for name in ("AugmentParams", "label_stats", "random_params", "transform_keypoints", "augment_ground_truth"):
        assert getattr(pvnet_amd, name) is getattr(A, name) and name in pvnet_amd.__all__
    b, H, W = 2, 6, 8
    img = torch.zeros(b, H, W, 3, dtype=torch.uint8)
    lab = torch.zeros(b, H, W, dtype=torch.uint8)
    state = torch.zeros(2, dtype=torch.int64)
    prm = A.AugmentParams(torch.zeros(b, 2, 3, dtype=torch.float64), torch.zeros(b, 2, 3, dtype=torch.float64),
                          torch.zeros(b, 4))
    kp = torch.zeros(b, 1, 9, 2, dtype=torch.float64)
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="device"):
        A.label_stats(lab, 1)
    with pytest.raises(RuntimeError, match="device"):
        A.random_params(lab, 1, (H, W), state)
    with pytest.raises(RuntimeError, match="device"):
        A.apply(img, lab, prm)
    with pytest.raises(RuntimeError, match="device"):
        A.augment_ground_truth(img, lab, kp, 1, state)
    # wrong shapes and kinds, before the device is looked at
    with pytest.raises(RuntimeError, match="label"):
        A.label_stats(lab.float(), 1)
    with pytest.raises(RuntimeError, match="label"):
        A.label_stats(lab[0], 1)
    with pytest.raises(RuntimeError, match="class_num"):
        A.label_stats(lab, 0)
    with pytest.raises(RuntimeError, match="out_size"):
        A.random_params(lab, 1, (0, W), state)
    with pytest.raises(RuntimeError, match="out_size"):
        A.random_params(lab, 1, 5, state)
    with pytest.raises(RuntimeError, match="state"):
        A.random_params(lab, 1, (H, W), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="state"):
        A.random_params(lab, 1, (H, W), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="rot_deg"):
        A.random_params(lab, 1, (H, W), state, rot_deg=(10, -10))
    with pytest.raises(RuntimeError, match="scale"):
        A.random_params(lab, 1, (H, W), state, scale=(0.0, 1.0))
    with pytest.raises(RuntimeError, match="margin"):
        A.random_params(lab, 1, (H, W), state, margin=0.7)
    with pytest.raises(RuntimeError, match="jitter"):
        A.random_params(lab, 1, (H, W), state, jitter=(0.1, 0.1, 0.1, 0.9))
    with pytest.raises(RuntimeError, match="jitter"):
        A.random_params(lab, 1, (H, W), state, jitter=(0.1, 0.1, 0.1))
    with pytest.raises(RuntimeError, match="image"):
        A.apply(img.permute(0, 3, 1, 2), lab, prm)
    with pytest.raises(RuntimeError, match="image"):
        A.apply(img.float(), lab, prm)
    with pytest.raises(RuntimeError, match="image"):
        A.apply(img[:, :, :4], lab, prm)
    with pytest.raises(RuntimeError, match="params"):
        A.apply(img, lab, (prm.fwd, prm.inv, prm.color))
    with pytest.raises(RuntimeError, match="params"):
        A.apply(img, lab, A.AugmentParams(prm.fwd, prm.inv.float(), prm.color))
    with pytest.raises(RuntimeError, match="params"):
        A.apply(img, lab, A.AugmentParams(prm.fwd, prm.inv[:1], prm.color))
    with pytest.raises(RuntimeError, match="background"):
        A.apply(img, lab, prm, background=torch.zeros(b, H, W + 1, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="background"):
        A.apply(img, lab, prm, background=torch.zeros(b, H, W, 3))
    with pytest.raises(RuntimeError, match="dtype"):
        A.apply(img, lab, prm, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="fill"):
        A.apply(img, lab, prm, fill=300)
    with pytest.raises(RuntimeError, match="std"):
        A.apply(img, lab, prm, std=(1, 0, 1))
    with pytest.raises(RuntimeError, match="mean"):
        A.apply(img, lab, prm, mean=(1, 2))
    with pytest.raises(RuntimeError, match="steps"):
        A.apply(img, lab, prm, steps=("blur",))
    with pytest.raises(RuntimeError, match="out must"):
        A.apply(img, lab, prm, out=(torch.zeros(b, 3, H, W + 1), torch.zeros(b, H, W, dtype=torch.uint8)))
    with pytest.raises(RuntimeError, match="out must"):
        A.apply(img, lab, prm, out=(torch.zeros(b, 3, H, W), torch.zeros(b, H, W, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="keypoints_2d"):
        A.augment_ground_truth(img, lab, kp[0], 1, state)
    with pytest.raises(RuntimeError, match="keypoints_2d"):
        A.transform_keypoints(torch.zeros(b, 9, 3), prm.fwd)
    with pytest.raises(RuntimeError, match="fwd"):
        A.transform_keypoints(torch.zeros(b, 9, 2), prm.fwd[:1])
    # transform_keypoints is plain torch: the forward map, x right and y down
    fwd = torch.tensor([[[0.0, -1.0, 5.0], [1.0, 0.0, -2.0]]], dtype=torch.float64)     # +90 degrees, then a shift
    out = A.transform_keypoints(torch.tensor([[[1.0, 0.0], [0.0, 1.0]]]), fwd)
    assert out.dtype == torch.float64 and out.tolist() == [[[5.0, -1.0], [4.0, -2.0]]]
