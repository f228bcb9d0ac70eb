"""CPU-side checks of libpvloss.so (include/pvloss.h): it builds for gfx950, exports exactly its
header, and rejects bad arguments on the host."""
import ctypes
import os
import re

import pytest

from tests.test_build_table import exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_loss_backward", "pv_loss_forward", "pv_loss_workspace_size"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _loss_lib
    build.build()
    return _loss_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    loss = build.LIBS["loss"]
    assert loss.out == os.path.join(REPO, "pvnet_amd", "libpvloss.so")
    assert loss.hdr == os.path.join(REPO, "include", "pvloss.h")
    assert [os.path.basename(s) for s in loss.srcs] == ["pvloss.hip"]
    assert set(build.closure(loss.srcs)) == {*loss.srcs, loss.hdr}
    assert b"gfx950" in open(loss.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    # the translation unit includes nothing else of csrc/, and no floating-point atomic
    src = open(loss.srcs[0]).read()
    assert [i for i in re.findall(r'#include "([^"]+)"', src)] == ["../../include/pvloss.h"]
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    assert not re.search(r"__expf|__logf|__fdividef|atomicAdd\(\s*\(?(float|double)", src)
    # the reference functions the header replaces are named in it
    hdr = open(loss.hdr).read()
    for name in ("smooth_l1_loss", "compute_precision_recall", "CrossEntropyLoss", "net_utils.py", "train_linemod.py"):
        assert name in hdr, name


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _loss_lib
    assert header_functions("pvloss.h") == NAMES
    assert exported(build.LIBS["loss"].out) == set(NAMES)
    assert {n for n, _, _ in _loss_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_loss_lib.py"


def test_header_constants_match_binding():
    from pvnet_amd import _loss_lib as P, _render_lib
    src = open(os.path.join(REPO, "include", "pvloss.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    assert (defs["PV_LOSS_LABEL_I64"], defs["PV_LOSS_LABEL_U8"], defs["PV_LOSS_LABEL_I32"]) == \
        (P.PV_LOSS_LABEL_I64, P.PV_LOSS_LABEL_U8, P.PV_LOSS_LABEL_I32) == \
        (_render_lib.PV_LABEL_I64, _render_lib.PV_LABEL_U8, _render_lib.PV_LABEL_I32)
    assert (defs["PV_LOSS_F32"], defs["PV_LOSS_F16"]) == (P.PV_LOSS_F32, P.PV_LOSS_F16) == \
        (_render_lib.PV_FIELD_F32, _render_lib.PV_FIELD_F16)
    assert defs["PV_LOSS_PIXELS"] == P.PV_LOSS_PIXELS == 8
    assert defs["PV_LOSS_THREADS"] == P.PV_LOSS_THREADS == 256
    assert defs["PV_LOSS_MAX_DIM"] == P.PV_LOSS_MAX_DIM == 2 ** 20
    assert defs["PV_LOSS_MAX_CLASSES"] == P.PV_LOSS_MAX_CLASSES == 1024
    assert defs["PV_LOSS_MAX_CHUNKS"] == P.PV_LOSS_MAX_CHUNKS == 8
    # a forward block's LDS (the f64 tree and 12 bytes a class) stays far below a CU's 160 KiB
    assert P.PV_LOSS_THREADS * 8 + 12 * P.PV_LOSS_MAX_CLASSES <= 64 * 1024
    # the structures are the header's
    assert ctypes.sizeof(P.LossDesc) == 4 * 8 + 17 * 8 + 9 * 4 + 4 == 208
    assert P.LossDesc.seg_strides.offset == 32 and P.LossDesc.vertex_strides.offset == 64
    assert P.LossDesc.target_strides.offset == 104 and P.LossDesc.label_strides.offset == 144
    assert P.LossDesc.seg_kind.offset == 168 and P.LossDesc.b.offset == 184 and P.LossDesc.sigma.offset == 204
    assert ctypes.sizeof(P.LossOut) == 4 * 8
    assert ctypes.sizeof(P.LossGrad) == 5 * 8 + 9 * 8
    assert P.LossGrad.grad_seg_strides.offset == 40 and P.LossGrad.grad_vertex_strides.offset == 72


def test_workspace_size(lib):
    from pvnet_amd._loss_lib import PV_LOSS_MAX_CHUNKS as P_MAX_CHUNKS
    f = lib.pv_loss_workspace_size
    assert f(-1, 8, 8, 1) == 0 and f(1, 0, 8, 1) == 0 and f(1, 8, 0, 1) == 0 and f(1, -8, 8, 1) == 0
    assert f(1, 8, 2 ** 20 + 1, 1) == 0 and f(1, 8, 8, 0) == 0 and f(1, 8, 8, -1) == 0 and f(1, 8, 8, 1025) == 0
    assert f(2 ** 31 - 1, 2 ** 20, 2 ** 20, 1) == 0                   # more blocks than a grid holds
    base = f(1, 1, 1, 1)
    assert base > 0 and base % 256 == 0 and f(0, 8, 8, 1) > 0
    # per block of 256 lanes x 8 pixels one partial of each kind (one per chunk for the vector field): it
    # grows with b H W, and with ncls
    per_block = 8 + 8 * P_MAX_CHUNKS + 4 + 12
    assert f(32, 480, 640, 1) >= 32 * (480 * 640 // 2048) * per_block
    assert f(1, 480, 640, 1) < f(2, 480, 640, 1) < f(2, 960, 640, 1) < f(2, 960, 1280, 1)
    assert f(2, 480, 640, 3) > f(2, 480, 640, 1)
    assert f(32, 480, 640, 1) < 1 << 20                                # and stays small


def test_argument_errors_without_device(lib):
    from pvnet_amd import _loss_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    big = 1 << 30
    H, W, C = 48, 64, 9

    def desc(ss=None, vs=None, ts=None, ls=None, **kw):
        d = dict(seg=p, vertex=p, target=p, label=p, seg_kind=P.PV_LOSS_F32, vertex_kind=P.PV_LOSS_F16,
                 target_kind=P.PV_LOSS_F32, label_kind=P.PV_LOSS_LABEL_U8, b=2, H=H, W=W, ncls=1, vn=C, sigma=1.0)
        d.update(kw)
        t = P.LossDesc(**d)
        t.seg_strides[:] = ss or (2 * H * W, H * W, W, 1)
        t.vertex_strides[:] = vs or (2 * C * H * W, W, 1, 2 * H * W, H * W)
        t.target_strides[:] = ts or (H * W * C * 2, W * C * 2, C * 2, 2, 1)
        t.label_strides[:] = ls or (H * W, W, 1)
        return t

    def outs(**kw):
        d = dict(loss_seg=p, loss_vertex=p, fg=p, counts=p)
        d.update(kw)
        return P.LossOut(**d)

    def grads(gs=None, gv=None, **kw):
        d = dict(g_seg=p, g_vertex=p, fg=p, grad_seg=p, grad_vertex=p)
        d.update(kw)
        t = P.LossGrad(**d)
        t.grad_seg_strides[:] = gs or (2 * H * W, H * W, W, 1)
        t.grad_vertex_strides[:] = gv or (2 * C * H * W, W, 1, 2 * H * W, H * W)
        return t

    def fwd(d=None, o=None, ws=p, nbytes=big, null=()):
        d, o = d or desc(), o or outs()
        return lib.pv_loss_forward(None if "d" in null else ctypes.byref(d), None if "o" in null else ctypes.byref(o),
                                   ws, nbytes, None)

    def bwd(d=None, g=None, null=()):
        d, g = d or desc(), g or grads()
        return lib.pv_loss_backward(None if "d" in null else ctypes.byref(d), None if "g" in null else ctypes.byref(g), None)

    def both(d):
        r = (fwd(d), bwd(d))
        assert r[0] == r[1], r
        return r[0]

    # NULL descriptors, both terms absent, a present term's inputs and outputs
    assert fwd(null=("d",)) == bwd(null=("d",)) == fwd(null=("o",)) == bwd(null=("g",)) == P.PV_EINVAL
    assert both(desc(seg=None, vertex=None)) == P.PV_EINVAL
    assert both(desc(seg=None, vertex=None, target=None)) == P.PV_EINVAL
    assert both(desc(label=None)) == P.PV_EINVAL and both(desc(target=None)) == P.PV_EINVAL
    assert fwd(o=outs(loss_seg=None)) == P.PV_EINVAL and fwd(o=outs(loss_vertex=None)) == P.PV_EINVAL
    for name in ("g_seg", "g_vertex", "fg", "grad_seg", "grad_vertex"):
        assert bwd(g=grads(**{name: None})) == P.PV_EINVAL, name
    # negative sizes, sizes out of range
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(H=-1), dict(W=-5), dict(H=2 ** 20 + 1), dict(W=2 ** 20 + 1),
               dict(ncls=0), dict(ncls=-2), dict(ncls=P.PV_LOSS_MAX_CLASSES + 1), dict(vn=0), dict(vn=-1),
               dict(ncls=1024, vn=1025)):
        assert both(desc(**kw)) == P.PV_EINVAL, kw
    # unknown kinds
    for kw in (dict(seg_kind=2), dict(seg_kind=-1), dict(vertex_kind=2), dict(vertex_kind=-1), dict(target_kind=7),
               dict(target_kind=-1), dict(label_kind=3), dict(label_kind=-1)):
        assert both(desc(**kw)) == P.PV_EINVAL, kw
    # sigma
    for s in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert both(desc(sigma=s)) == P.PV_EINVAL, s
    # negative strides
    for i in range(4):
        ss = [2 * H * W, H * W, W, 1]
        ss[i] = -1
        assert both(desc(ss=ss)) == P.PV_EINVAL
        assert bwd(g=grads(gs=ss)) == P.PV_EINVAL
    for i in range(5):
        vs = [H * W * C * 2, W * C * 2, C * 2, 2, 1]
        vs[i] = -2
        assert both(desc(vs=vs)) == P.PV_EINVAL and both(desc(ts=vs)) == P.PV_EINVAL
        assert bwd(g=grads(gv=vs)) == P.PV_EINVAL
    for i in range(3):
        ls = [H * W, W, 1]
        ls[i] = -1
        assert both(desc(ls=ls)) == P.PV_EINVAL
    # the workspace
    need = lib.pv_loss_workspace_size(2, H, W, 1)
    assert need > 0
    assert fwd(ws=None) == P.PV_EWORKSPACE and fwd(nbytes=need - 1) == P.PV_EWORKSPACE and fwd(nbytes=0) == P.PV_EWORKSPACE
    assert fwd(ws=264) == P.PV_EALIGN
    # alignment to the element
    assert both(desc(seg=258)) == P.PV_EALIGN and both(desc(vertex=257)) == P.PV_EALIGN and both(desc(target=258)) == P.PV_EALIGN
    assert both(desc(label=260, label_kind=P.PV_LOSS_LABEL_I64)) == P.PV_EALIGN
    assert both(desc(label=258, label_kind=P.PV_LOSS_LABEL_I32)) == P.PV_EALIGN
    assert fwd(o=outs(loss_seg=258)) == P.PV_EALIGN and fwd(o=outs(fg=260)) == P.PV_EALIGN and fwd(o=outs(counts=260)) == P.PV_EALIGN
    assert bwd(g=grads(g_seg=258)) == P.PV_EALIGN and bwd(g=grads(fg=260)) == P.PV_EALIGN
    assert bwd(g=grads(grad_seg=258)) == P.PV_EALIGN and bwd(g=grads(grad_vertex=257)) == P.PV_EALIGN
    # nothing to do: success, no launch, whatever the pointers
    assert both(desc(b=0)) == 0
    assert fwd(desc(b=0, seg=None, vertex=None, target=None, label=None), outs(loss_seg=None, loss_vertex=None, fg=None, counts=None),
               ws=None, nbytes=0) == 0
    assert bwd(desc(b=0, seg=None, vertex=None, target=None, label=None),
               grads(g_seg=None, g_vertex=None, fg=None, grad_seg=None, grad_vertex=None)) == 0
    assert both(desc(b=0, vn=0)) == P.PV_EINVAL and both(desc(b=0, sigma=0.0)) == P.PV_EINVAL


def test_python_layer_rejects_before_any_call():
    import torch
    import pvnet_amd
    from pvnet_amd import net_utils as N
    assert pvnet_amd.pvnet_loss is N.pvnet_loss and "pvnet_loss" in pvnet_amd.__all__
    b, H, W, vn = 2, 6, 8, 3
    seg, ver = torch.zeros(b, 2, H, W), torch.zeros(b, 2 * vn, H, W)
    lab, tgt = torch.zeros(b, H, W, dtype=torch.uint8), torch.zeros(b, H, W, vn, 2)
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="device"):
        N.pvnet_loss(seg, ver, lab, tgt)
    with pytest.raises(RuntimeError, match="device"):
        N.pvnet_loss(seg, ver, lab, tgt.permute(0, 3, 4, 1, 2).reshape(b, 2 * vn, H, W))
    with pytest.raises(RuntimeError, match="device"):
        N.smooth_l1_loss(ver, tgt, torch.ones(b, 1, H, W))
    with pytest.raises(RuntimeError, match="device"):
        N.compute_precision_recall(seg, lab)
    # wrong shapes and kinds, before the device is looked at
    with pytest.raises(RuntimeError, match="seg_pred"):
        N.pvnet_loss(torch.zeros(b, 3, H, W), ver, lab, tgt)
    with pytest.raises(RuntimeError, match="seg_pred"):
        N.pvnet_loss(seg.double(), ver, lab, tgt)
    with pytest.raises(RuntimeError, match="seg_pred"):
        N.pvnet_loss(seg, ver, lab, tgt, class_num=2)
    with pytest.raises(RuntimeError, match="vertex_pred"):
        N.pvnet_loss(seg, torch.zeros(b, 2 * vn, H, W + 1), lab, tgt)
    with pytest.raises(RuntimeError, match="vertex_pred"):
        N.pvnet_loss(seg, torch.zeros(b, 2 * vn + 1, H, W), lab, tgt)
    with pytest.raises(RuntimeError, match="vertex_target"):
        N.pvnet_loss(seg, ver, lab, torch.zeros(b, H, W, vn + 1, 2))
    with pytest.raises(RuntimeError, match="vertex_target"):
        N.pvnet_loss(seg, ver, lab, torch.zeros(b, H, W, vn, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="label"):
        N.pvnet_loss(seg, ver, lab.float(), tgt)
    with pytest.raises(RuntimeError, match="label"):
        N.pvnet_loss(seg, ver, lab[0], tgt)
    with pytest.raises(RuntimeError, match="sigma"):
        N.pvnet_loss(seg, ver, lab, tgt, sigma=0.0)
    with pytest.raises(RuntimeError, match="class_num"):
        N.pvnet_loss(seg, ver, lab, tgt, class_num=0)
    with pytest.raises(RuntimeError, match="both predictions"):
        N.pvnet_loss(seg, None, lab, tgt)
    with pytest.raises(RuntimeError, match="vertex_weights"):
        N.smooth_l1_loss(ver, tgt, torch.ones(b, H, W))
    with pytest.raises(NotImplementedError, match="normalize=False"):
        N.smooth_l1_loss(ver, tgt, torch.ones(b, 1, H, W), normalize=False)
