"""CPU-side checks of libpvrender.so (include/pvrender.h): it builds for gfx950, exports exactly its
header, and rejects bad arguments on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_build_table import exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _render_lib
    build.build()
    return _render_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    render = build.LIBS["render"]
    assert render.out == os.path.join(REPO, "pvnet_amd", "libpvrender.so")
    assert render.hdr == os.path.join(REPO, "include", "pvrender.h")
    assert [os.path.basename(s) for s in render.srcs] == ["pvrender.hip"]
    assert set(build.closure(render.srcs)) == {*render.srcs, render.hdr}
    assert b"gfx950" in open(render.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _render_lib
    names = header_functions("pvrender.h")
    assert names == ["pv_render_labels", "pv_render_workspace_size", "pv_vertex_field"]
    assert exported(build.LIBS["render"].out) == set(names)
    bound = {n for n, _, _ in _render_lib.SIGNATURES}
    assert bound == set(names)
    for n in names:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_render_lib.py"


def test_header_constants_match_binding():
    from pvnet_amd import _lib, _render_lib as P
    src = open(os.path.join(REPO, "include", "pvrender.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    assert (defs["PV_LABEL_I64"], defs["PV_LABEL_U8"], defs["PV_LABEL_I32"]) == \
        (P.PV_LABEL_I64, P.PV_LABEL_U8, P.PV_LABEL_I32) == (_lib.PV_MASK_I64, _lib.PV_MASK_U8, _lib.PV_MASK_I32)
    assert (defs["PV_FIELD_F32"], defs["PV_FIELD_F16"]) == (P.PV_FIELD_F32, P.PV_FIELD_F16) == \
        (_lib.PV_VERTEX_F32, _lib.PV_VERTEX_F16)
    assert (defs["PV_KP_F64"], defs["PV_KP_F32"]) == (P.PV_KP_F64, P.PV_KP_F32) == (0, 1)
    assert defs["PV_RENDER_SUBPIXEL_BITS"] == P.PV_RENDER_SUBPIXEL_BITS == 8
    assert defs["PV_RENDER_MAX_SNAP"] == P.PV_RENDER_MAX_SNAP == 2 ** 29
    assert defs["PV_RENDER_MAX_DIM"] == P.PV_RENDER_MAX_DIM == 2 ** 20
    assert "#define PV_RENDER_SNAP_INVALID (-2147483647 - 1)" in src and P.PV_RENDER_SNAP_INVALID == -2 ** 31
    # the structures are the header's
    assert ctypes.sizeof(P.RenderMeshes) == 4 * 8 + 6 * 4
    assert P.RenderMeshes.nmodels.offset == 32 and P.RenderMeshes.max_faces.offset == 48
    assert ctypes.sizeof(P.RenderBatch) == 6 * 4 + 5 * 8 + 8 + 8
    assert P.RenderBatch.inst_off.offset == 24 and P.RenderBatch.K_stride.offset == 64 and P.RenderBatch.znear.offset == 72
    assert ctypes.sizeof(P.RenderOut) == 6 * 8
    assert ctypes.sizeof(P.FieldDesc) == 3 * 8 + 8 * 8 + 8 * 4
    assert P.FieldDesc.label_strides.offset == 24 and P.FieldDesc.vertex_strides.offset == 48
    assert P.FieldDesc.label_kind.offset == 88 and P.FieldDesc.vn.offset == 116


def test_workspace_size(lib):
    f = lib.pv_render_workspace_size
    assert f(0, 8, 8, 0, 0) == 0 and f(-1, 8, 8, 0, 0) == 0
    assert f(1, 0, 8, 0, 0) == 0 and f(1, 8, -3, 0, 0) == 0 and f(1, 8, 2 ** 20 + 1, 0, 0) == 0
    assert f(1, 8, 8, -1, 0) == 0 and f(1, 8, 8, 0, -1) == 0
    base = f(1, 1, 1, 0, 0)
    assert base > 0 and base % 256 == 0
    assert f(2, 48, 64, 0, 0) >= 2 * 48 * 64 * 8                     # one 64-bit key per pixel
    assert f(2, 48, 64, 1000, 4) >= 2 * 48 * 64 * 8 + 1000 * 16      # and 16 bytes per projected vertex
    assert f(2, 48, 64, 1000, 4) > f(2, 48, 64, 1000, 0)


def test_render_argument_errors_without_device(lib):
    from pvnet_amd import _render_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    big = 1 << 30

    def meshes(**kw):
        d = dict(verts=p, vert_off=p, faces=p, face_off=p, nmodels=1, total_v=8, total_f=12, max_verts=8,
                 max_faces=12, reserved_=0)
        d.update(kw)
        return P.RenderMeshes(**d)

    def batch(**kw):
        d = dict(b=2, H=48, W=64, ninst=1, total_inst=2, label_kind=P.PV_LABEL_U8, inst_off=None, model_id=p,
                 label=p, pose=p, K=p, K_stride=0, znear=1e-3)
        d.update(kw)
        return P.RenderBatch(**d)

    def outs(**kw):
        d = dict(label=p, inst=p, depth=p, snap_xy=None, snap_z=None, won=None)
        d.update(kw)
        return P.RenderOut(**d)

    def call(m=None, bt=None, o=None, ws=p, nbytes=big, null=()):
        m, bt, o = m or meshes(), bt or batch(), o or outs()
        args = [None if "m" in null else ctypes.byref(m), None if "bt" in null else ctypes.byref(bt),
                None if "o" in null else ctypes.byref(o)]
        return lib.pv_render_labels(*args, ws, nbytes, None)

    for null in ("m", "bt", "o"):
        assert call(null=(null,)) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(ninst=-1), dict(total_inst=-2), dict(K_stride=-9)):
        assert call(bt=batch(**kw)) == P.PV_EINVAL, kw
    for kw in (dict(H=0), dict(W=0), dict(H=-4), dict(W=-1), dict(W=2 ** 20 + 1)):
        assert call(bt=batch(**kw)) == P.PV_EINVAL, kw
    for z in (0.0, -1.0, float("nan"), -float("inf")):
        assert call(bt=batch(znear=z)) == P.PV_EINVAL, z
    for kw in (dict(nmodels=-1), dict(total_v=-1), dict(total_f=-1), dict(max_verts=-1), dict(max_faces=-1)):
        assert call(m=meshes(**kw)) == P.PV_EINVAL, kw
    assert call(m=meshes(nmodels=0)) == P.PV_EINVAL                    # instances, but no model
    for kind in (-1, 3, 99):
        assert call(bt=batch(label_kind=kind)) == P.PV_EINVAL
    assert call(bt=batch(total_inst=3)) == P.PV_EINVAL                 # not b * ninst, and no inst_off
    assert call(o=outs(label=None, inst=None, depth=None)) == P.PV_EINVAL
    assert call(o=outs(label=None, inst=None, depth=None, won=p, snap_xy=p)) == P.PV_EINVAL
    for name in ("model_id", "label", "pose", "K"):
        assert call(bt=batch(**{name: None})) == P.PV_EINVAL, name
    for name in ("verts", "vert_off", "faces", "face_off"):
        assert call(m=meshes(**{name: None})) == P.PV_EINVAL, name
    # the workspace
    need = lib.pv_render_workspace_size(2, 48, 64, 2 * 8, 2)
    assert need > 0
    assert call(ws=None) == P.PV_EWORKSPACE
    assert call(nbytes=need - 1) == P.PV_EWORKSPACE and call(nbytes=0) == P.PV_EWORKSPACE
    assert call(ws=264) == P.PV_EALIGN
    assert call(bt=batch(pose=260)) == P.PV_EALIGN
    # nothing to do: success, no launch, whatever the pointers
    assert call(bt=batch(b=0, total_inst=0)) == 0
    assert call(bt=batch(b=0, total_inst=0, model_id=None, pose=None, K=None), o=outs(label=None, inst=None, depth=None),
                ws=None, nbytes=0) == 0
    assert call(bt=batch(b=0, total_inst=0, H=0)) == P.PV_EINVAL


def test_field_argument_errors_without_device(lib):
    from pvnet_amd import _render_lib as P
    p = 256

    def desc(ls=(48 * 64, 64, 1), vs=(48 * 64 * 18, 64 * 18, 18, 2, 1), **kw):
        d = dict(label=p, keypoints=p, vertex=p, label_kind=P.PV_LABEL_U8, kp_kind=P.PV_KP_F64,
                 vertex_kind=P.PV_FIELD_F32, b=2, H=48, W=64, ncls=1, vn=9)
        d.update(kw)
        t = P.FieldDesc(**d)
        t.label_strides[:] = ls
        t.vertex_strides[:] = vs
        return t

    def call(d):
        return lib.pv_vertex_field(ctypes.byref(d) if d is not None else None, None)

    assert call(None) == P.PV_EINVAL
    for kw in (dict(b=-1), dict(H=0), dict(W=0), dict(H=-1), dict(ncls=0), dict(vn=0), dict(ncls=-2), dict(vn=-1),
               dict(label_kind=3), dict(label_kind=-1), dict(kp_kind=2), dict(vertex_kind=2), dict(vertex_kind=-1),
               dict(label=None), dict(keypoints=None), dict(vertex=None)):
        assert call(desc(**kw)) == P.PV_EINVAL, kw
    for i in range(3):
        ls = [48 * 64, 64, 1]
        ls[i] = -1
        assert call(desc(ls=ls)) == P.PV_EINVAL
    for i in range(5):
        vs = [48 * 64 * 18, 64 * 18, 18, 2, 1]
        vs[i] = -2
        assert call(desc(vs=vs)) == P.PV_EINVAL
    assert call(desc(keypoints=264)) == P.PV_EALIGN and call(desc(vertex=258)) == P.PV_EALIGN
    assert call(desc(b=0)) == 0 and call(desc(b=0, label=None, keypoints=None, vertex=None)) == 0
    assert call(desc(b=0, vn=0)) == P.PV_EINVAL


def test_python_layer_rejects_before_any_call():
    import torch
    from pvnet_amd import render as Rn
    import pvnet_amd
    assert pvnet_amd.render_labels is Rn.render_labels and pvnet_amd.MeshTable is Rn.MeshTable
    assert pvnet_amd.vertex_field is Rn.vertex_field and pvnet_amd.mask_iou is Rn.mask_iou
    assert pvnet_amd.render_ground_truth is Rn.render_ground_truth
    box = (np.zeros((8, 3), np.float32), np.zeros((12, 3), np.int32))
    t = Rn.MeshTable([box], device="cpu")
    assert (t.nmodels, t.total_v, t.total_f, t.max_verts, t.max_faces) == (1, 8, 12, 8, 12)
    assert t.faces.dtype == torch.int32 and t.verts.dtype == torch.float32 and t.vert_off.tolist() == [0, 8]
    with pytest.raises(ValueError):
        Rn.MeshTable([])
    with pytest.raises(RuntimeError, match="device"):
        Rn.render_labels(t, torch.zeros(1, 1, 3, 4), [0], [1], np.eye(3), 8, 8)
    with pytest.raises(RuntimeError, match="device"):
        Rn.vertex_field(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 1, 9, 2), 1)
    with pytest.raises(RuntimeError, match="keypoints_2d"):
        Rn.vertex_field(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 2, 9, 2), 1)
    with pytest.raises(RuntimeError, match="label"):
        Rn.vertex_field(torch.zeros(1, 8, 8, dtype=torch.float32), torch.zeros(1, 1, 9, 2), 1)
    with pytest.raises(RuntimeError, match="shape"):
        Rn.mask_iou(torch.zeros(1, 8, 8), torch.zeros(1, 8, 9), 1)
    a = torch.tensor([[[0, 1, 1, 2]]])
    b = torch.tensor([[[1, 1, 0, 2]]])
    iou = Rn.mask_iou(a, b, 3)
    assert iou.dtype == torch.float64 and iou.shape == (1, 3)
    assert iou[0, 0] == 1 / 3 and iou[0, 1] == 1.0 and torch.isnan(iou[0, 2])
