"""CPU-side checks of libpvmodel.so (include/pvmodel.h): it builds for gfx950, exports exactly its
header, and rejects bad arguments on the host."""
import ctypes
import os
import re

import pytest

from tests import model_ref as M
from tests.test_build_table import exported, header_functions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pv_farthest_points", "pv_model_diameter", "pv_model_extent", "pv_model_workspace_size"]


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _model_lib
    build.build()
    return _model_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    model = build.LIBS["model"]
    assert model.out == os.path.join(REPO, "pvnet_amd", "libpvmodel.so")
    assert model.hdr == os.path.join(REPO, "include", "pvmodel.h")
    assert [os.path.basename(s) for s in model.srcs] == ["pvmodel.hip"]
    assert set(build.closure(model.srcs)) == {*model.srcs, model.hdr}
    assert b"gfx950" in open(model.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()
    # the translation unit includes nothing else of csrc/
    src = open(model.srcs[0]).read()
    assert [i for i in re.findall(r'#include "([^"]+)"', src)] == ["../../include/pvmodel.h"]
    assert "-ffp-contract=off" in build.HIPCC_FLAGS


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _model_lib
    assert header_functions("pvmodel.h") == NAMES
    assert exported(build.LIBS["model"].out) == set(NAMES)
    assert {n for n, _, _ in _model_lib.SIGNATURES} == set(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} has no ctypes signature in pvnet_amd/_model_lib.py"


def test_header_constants_match_binding():
    from pvnet_amd import _model_lib as P
    src = open(os.path.join(REPO, "include", "pvmodel.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)\)?[ \t]*(?:/\*|\n)", src)}
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    assert defs["PV_MODEL_SUM_LANES"] == P.PV_MODEL_SUM_LANES == M.SUM_LANES == 256
    assert defs["PV_MODEL_MAX_K"] == P.PV_MODEL_MAX_K == M.MAX_K == 1024
    assert defs["PV_MODEL_BLOCK_MAX_PN"] == P.PV_MODEL_BLOCK_MAX_PN == M.BLOCK_MAX_PN
    assert defs["PV_MODEL_CHUNK"] == P.PV_MODEL_CHUNK == M.CHUNK
    assert defs["PV_MODEL_TILE"] == P.PV_MODEL_TILE == M.TILE
    # the block form's LDS (12 bytes a point and the reduction slots) fits a CU's 160 KiB
    assert P.PV_MODEL_BLOCK_MAX_PN * 12 + 512 <= 160 * 1024 and P.PV_MODEL_BLOCK_MAX_PN % 1024 == 0
    assert (defs["PV_FPS_START_CENTROID"], defs["PV_FPS_START_CENTROID_KEPT"], defs["PV_FPS_START_INDEX"]) == \
        (P.PV_FPS_START_CENTROID, P.PV_FPS_START_CENTROID_KEPT, P.PV_FPS_START_INDEX) == \
        (M.START_CENTROID, M.START_CENTROID_KEPT, M.START_INDEX) == (0, 1, 2)
    assert ctypes.sizeof(P.ModelPoints) == 2 * 8 + 4 * 4
    assert P.ModelPoints.nmodels.offset == 16 and P.ModelPoints.max_pn.offset == 24


def test_workspace_size(lib):
    f = lib.pv_model_workspace_size
    assert f(-1, 8, 1) == 0 and f(1, -8, 1) == 0 and f(1, 8, 0) == 0 and f(1, 8, -1) == 0 and f(1, 8, 1025) == 0
    base = f(1, 0, 1)
    assert base > 0 and base % 256 == 0 and f(0, 0, 1) > 0
    assert f(1, 100000, 8) >= 100000 * 8                            # one running minimum per point
    assert f(3, 100000, 8) > f(1, 100000, 8) and f(1, 100000, 1024) == f(1, 100000, 1)


def test_argument_errors_without_device(lib):
    from pvnet_amd import _model_lib as P
    p = 256     # any non-NULL, 256-byte aligned value: rejected calls touch no pointer
    big = 1 << 30

    def points(**kw):
        d = dict(points=p, off=p, nmodels=2, total=100, max_pn=60, reserved_=0)
        d.update(kw)
        return P.ModelPoints(**d)

    def fps(d=None, k=8, start=P.PV_FPS_START_CENTROID, sidx=None, idx=p, picked=p, pd2=p, ws=p, nbytes=big, null=False):
        d = d or points()
        return lib.pv_farthest_points(None if null else ctypes.byref(d), k, start, sidx, idx, picked, pd2, ws, nbytes, None)

    def ext(d=None, bbox=p, cen=p, cnt=p, null=False):
        d = d or points()
        return lib.pv_model_extent(None if null else ctypes.byref(d), bbox, cen, cnt, None)

    def dia(d=None, out=p, ws=p, nbytes=big, null=False):
        d = d or points()
        return lib.pv_model_diameter(None if null else ctypes.byref(d), out, ws, nbytes, None)

    # NULL descriptor, NULL outputs and inputs
    assert fps(null=True) == ext(null=True) == dia(null=True) == P.PV_EINVAL
    assert fps(idx=None) == P.PV_EINVAL and dia(out=None) == P.PV_EINVAL
    assert ext(bbox=None, cen=None, cnt=None) == P.PV_EINVAL
    for kw in (dict(points=None), dict(off=None)):
        assert fps(points(**kw)) == ext(points(**kw)) == dia(points(**kw)) == P.PV_EINVAL, kw
    # negative sizes and max_pn
    for kw in (dict(nmodels=-1), dict(total=-1), dict(max_pn=-1), dict(nmodels=-3, total=-3)):
        assert fps(points(**kw)) == ext(points(**kw)) == dia(points(**kw)) == P.PV_EINVAL, kw
    # k and start
    for k in (0, -1, P.PV_MODEL_MAX_K + 1):
        assert fps(k=k) == P.PV_EINVAL, k
    for s in (-1, 3, 99):
        assert fps(start=s) == P.PV_EINVAL, s
    assert fps(start=P.PV_FPS_START_INDEX, sidx=None) == P.PV_EINVAL
    # the workspace
    need = lib.pv_model_workspace_size(2, 100, 8)
    assert need > 0 and lib.pv_model_workspace_size(2, 100, 1) == need
    assert fps(ws=None) == dia(ws=None) == P.PV_EWORKSPACE
    assert fps(nbytes=need - 1) == dia(nbytes=need - 1) == P.PV_EWORKSPACE
    assert fps(nbytes=0) == dia(nbytes=0) == P.PV_EWORKSPACE
    assert fps(ws=264) == dia(ws=264) == P.PV_EALIGN
    assert fps(picked=260) == P.PV_EALIGN and fps(idx=258) == P.PV_EALIGN and dia(out=260) == P.PV_EALIGN
    assert ext(cen=260) == P.PV_EALIGN and ext(cnt=258) == P.PV_EALIGN
    # a model too large for the diameter's grid
    assert dia(points(total=2 ** 31 - 1, max_pn=2 ** 31 - 1)) == P.PV_EINVAL
    # nothing to do: success, no launch, whatever the pointers
    empty = dict(nmodels=0, total=0, max_pn=0)
    assert fps(points(**empty)) == ext(points(**empty)) == dia(points(**empty)) == 0
    assert fps(points(points=None, off=None, **empty), idx=None, picked=None, pd2=None, ws=None, nbytes=0) == 0
    assert ext(points(points=None, off=None, **empty), bbox=None, cen=None, cnt=None) == 0
    assert dia(points(points=None, off=None, **empty), out=None, ws=None, nbytes=0) == 0
    assert fps(points(**empty), k=0) == P.PV_EINVAL and fps(points(**empty), start=7) == P.PV_EINVAL


def test_python_layer_rejects_before_any_call():
    import numpy as np
    import pvnet_amd
    from pvnet_amd import evaluation_utils as EU
    from pvnet_amd import models as Mo
    from pvnet_amd import render as Rn
    for name in ("extent", "farthest_points", "diameter", "corners_3d", "keypoints_3d"):
        assert getattr(pvnet_amd, name) is getattr(Mo, name)
    assert callable(EU.ModelTable.from_meshes)
    t = Rn.MeshTable([(np.zeros((8, 3), np.float32), np.zeros((12, 3), np.int32))], device="cpu")
    for call in (lambda: Mo.extent(t), lambda: Mo.diameter(t), lambda: Mo.farthest_points(t, 8),
                 lambda: Mo.corners_3d(t), lambda: Mo.keypoints_3d(t), lambda: EU.ModelTable.from_meshes(t)):
        with pytest.raises(RuntimeError, match="device"):
            call()
    with pytest.raises(RuntimeError, match="MeshTable or a ModelTable"):
        Mo.extent(object())
    with pytest.raises(ValueError, match="symmetric"):
        EU.ModelTable.from_meshes(t, symmetric=[True, False])
