"""CPU-side checks of libpvpose.so (include/pvpose.h): it builds for gfx950, exports exactly its
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
    from pvnet_amd import build, _pose_lib
    build.build()
    return _pose_lib.load()


def test_library_builds_for_gfx950(lib):
    from pvnet_amd import build
    pose = build.LIBS["pose"]
    assert pose.out == os.path.join(REPO, "pvnet_amd", "libpvpose.so")
    assert pose.hdr == os.path.join(REPO, "include", "pvpose.h")
    assert [os.path.basename(s) for s in pose.srcs] == ["pvepnp.hip"]
    assert b"gfx950" in open(pose.out, "rb").read()
    assert build.build() == build.LIBS["vote"].out and not build.needs_build()


def test_exports_exactly_the_header(lib):
    from pvnet_amd import build, _pose_lib
    names = header_functions("pvpose.h")
    assert names == ["pv_epnp", "pv_rt6_to_Rt"]
    assert exported(build.LIBS["pose"].out) == set(names)
    bound = {n for n, _, _ in _pose_lib.SIGNATURES}
    for n in names:
        assert hasattr(lib, n) and n in bound, f"{n} has no ctypes signature in pvnet_amd/_pose_lib.py"


def test_header_constants_match_binding():
    from pvnet_amd import _pose_lib as P
    src = open(os.path.join(REPO, "include", "pvpose.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z_]+) \(?(-?\d+)\)?", src)}
    assert (defs["PV_EPNP_OK"], defs["PV_EPNP_DEGENERATE"]) == (P.PV_EPNP_OK, P.PV_EPNP_DEGENERATE) == (0, 1)
    assert (defs["PV_EPNP_MIN_POINTS"], defs["PV_EPNP_MAX_POINTS"]) == (P.PV_EPNP_MIN_POINTS, P.PV_EPNP_MAX_POINTS) == (6, 64)
    assert (defs["PV_OK"], defs["PV_EINVAL"], defs["PV_EWORKSPACE"], defs["PV_EALIGN"]) == \
        (0, P.PV_EINVAL, P.PV_EWORKSPACE, P.PV_EALIGN)
    # the batch structure is the header's: two int32, four pointers, two int64
    assert ctypes.sizeof(P.EpnpBatch) == 8 + 4 * 8 + 2 * 8 and ctypes.sizeof(P.EpnpDiag) == 3 * 8
    assert P.EpnpBatch.pts3d_stride.offset == 40 and P.EpnpBatch.K.offset == 32


def test_argument_errors_without_device(lib):
    from pvnet_amd import _pose_lib as P
    p = 256     # any non-NULL value: rejected calls touch no pointer

    def batch(**kw):
        d = dict(b=2, pn=9, pts2d=p, pts2d64=None, pts3d=p, K=p, pts3d_stride=0, K_stride=0)
        d.update(kw)
        return P.EpnpBatch(**d)

    def call(bt, Rt=p, rt6=p, diag=None):
        return lib.pv_epnp(ctypes.byref(bt) if bt is not None else None, Rt, rt6, diag, None)

    assert call(None) == P.PV_EINVAL
    assert call(batch(b=-1)) == P.PV_EINVAL
    for pn in (-1, 0, 4, 5, 65, 1 << 20):
        assert call(batch(pn=pn)) == P.PV_EINVAL
    assert call(batch(pts2d=None)) == P.PV_EINVAL            # both point pointers NULL
    assert call(batch(pts3d=None)) == P.PV_EINVAL
    assert call(batch(K=None)) == P.PV_EINVAL
    assert call(batch(), Rt=None, rt6=None) == P.PV_EINVAL
    assert call(batch(pts3d_stride=-27)) == P.PV_EINVAL
    assert call(batch(K_stride=-9)) == P.PV_EINVAL
    # nothing to do: success, no launch
    assert call(batch(b=0)) == 0
    assert call(batch(b=0, pts2d=None, pts3d=None, K=None), Rt=None, rt6=None) == 0
    assert call(batch(b=0, pn=5)) == P.PV_EINVAL
    f = lib.pv_rt6_to_Rt
    assert f(p, p, -1, None) == P.PV_EINVAL
    assert f(None, p, 1, None) == P.PV_EINVAL and f(p, None, 1, None) == P.PV_EINVAL
    assert f(p, p, 0, None) == 0 and f(None, None, 0, None) == 0


def test_python_layer_rejects_host_tensors_and_few_points():
    import torch
    from pvnet_amd import extend_utils as X
    K = np.eye(3)
    with pytest.raises(RuntimeError, match="device"):
        X.pnp_batch(torch.zeros(1, 9, 2), np.zeros((9, 3)), K)
    with pytest.raises(ValueError, match="method"):
        X.pnp_batch(torch.zeros(1, 9, 2), np.zeros((9, 3)), K, method="p3p")
    for pn in (4, 5, 65):
        with pytest.raises(RuntimeError, match="p3p_lm"):
            X.pnp_batch(_fake_device_points(pn), np.zeros((pn, 3)), K)


def _fake_device_points(pn):
    """A tensor whose device says "cuda" without a device: the point count is checked before anything is touched."""
    class T:
        device = type("D", (), {"type": "cuda"})()
        shape = (1, pn, 2)

        def dim(self):
            return 3
    return T()


def test_evaluator_rejects_unknown_method():
    import torch
    from pvnet_amd.evaluation_utils import Evaluator, ModelTable
    t = ModelTable([(np.zeros((4, 3)), 1.0, False)], device="cpu")
    ev = Evaluator(t, np.zeros((9, 3)))
    with pytest.raises(ValueError, match="method"):
        ev.evaluate(torch.zeros(1, 9, 2), torch.zeros(1, 3, 4), None, np.eye(3), method="epnp_ransac")
