"""The memory contract of libpvicp.so's entry, held through ctypes on guarded buffers exactly
as tests/test_gpu_memory_contract.py holds the other libraries': outputs and an exactly sized workspace
between patterned guards, the workspace prefilled with 0x00 / 0xFF / 0xA5, every input surrounded by
0x00 and by 0xFF, all runs bit-identical, and the 0x00 run equal to tests/icp_ref.py.

Shapes: 25 x 41 = 1025 pixels, one more than a block's 1024, so a second block of one pixel whose lane
0 alone has work, and a width that is no multiple of the lane run of 4; the object reaches the last
interior pixel; the last pose reads the last image.  One pose arrives converged (nothing of it may be
written, and its rows of the workspace are neither written nor read), one has an img_id outside the
images (its blocks must read no map)."""
import ctypes

import numpy as np
import pytest

from tests import icp_cases as C
from tests import icp_ref as R
from tests.test_gpu_memory_contract import Spec, contract, defines, untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built(device):
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("shape", [(25, 41), (17, 64), (3, 3)])
@pytest.mark.parametrize("with_neq", [True, False])
def test_iterate_memory_contract(device, shape, with_neq):
    from pvnet_amd import _icp_lib as P
    L = P.load()
    d = defines("pvicp.h")
    assert (d["PV_ICP_BLOCK"], d["PV_ICP_RUN"], d["PV_ICP_NSUM"], d["PV_ICP_CONVERGED"]) == (1024, 4, 28, 1)
    H, W = shape
    b, n_img = 4, 2
    de = np.stack([C.bumpy(H, W, shift=0.001 * i) for i in range(b)])
    dt = np.stack([C.bumpy(H, W, shift=0.003, tilt=0.002), C.bumpy(H, W, shift=-0.002, tilt=-0.003)])
    dt[1, H // 2, W // 2] = 0.0
    img_id = np.array([0, 1, 7, 1], np.int32)                             # the third: outside; the last pose on the last image
    K = np.stack([C.K_SKEW + np.diag([i, i, 0.0]) for i in range(b)])
    rng = np.random.default_rng(3)
    from tests import render_ref as RR
    poses = np.stack([RR.pose(RR.random_rotation(rng), [0.0, 0.01 * i, 0.7]) for i in range(b)])
    status0 = np.array([0, R.CONVERGED, 0, 0], np.int32)
    iters0 = np.array([0, 5, 0, 2], np.int32)
    par = {**C.BASE, "min_count": 1}
    need = int(L.pv_icp_workspace_size(b, H, W))
    nblk = -(-H * W // 1024)
    assert need == -(-b * nblk * (28 * 8 + 4) // 256) * 256
    inputs = dict(depth_test=dt, img_id=img_id, depth_est=de, K=K)
    outputs = dict(pose=((b, 3, 4), np.float64, 0, poses), status=((b,), np.int32, 0, status0), iters=((b,), np.int32, 0, iters0),
                   cnt=((b,), np.int32), stats=((b, 3), np.float64))
    if with_neq:
        outputs["neq"] = ((b, 28), np.float64)

    def call(ptr, ws, nbytes, stream):
        bt = P.IcpBatch(b, n_img, H, W, par["min_count"], 0, ptr["depth_test"], ptr["img_id"], ptr["depth_est"], ptr["K"], 9,
                        par["dist_max"], par["edge_max"], par["lam"], par["max_rot"], par["max_trans"], par["eps_rot"],
                        par["eps_trans"])
        so = P.IcpState(ptr["pose"], ptr["status"], ptr["iters"], ptr["cnt"], ptr["stats"], ptr.get("neq"))
        return L.pv_icp_iterate(ctypes.byref(bt), ctypes.byref(so), ws, nbytes, stream)

    spec = Spec("pv_icp_iterate", inputs, outputs, call, P.check, ws=need)

    def parity(base):
        st = R.new_state(poses)
        st["status"][:], st["iters"][:] = status0, iters0
        R.iterate(st, de, dt, K, img_id, **par)
        live = [0, 2, 3]
        for k in outputs:
            got, want = base[k][live], st[k][live]
            np.testing.assert_array_equal(got.view(np.uint64) if got.dtype == np.float64 else got, want.view(np.uint64)
                                          if want.dtype == np.float64 else want, err_msg=k)
        # the converged pose: its state as it came, its outputs never written
        np.testing.assert_array_equal(base["pose"][1], poses[1])
        assert base["status"][1] == R.CONVERGED and base["iters"][1] == 5
        assert untouched(base["cnt"][1]) and untouched(base["stats"][1]) and (not with_neq or untouched(base["neq"][1]))
        assert base["status"][2] == R.BAD_INPUT and np.isnan(base["stats"][2]).all()
        assert base["cnt"][3] == (H - 2) * (W - 2) - 1                  # every interior pixel but the sensor's hole
        if H > 3:
            assert base["status"][3] == R.RUNNING and base["iters"][3] == 3 and base["status"][0] == R.RUNNING

    contract(device, spec, parity)
