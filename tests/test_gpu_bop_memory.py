"""The memory contract of libpvbop.so's two entries, held through ctypes on guarded buffers
exactly as tests/test_gpu_memory_contract.py holds the other libraries': outputs and an exactly sized
workspace between patterned guards, the workspace prefilled with 0x00 / 0xFF / 0xA5, every input
surrounded by 0x00 and by 0xFF, all runs bit-identical, and the 0x00 run equal to tests/bop_ref.py.

Shapes: two chunks of 1024 vertices with the second one vertex long, and two symmetry tiles of 32
with the second one symmetry long, for a model that is the last of its table (a read past either
table's end would land in the surround); one pixel more than a block's 1024, the last pose on the
last image."""
import ctypes

import numpy as np
import pytest

from tests import bop_ref as R
from tests import render_ref as RR
from tests.test_gpu_memory_contract import Spec, contract, defines, untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built(device):
    import __graft_entry__ as g
    g.build()


def sym_case():
    rng = np.random.default_rng(41)
    models = [(rng.normal(size=(pn, 3)) * 0.05).astype(np.float32) for pn in (5, 1025)]
    syms = [np.eye(4)[None, :3]] + [np.stack([np.eye(4)[:3]] + [RR.pose(RR.random_rotation(rng), rng.normal(size=3) * 0.01)
                                                                 for _ in range(32)])]
    mid = np.array([1, 0, 1, 7], np.int32)                           # the last: outside the table
    Pg = np.stack([RR.pose(RR.random_rotation(rng), [0.01, -0.02, 0.7]) for _ in mid])
    Pe = np.stack([RR.pose(RR.random_rotation(rng), [0.02, -0.01, 0.75]) for _ in mid])
    K = np.stack([np.array([[572.4, 0.7, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]]) + i for i in range(len(mid))])
    return models, syms, mid, Pe, Pg, K


@pytest.mark.parametrize("metrics", [3, 1, 2])
def test_sym_errors_memory_contract(device, metrics):
    from pvnet_amd import _bop_lib as P
    L = P.load()
    d = defines("pvbop.h")
    assert (d["PV_BOP_MSSD"], d["PV_BOP_MSPD"], d["PV_BOP_NCOL"]) == (1, 2, 2)
    models, syms, mid, Pe, Pg, K = sym_case()
    b, max_pn, max_ns = len(mid), 1025, 33
    off = np.cumsum([0] + [len(m) for m in models]).astype(np.int32)
    soff = np.cumsum([0] + [len(s) for s in syms]).astype(np.int32)
    need = int(L.pv_bop_workspace_size(b, max_pn, max_ns))
    assert need == -(-b * 2 * max_ns * 16 // 256) * 256                  # chunks x symmetries x two columns of f64, to 256 bytes
    inputs = dict(pose_est=Pe, pose_gt=Pg, model=np.concatenate(models), model_off=off, model_id=mid,
                  syms=np.concatenate(syms), sym_off=soff, K=K)

    def call(ptr, ws, nbytes, stream):
        bt = P.BopBatch(b, int(off[-1]), int(soff[-1]), len(models), max_pn, max_ns, metrics, 0, ptr["pose_est"], ptr["pose_gt"],
                        ptr["model"], ptr["model_off"], ptr["model_id"], ptr["syms"], ptr["sym_off"], ptr["K"], 9)
        return L.pv_bop_sym_errors(ctypes.byref(bt), ptr["err"], ptr["best"], ws, nbytes, stream)

    spec = Spec("pv_bop_sym_errors", inputs, dict(err=((b, 2), np.float64), best=((b, 2), np.int32)), call, P.check, ws=need)

    def parity(base):
        names = [m for m, bit in (("mssd", 1), ("mspd", 2)) if metrics & bit]
        err, best = R.sym_errors(models, syms, Pe, Pg, K, mid, metrics=names)
        for c, bit in ((0, 1), (1, 2)):
            if metrics & bit:
                np.testing.assert_array_equal(base["err"][:, c].view(np.uint64), err[:, c].view(np.uint64))
                np.testing.assert_array_equal(base["best"][:, c], best[:, c])
                assert np.isnan(base["err"][3, c]) and np.isfinite(base["err"][:3, c]).all()
            else:
                assert untouched(base["err"][:, c]) and untouched(base["best"][:, c])

    contract(device, spec, parity)


@pytest.mark.parametrize("ntau", [1, 32])
def test_vsd_memory_contract(device, ntau):
    from pvnet_amd import _bop_lib as P
    L = P.load()
    assert defines("pvbop.h")["PV_BOP_MAX_TAUS"] == 32
    rng = np.random.default_rng(43)
    H, W, b, n_img = 25, 41, 3, 2                                        # 1025 pixels: a second block of one pixel
    K = np.array([[90.0, 0.0, 20.3], [0.0, 88.0, 12.1], [0.0, 0.0, 1.0]])

    def surface(shift):
        y, x = np.mgrid[:H, :W]
        z = 0.5 + 0.002 * ((x + shift) % 7) + 0.001 * y
        return np.where((x - 20 - shift) ** 2 + (y - 12) ** 2 < 150, z, np.inf).astype(np.float32)

    dg = np.stack([surface(0), surface(2), surface(-3)])
    de = np.stack([surface(1), surface(3), surface(4)])
    de[:, -1, -1] = dg[:, -1, -1] = 0.52                                 # the last pixel is in every count
    sensor = np.where(rng.random((n_img, H, W)) < 0.2, 0.0, 0.51 + 0.01 * rng.random((n_img, H, W))).astype(np.float32)
    img_id = np.array([0, 1, 1], np.int32)                               # the last pose reads the last image
    taus = np.sort(rng.random((b, ntau)) * 0.01, 1)
    inputs = dict(depth_test=sensor, img_id=img_id, depth_est=de, depth_gt=dg, K=K, taus=taus)

    def call(ptr, ws, nbytes, stream):
        bt = P.VsdBatch(b, n_img, H, W, ntau, 0, ptr["depth_test"], ptr["img_id"], ptr["depth_est"], ptr["depth_gt"], ptr["K"], 0,
                        0.015, ptr["taus"])
        return L.pv_bop_vsd(ctypes.byref(bt), ptr["counts"], ptr["err"], stream)

    spec = Spec("pv_bop_vsd", inputs, dict(counts=((b, 2 + ntau), np.int64), err=((b, ntau), np.float64)), call, P.check)

    def parity(base):
        counts, err = R.vsd(sensor, de, dg, K, 0.015, taus, img_id)
        np.testing.assert_array_equal(base["counts"], counts)
        np.testing.assert_array_equal(base["err"].view(np.uint64), err.view(np.uint64))
        assert (counts[:, 1] > 0).all() and (counts[:, 0] > counts[:, 1]).all()

    contract(device, spec, parity)
