"""pv_epnp's arithmetic without a device: pvnet_amd/csrc/pvepnp_core.h compiled for the host
(tests/epnp_host.cpp; the kernel's lane phases become loops over the lanes) against tests/epnp_ref.py,
on the cases and at the tolerance of the device test (tests/test_gpu_epnp.py), and on the edge
families of tests/epnp_cases.py at the gates DESIGN 10c sets for them."""
import collections
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import epnp_cases as C
from tests import epnp_ref as E
from tests.test_pnp_oracle import K_LM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def build_host_form(directory):
    """Compile tests/epnp_host.cpp into `directory` -> run(p3, p2 (f64 or f32), K) -> dict."""
    from pvnet_amd import build
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cxx = [cxx] if cxx else [build.hipcc(), "-x", "c++"]      # hipcc's clang compiles plain C++ too
    so = os.path.join(str(directory), "libpvepnp_host.so")
    subprocess.check_call([*cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(REPO, "tests", "epnp_host.cpp")])
    f = ctypes.CDLL(so).pv_epnp_host
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 8

    def run(p3, p2, K):
        p3 = np.ascontiguousarray(p3, np.float64)
        K = np.ascontiguousarray(K, np.float64)
        p2 = np.ascontiguousarray(p2)
        Rt, rt6, ce, n = np.zeros((3, 4)), np.zeros(6), np.zeros(3), ctypes.c_int(0)
        f32 = p2.dtype == np.float32
        st = f(p3.shape[0], p3.ctypes.data, K.ctypes.data, p2.ctypes.data if f32 else None,
               None if f32 else p2.ctypes.data, Rt.ctypes.data, rt6.ctypes.data, ce.ctypes.data,
               ctypes.addressof(n))
        return dict(Rt=Rt, rt6=rt6, cand_err=ce, n_used=n.value, status=st)
    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_form(tmp_path_factory.mktemp("epnp_host"))


@pytest.mark.parametrize("pn", [6, 7, 9, 21, 63, 64])
def test_host_form_matches_reference(pn, host):
    from oracle.pnp import rodrigues_vec_to_mat
    rng = np.random.default_rng(pn)
    worst, compared = 0.0, 0
    for trial in range(12):
        p3 = E.cuboid_model() if (pn == 9 and trial % 2) else E.random_model(rng, pn)
        Rt = E.random_pose(rng, 3.0)
        p2 = E.project(Rt, p3, K_LM) + (0.0, 1.0, 3.0)[trial % 3] * rng.standard_normal((pn, 2))
        if trial % 4 == 3:
            p2 = p2.astype(np.float32)
        r, h = E.epnp(p3, p2.astype(np.float64), K_LM), host(p3, p2, K_LM)
        assert r["status"] == h["status"] == E.OK
        worst = max(worst, np.abs(h["Rt"] - r["Rt"]).max(), np.abs(h["cand_err"] - r["cand_err"]).max(),
                    np.abs(rodrigues_vec_to_mat(h["rt6"][:3]) - r["Rt"][:, :3]).max())
        s = np.sort(r["cand_err"])
        if s[1] - s[0] > max(1e-9 * s[1], TOL):      # the rule of tests/test_gpu_epnp.py, explained there
            compared += 1
            assert h["n_used"] == r["n_used"]
        if trial % 3 == 0 and p2.dtype == np.float64:
            assert np.abs(h["Rt"] - Rt).max() < 1e-9
    print(f"pn {pn}: worst host form vs reference {worst:.2e}; n_used compared on {compared} of 12 images")
    assert compared >= 1            # 8 of the 12 images are noisy: the comparison is not empty
    assert worst < TOL


def test_host_form_degenerate_inputs(host):
    rng = np.random.default_rng(5)
    p3 = E.cuboid_model()
    p2 = E.project(E.random_pose(rng), p3, K_LM)
    planar = p3.copy()
    planar[:, 2] = 0.01
    nan, inf = p2.copy(), p2.copy()
    nan[4, 1] = np.nan
    inf[0, 0] = np.inf
    for what, (m, q) in dict(planar=(planar, p2), nan=(p3, nan), inf=(p3, inf), zeros=(p3, np.zeros_like(p2)),
                             zeros32=(p3, np.zeros_like(p2, dtype=np.float32))).items():
        h = host(m, q, K_LM)
        assert h["status"] == E.DEGENERATE and E.epnp(m, q.astype(np.float64), K_LM)["status"] == E.DEGENERATE, what
        np.testing.assert_array_equal(h["Rt"], IDENT)
        np.testing.assert_array_equal(h["rt6"], np.zeros(6))


# ---------------------------------------------------------------------------- the edge families (tests/epnp_cases.py)
def host_results(host, name):
    f = C.family(name)
    return [host(f["p3"][i], f["p2"][i], f["K"][i]) for i in range(len(f["p3"]))]


@pytest.mark.parametrize("name", C.ALL_FAMILIES)
def test_host_form_on_the_edge_families(name, host):
    """C.check_family: exact data against the truth (1e-9) wherever the model is above the thin band;
    separated eigenvalues against the reference image by image (TOL, or max(TOL, 100 d) where the
    reference resolves no better), n_used where the reference's candidates are apart, +inf equal to
    +inf only; repeated eigenvalues under noise by the rms gate (the reference's basis in the
    eigenspace is LAPACK's, so no image-by-image comparison exists); the thin models' status and the
    degenerate answer bit for bit; the rotation vector in the theta family."""
    m = C.check_family(name, host_results(host, name))
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" if "ratio" not in k else f"{k} {v:.3f}" for k, v in m.items()))


def test_host_form_n_used_comparisons_are_not_empty(host):
    """Every winner N = 1, 2, 3 was compared with the reference's in at least 3 images, and a
    candidate at +inf with another one winning in at least 3."""
    count = collections.Counter()
    inf_and_winner = 0
    for name in C.ALL_FAMILIES:
        if C.is_repeated(name):
            continue
        gate = C.gates(name)
        got = host_results(host, name)
        for i, (r, _) in enumerate(C.traces(name)):
            s = np.sort(r["cand_err"])
            if r["status"] == E.OK and s[1] - s[0] > max(1e-9 * s[1], gate[i]):
                assert got[i]["n_used"] == r["n_used"]
                count[r["n_used"]] += 1
                if np.isinf(r["cand_err"]).any():
                    np.testing.assert_array_equal(np.isinf(got[i]["cand_err"]), np.isinf(r["cand_err"]))
                    inf_and_winner += 1
    print(f"n_used compared: N=1 {count[1]}, N=2 {count[2]}, N=3 {count[3]}; with a candidate at +inf {inf_and_winner}")
    assert min(count[1], count[2], count[3]) >= 3 and inf_and_winner >= 3
