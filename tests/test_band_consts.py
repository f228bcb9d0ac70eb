"""The per-launch constants of k_vote_mfma's band re-check (kx, ky, inv1k, gq, Kb:
pvnet_amd/csrc/pv_band.h), which the host makes once per launch
for VoteArgs where every lane of every wave used to make them: pv_band.h compiled for
the host (tests/band_consts_host.cpp) gives, bit for bit, the numpy float32 restatement
of tests/test_band_filter.py, and the filter built from the host's values contains
round 5's queue (the inclusion that file checks, here with the host's K and gq)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_band_filter import constants, fma32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
THRS = [0.05, 0.5, 0.9, 0.99, 0.999999]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from pvnet_amd import build
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cxx = [cxx] if cxx else [build.hipcc(), "-x", "c++"]      # hipcc's clang compiles plain C++ too
    so = str(tmp_path_factory.mktemp("band_host") / "libpvband_host.so")
    subprocess.check_call([*cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(REPO, "tests", "band_consts_host.cpp")])
    f = ctypes.CDLL(so).pv_band_consts_host
    f.restype = None
    f.argtypes = [ctypes.c_float] * 3 + [ctypes.c_void_p]

    def run(tau, gzf, gzr):
        out = np.zeros(5, f32)
        f(float(tau), float(gzf), float(gzr), out.ctypes.data)
        return out
    return run


def restated(tau, gzf, gzr):
    """The kernel's former per-lane expressions, one float32 rounding per operation."""
    kx = f32(f32(gzr / tau) * f32(1.0001))
    ky = f32(gzr * f32(1.0001))
    inv1k = f32(f32(1.0002) / f32(f32(1.0) - f32(ky * f32(1.0001))))
    gq = f32(f32(f32(gzf / f32(gzf + gzr)) * f32(1.0011)) * inv1k)
    Kb = f32(f32(kx + ky) * inv1k)
    return np.array([kx, ky, inv1k, gq, Kb], f32)


@pytest.mark.parametrize("thr", THRS)
def test_host_constants_equal_restatement(thr, host):
    tau, gzf, gzr = constants(thr)
    got, want = host(tau, gzf, gzr), restated(tau, gzf, gzr)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("thr", THRS)
def test_host_filter_contains_old_queue(thr, host):
    """tests/test_band_filter.py::test_new_queue_contains_old with K and gq as the host made them."""
    rng = np.random.default_rng(int(thr * 1e6) + 1)
    tau, gzf, gzr = constants(thr)
    kx, ky, _, gq, K = host(tau, gzf, gzr)
    n = 400_000
    Bv = f32(10.0) ** rng.uniform(-1, 4.5, n).astype(f32)
    s = np.ldexp(f32(1.0), -rng.integers(0, 10, n)).astype(f32)
    G = f32(f32(gzf * Bv) * s) * f32(1.001)                          # round 5's per-pair constant
    gb = f32(f32(f32(gzf + gzr) * Bv) * s) * f32(1.00001)            # the hot loop's bound
    Gn = f32(gb * gq)
    d = (Bv * s * rng.uniform(0, 1, n).astype(f32)).astype(f32)
    X = (d * rng.uniform(-1, 1, n).astype(f32)).astype(f32)
    Yabs = np.abs(X) * rng.uniform(0, 3, n).astype(f32)
    Y = np.where(rng.random(n) < 0.5, Yabs, -Yabs).astype(f32)
    g = fma32(kx, np.abs(X), fma32(ky, np.abs(Y), G))
    frac = rng.choice(np.array([1.0, 0.999999, 1.000001, 0.5, -1.0, -0.999999, -1.000001], dtype=f32), n)
    X = (np.abs(Y) + (g * frac).astype(f32)).astype(f32)
    g = fma32(kx, np.abs(X), fma32(ky, np.abs(Y), G))                # g of the final X
    z = (X - np.abs(Y)).astype(f32)
    old = np.abs(z) <= g
    new = fma32(-K, np.abs(X), np.abs(z)) <= Gn
    assert old.sum() > n // 4
    bad = old & ~new
    assert not bad.any(), f"{bad.sum()} pairs queued by the round-5 test but not by the filter (thr {thr})"
