"""hyp_class (pvnet_amd/csrc/pv_hypclass.h, part of pv_common.h): a hypothesis's class for
k_vote_mfma -- bit 0 fast, bit 1 exact-only, neither for a non-finite one -- which the
hypotheses' producers now store as ballots beside the hypotheses instead of every vote wave
working it out again.  The header compiled for the host (tests/hyp_class_host.cpp) gives,
value for value, a numpy float32 restatement of the expressions the vote kernel's prologue
used to evaluate: isfinite of both coordinates, hyp_exact_only (beyond kHypMax, or within
kLattice of a lattice point on both axes, with rintf's round-half-even) and the matrix-core
kernel's own range |h| < kMHypMax."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FAST, EXACT = 1, 2
K_HYP_MAX, K_LATTICE, K_M_HYP_MAX = f32(1.0e17), f32(2.5e-6), f32(8.0e6)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from pvnet_amd import build
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cxx = [cxx] if cxx else [build.hipcc(), "-x", "c++"]      # hipcc's clang compiles plain C++ too
    so = str(tmp_path_factory.mktemp("hyp_class") / "libpvhypclass_host.so")
    subprocess.check_call([*cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(REPO, "tests", "hyp_class_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.pv_hyp_class_host.restype = None
    lib.pv_hyp_class_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.pv_hyp_class_consts.restype = None
    lib.pv_hyp_class_consts.argtypes = [ctypes.c_void_p]

    def run(hx, hy):
        hx = np.ascontiguousarray(hx, f32)
        hy = np.ascontiguousarray(hy, f32)
        out = np.zeros(hx.shape, np.uint32)
        lib.pv_hyp_class_host(hx.ctypes.data, hy.ctypes.data, hx.size, out.ctypes.data)
        return out
    run.lib = lib
    return run


def restated(hx, hy):
    """The prologue's expressions, one float32 operation at a time (np.rint rounds half to even, as rintf)."""
    hx, hy = np.asarray(hx, f32), np.asarray(hy, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(hx) & np.isfinite(hy)
        big = ~(np.abs(hx) <= K_HYP_MAX) | ~(np.abs(hy) <= K_HYP_MAX)
        lat = (np.abs((hx - np.rint(hx)).astype(f32)) < K_LATTICE) & (np.abs((hy - np.rint(hy)).astype(f32)) < K_LATTICE)
        xo = fin & (big | lat | ~((np.abs(hx) < K_M_HYP_MAX) & (np.abs(hy) < K_M_HYP_MAX)))
    return (np.where(fin & ~xo, FAST, 0) | np.where(xo, EXACT, 0)).astype(np.uint32)


def _neighbours(x, n=3):
    """x and its n float32 neighbours on either side."""
    x = f32(x)
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        out += [lo, hi]
    return out


def _special_values():
    tiny = np.finfo(f32).tiny
    sub = [f32(1e-45), f32(tiny / 2), np.nextafter(f32(tiny), f32(0))]            # subnormals
    v = [f32(0.0), f32(-0.0), *sub, f32(tiny), f32(np.nan), f32(np.inf), f32(-np.inf), np.finfo(f32).max]
    v += [f32(k) for k in (1, 2, 3, 7, 640, 65535, 2 ** 22, 2 ** 23, 2 ** 23 + 2, 2 ** 24)]      # integers
    v += [f32(k + 0.5) for k in (0, 1, 2, 3, 4, 99, 2 ** 20, 2 ** 22)]                        # half-integers
    for base in (0.0, 1.0, 2.0, 5.0, 17.0, 320.0):                                            # around kLattice
        for d in (*_neighbours(K_LATTICE), f32(2.4e-6), f32(2.6e-6), f32(1e-6), f32(5e-6)):
            v += [f32(f32(base) + d), f32(f32(base) - d)]
    v += _neighbours(K_HYP_MAX) + _neighbours(K_M_HYP_MAX) + [f32(1e16), f32(1e18), f32(7.9e6), f32(8.1e6)]
    v = np.array(v, f32)
    v = np.concatenate([v, -v])
    return np.unique(v.view(np.uint32)).view(f32)           # (by bit pattern: keeps -0 and NaN)


def test_constants(host):
    got = np.zeros(3, f32)
    host.lib.pv_hyp_class_consts(got.ctypes.data)
    np.testing.assert_array_equal(got.view(np.uint32), np.array([K_HYP_MAX, K_LATTICE, K_M_HYP_MAX]).view(np.uint32))


def test_special_values_all_pairs(host):
    v = _special_values()
    hx, hy = (a.ravel() for a in np.meshgrid(v, v, indexing="ij"))
    got, want = host(hx, hy), restated(hx, hy)
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got)) == {0, FAST, EXACT}          # never both bits
    # what each class means, on chosen values
    c = lambda x, y: int(host([x], [y])[0])
    assert c(0.0, -0.0) == EXACT and c(3.0, 640.0) == EXACT            # lattice points
    assert c(0.5, 2.5) == FAST and c(3.0, 0.5) == FAST                 # one axis off the lattice is enough
    assert c(1e-45, -1e-45) == EXACT                                   # subnormals round to the lattice point 0
    assert c(np.nan, 1.5) == 0 and c(1.5, np.inf) == 0 and c(-np.inf, np.nan) == 0
    assert c(K_M_HYP_MAX, 0.5) == EXACT and c(np.nextafter(K_M_HYP_MAX, f32(0)), 0.5) == FAST
    assert c(0.5, -K_M_HYP_MAX) == EXACT and c(0.5, -np.nextafter(K_M_HYP_MAX, f32(0))) == FAST
    assert c(K_HYP_MAX, 0.5) == EXACT and c(np.nextafter(K_HYP_MAX, f32(np.inf)), 0.5) == EXACT
    assert c(np.finfo(f32).max, 0.5) == EXACT
    assert c(5.0 + 2e-6, 17.0 - 2e-6) == EXACT and c(5.0 + 4e-6, 17.0) == FAST


def test_random_values(host):
    rng = np.random.default_rng(7)
    n = 200_000
    mag = f32(10.0) ** rng.uniform(-8, 19, n).astype(f32)
    hx = (mag * rng.choice(np.array([-1, 1], f32), n)).astype(f32)
    hy = (rng.uniform(-700, 700, n)).astype(f32)
    # a share on or next to the lattice
    k = n // 4
    hx[:k] = np.rint(rng.uniform(-700, 700, k)).astype(f32) + rng.choice(
        np.array([0, 1e-6, -1e-6, 2.5e-6, -2.5e-6, 3e-6], f32), k)
    hy[:k] = np.rint(hy[:k]) + rng.choice(np.array([0, 2e-6, -2.4e-6, 2.6e-6], f32), k)
    got = host(hx, hy)
    np.testing.assert_array_equal(got, restated(hx, hy))
    assert (got == FAST).sum() > n // 4 and (got == EXACT).sum() > n // 8
