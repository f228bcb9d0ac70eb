"""tests/front_ref.py, the numpy restatement of the front half's counter RNG, against
pvnet_amd/csrc/pv_rng.h compiled for the host (tests/rng_host.cpp): bit-equal on 10^5
(seed, key, n) triples with the word-boundary values, the known answers of user seed
20240 (so that moving or editing the functions cannot change them unnoticed), and the
restatement's own uniformity, so that what tests/test_gpu_front_half.py injects is fair."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import front_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, U32, F32 = np.uint64, np.uint32, np.float32
M64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from pvnet_amd import build
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cxx = [cxx] if cxx else [build.hipcc(), "-x", "c++"]      # hipcc's clang compiles plain C++ too
    so = str(tmp_path_factory.mktemp("rng_host") / "libpvrng_host.so")
    subprocess.check_call([*cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(REPO, "tests", "rng_host.cpp")])
    L = ctypes.CDLL(so)
    for name in ("pv_rng_mix64", "pv_rng_hash32", "pv_rng_rand_unit"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * (3 if name.endswith("unit") else 2)
    L.pv_rng_rand_index.restype = None
    L.pv_rng_rand_index.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 4

    class Host:
        @staticmethod
        def mix64(z):
            z = np.ascontiguousarray(z, U64)
            out = np.empty_like(z)
            L.pv_rng_mix64(z.size, z.ctypes.data, out.ctypes.data)
            return out

        @staticmethod
        def hash32(x):
            x = np.ascontiguousarray(x, U32)
            out = np.empty_like(x)
            L.pv_rng_hash32(x.size, x.ctypes.data, out.ctypes.data)
            return out

        @staticmethod
        def rand_index(seed, key, n):
            seed, key, n = np.ascontiguousarray(seed, U64), np.ascontiguousarray(key, U64), np.ascontiguousarray(n, np.int32)
            out = np.empty(seed.shape, np.int32)
            L.pv_rng_rand_index(seed.size, seed.ctypes.data, key.ctypes.data, n.ctypes.data, out.ctypes.data)
            return out

        @staticmethod
        def rand_unit(seed, key):
            seed, key = np.ascontiguousarray(seed, U64), np.ascontiguousarray(key, U64)
            out = np.empty(seed.shape, F32)
            L.pv_rng_rand_unit(seed.size, seed.ctypes.data, key.ctypes.data, out.ctypes.data)
            return out
    return Host


def triples():
    """>= 10^5 (seed, key, n): the cross product of the word-boundary values, then random ones --
    keys below and above 2^32, n over every magnitude."""
    es = np.array([0, 1, M64, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 20240, 0x9e3779b97f4a7c15], U64)
    ek = np.array([0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 33 + 1, 2 ** 63, M64, 9215, 307199], U64)
    en = np.array([1, 2, 3, 255, 256, 29861, 2 ** 16, 2 ** 24 + 1, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1], np.int32)
    s, k, n = (a.reshape(-1) for a in np.meshgrid(es, ek, en, indexing="ij"))
    rng = np.random.default_rng(2024)
    m = 120_000
    rs = rng.integers(0, 2 ** 64, m, dtype=U64)
    rs[::7] >>= U64(32)                                                   # seeds below 2^32
    rk = rng.integers(0, 2 ** 64, m, dtype=U64) >> rng.integers(0, 64, m).astype(U64)
    rn = (rng.integers(1, 2 ** 31, m) >> rng.integers(0, 31, m)).clip(1, 2 ** 31 - 1).astype(np.int32)
    rn[:100] = 1
    rn[100:200] = 2 ** 31 - 1
    rs[200:300] = 0
    rs[300:400] = U64(M64)
    return np.concatenate([s, rs]), np.concatenate([k, rk]), np.concatenate([n, rn])


def test_restatement_equals_host_bit_for_bit(host):
    s, k, n = triples()
    assert s.size >= 100_000
    assert (k > U64(2 ** 32)).sum() > 10_000 and (k < U64(2 ** 32)).sum() > 10_000
    assert (n == 1).sum() >= 100 and (n == 2 ** 31 - 1).sum() >= 100
    assert (s == 0).sum() >= 100 and (s == U64(M64)).sum() >= 100
    np.testing.assert_array_equal(R.mix64(s), host.mix64(s))
    np.testing.assert_array_equal(R.mix64(k), host.mix64(k))
    x = np.concatenate([R._lo(s), R._lo(k), np.array([0, 1, 2 ** 32 - 1, 2 ** 31], U32)])
    np.testing.assert_array_equal(R.hash32(x), host.hash32(x))
    got, want = R.rand_index(s, k, n), host.rand_index(s, k, n)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    assert np.all(want >= 0) and np.all(want < n)
    assert np.all(want[n == 1] == 0)
    u, uh = R.rand_unit(s, k), host.rand_unit(s, k)
    assert u.dtype == F32
    np.testing.assert_array_equal(u.view(U32), uh.view(U32))
    assert np.all(uh >= 0) and np.all(uh < 1)


def test_known_answers_seed_20240(host):
    """From a host copy of the functions as they stood in pv_common.h."""
    hs, ks = R.seeds(20240)
    assert hs == 7247227743336886627
    assert ks == 16941140077177136420
    assert int(host.mix64([20240])[0]) == hs and int(host.mix64([20240 ^ R.KEEP_XOR])[0]) == ks
    keys = np.array([0, 1, 2, 9215, 2 ** 32 + 5], U64)
    want = [27200, 11551, 21200, 12729, 4050]
    for f in (R.rand_index, host.rand_index):
        assert f(np.full(5, hs, U64), keys, np.full(5, 29861, np.int32)).tolist() == want
    keys = np.array([0, 1, 307199, 393335, 2 ** 32 + 5], U64)
    want = ["0.364847183", "0.258624673", "0.873308182", "0.55992502", "0.355998039"]
    for f in (R.rand_unit, host.rand_unit):
        assert ["%.9g" % v for v in f(np.full(5, ks, U64), keys)] == want


def test_pairs_and_keep_mask_layout():
    """pairs / keep_mask against the scalar definitions, key by key."""
    seed, nh, vn = 0xfeedface12345678, 5, 3
    tn = [7, 0, 1000]
    hs, ks = R.seeds(seed)
    p = R.pairs(seed, tn, nh, vn)
    assert p.shape == (3, nh, vn, 2) and p.dtype == np.int32
    for b in range(3):
        for h in range(nh):
            for v in range(vn):
                gid = (b * nh + h) * vn + v
                want = [0, 0] if tn[b] == 0 else [int(R.rand_index(hs, 2 * gid + e, tn[b])) for e in (0, 1)]
                assert p[b, h, v].tolist() == want
    rng = np.random.default_rng(1)
    fg = rng.random((3, 9, 11)) < 0.6
    fg[1] = False
    fg[1, 0, :5] = True                       # 5 <= max_num: kept whole
    max_num = 20
    k = R.keep_mask(seed, fg, max_num)
    assert k.shape == fg.shape and k.dtype == np.uint8 and np.all(k[1] == 1)
    for b in (0, 2):
        n = int(fg[b].sum())
        assert n > max_num
        pk = F32(max_num) / F32(n)
        for p_ in range(99):
            assert k[b].reshape(-1)[p_] == (R.rand_unit(ks, b * 99 + p_) < pk)


def test_restatement_is_uniform():
    """rand_index over 16 buckets of [0, n) on 10^6 consecutive keys: chi-square with 15 degrees of
    freedom below its 0.9999 quantile, 44.3.  Kept counts at max_num / fg = 0.2 within 4 sigma of
    max_num, sigma^2 = max_num (1 - 0.2)."""
    hs, ks = R.seeds(20240)
    n = 29861
    idx = R.rand_index(hs, np.arange(10 ** 6, dtype=U64), n)
    assert idx.min() >= 0 and idx.max() < n
    bucket = idx.astype(np.int64) * 16 // n
    got = np.bincount(bucket, minlength=16)
    exp = np.bincount(np.arange(n, dtype=np.int64) * 16 // n, minlength=16) * (10 ** 6 / n)
    chi2 = float(((got - exp) ** 2 / exp).sum())
    print("chi2", chi2)
    assert chi2 < 44.3, chi2
    # both draws of a pair are as likely to be any index: the odd keys alone
    got = np.bincount(bucket[1::2], minlength=16)
    chi2 = float(((got - exp / 2) ** 2 / (exp / 2)).sum())
    assert chi2 < 44.3, chi2
    for fg, max_num in ((5000, 1000), (40000, 8000)):
        kept = int((R.rand_unit(ks, np.arange(fg, dtype=U64)) < F32(max_num) / F32(fg)).sum())
        sigma = (max_num * (1 - max_num / fg)) ** 0.5
        print("kept", kept, "of", fg, "sigma", sigma)
        assert abs(kept - max_num) <= 4 * sigma, (kept, max_num, sigma)
