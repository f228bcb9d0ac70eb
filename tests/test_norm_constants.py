"""kN1SqLow / kN1SqMax (pv_common.h): the vote kernels test a pixel's validity
on its squared norm s instead of on norm1 = sqrtf(s).  For every float32 s,
sqrtf(s) <= c  <=>  s <= T, with (c, T) = (1e-6f, kN1SqLow) and (1e18f,
kN1SqMax); numpy's float32 sqrt is the correctly rounded one the library is
built with."""
import os
import re

import numpy as np
import pytest

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pvnet_amd", "csrc", "pv_common.h")


def _const(name):
    m = re.search(r"constexpr float " + name + r" = (0x[0-9a-fA-F.]+p[+-]?\d+)f;", open(HDR).read())
    assert m, name
    return np.float32(float.fromhex(m.group(1)))


CASES = [(np.float32(1e-6), "kN1SqLow"), (np.float32(1e18), "kN1SqMax")]


@pytest.mark.parametrize("c, name", CASES)
def test_every_float_near_the_constant(c, name):
    T = _const(name)
    bits = T.view(np.uint32).astype(np.int64) + np.arange(-64, 65)
    s = bits.astype(np.uint32).view(np.float32)
    np.testing.assert_array_equal(np.sqrt(s) <= c, s <= T)
    # T is the largest float whose root is <= c
    assert np.sqrt(T) <= c and not np.sqrt(np.nextafter(T, np.float32(np.inf))) <= c


@pytest.mark.parametrize("c, name", CASES)
def test_whole_positive_range(c, name):
    """A log-spaced sweep (every 509th bit pattern from +0 through the subnormals to
    +inf), the range's ends, and NaN."""
    T = _const(name)
    s = np.arange(0, 0x7f800000 + 1, 509, dtype=np.int64).astype(np.uint32).view(np.float32)
    s = np.concatenate([s, np.float32([0.0, np.finfo(np.float32).tiny, 1e-45, np.finfo(np.float32).max, np.inf,
                                       np.nan])])
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(np.sqrt(s) <= c, s <= T)
