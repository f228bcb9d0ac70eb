"""tests/guarded.py on CPU tensors: check() sees a one-byte write on either side of a view, at the far
end of a guard and inside an input, passes when only the view is written, and views are placed as asked."""
import re

import numpy as np
import pytest
import torch

from tests.guarded import ALIGN, GUARD, Guarded


def raw(g, i=-1):
    """The whole allocation behind buffer i, and the view's first and one-past-last byte in it."""
    b = g.bufs[i]
    return b.base, b.start, b.start + b.nbytes


def flip(base, pos):
    base[pos] = int(base[pos]) ^ 0x01


def test_placement_alignment_and_offset():
    g = Guarded("cpu")
    for shape, dtype, offset in [((3, 5), torch.float32, 0), ((7,), torch.uint8, 1), ((7,), torch.uint8, 5),
                                 ((2, 3), torch.float64, 8), ((4,), torch.float16, 2), ((1,), torch.int64, 0)]:
        t = g.out(shape, dtype, fill=0xCD, offset=offset)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        assert t.data_ptr() % ALIGN == offset
        base, lo, hi = raw(g)
        assert t.data_ptr() == base.data_ptr() + lo and hi - lo == t.numel() * t.element_size()
        assert lo >= GUARD and base.numel() - hi == GUARD
        assert (base[lo:hi] == 0xCD).all()
        # the pattern depends on the position: no constant equals more than one byte in 256 of a guard
        front = base[:lo].numpy()
        np.testing.assert_array_equal(front, ((131 * np.arange(lo) + 7) & 0xFF).astype(np.uint8))
        assert max(np.bincount(front, minlength=256)) <= lo // 256 + 1
    w = g.workspace(1000, fill=0xA5)
    assert w.dtype == torch.uint8 and w.numel() == 1000 and w.data_ptr() % ALIGN == 0 and (w == 0xA5).all()
    with pytest.raises(ValueError, match="multiple of its element size"):
        g.out((2,), torch.float32, offset=1)
    g.check()


def test_input_placement():
    g = Guarded("cpu")
    for a, surround in [(np.arange(15, dtype=np.float32).reshape(3, 5), 0xFF), (np.arange(7, dtype=np.uint8), 0x00),
                        (np.array([[1.5, -2.0]], np.float64), 0xFF), (np.arange(6, dtype=np.float16), 0xFF)]:
        t = g.inp(a, surround=surround)
        assert tuple(t.shape) == a.shape and t.data_ptr() % ALIGN == 0
        np.testing.assert_array_equal(t.numpy(), a)
        base, lo, hi = raw(g)
        assert hi - lo == a.nbytes and lo >= GUARD and base.numel() - hi == GUARD  # ends on the last byte before the surround
        assert (base[:lo] == surround).all() and (base[hi:] == surround).all()
    # 0xFF is a NaN for every float width
    assert np.isnan(raw(g)[0][:8].numpy().view(np.float16)).all()
    g.check()


def test_writing_only_the_views_passes():
    g = Guarded("cpu")
    o = g.out((5, 7), torch.float32)
    o1 = g.out((9,), torch.uint8, offset=1)
    w = g.workspace(300)
    x = g.inp(np.ones((4, 4), np.int32), surround=0xFF)
    o.fill_(float("nan"))
    o1.fill_(0)
    w.fill_(0xFF)
    assert int(x.sum()) == 16
    g.check()
    g.check()


@pytest.mark.parametrize("where,side,offset", [("before", "front guard", "-1"), ("after", "rear guard", "+0"),
                                               ("last", "rear guard", f"+{GUARD - 1}"),
                                               ("first", "front guard", None)])
def test_a_one_byte_write_outside_a_view_is_caught(where, side, offset):
    g = Guarded("cpu")
    g.out((3,), torch.float32, name="quiet")
    t = g.out((5, 7), torch.float16, offset=2, name="victim")
    base, lo, hi = raw(g)
    pos = {"before": lo - 1, "after": hi, "last": base.numel() - 1, "first": 0}[where]
    flip(base, pos)
    t.fill_(1.0)
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert "victim" in msg and side in msg and "quiet" not in msg and "1 bytes" in msg
    want = offset if offset is not None else f"{-lo:+d}"
    assert f"first at {want} " in msg and f"last at {want} " in msg


def test_a_write_of_the_pattern_bytes_own_constant_is_caught():
    """A kernel that stores one constant over a guard: at most one byte in 256 already holds it."""
    for const in (0x00, 0xFF, 0x7E):
        g = Guarded("cpu")
        g.out((16,), torch.float32, name="victim")
        base, lo, hi = raw(g)
        base[hi:hi + 512] = const
        with pytest.raises(AssertionError) as e:
            g.check()
        hit = re.search(r"rear guard changed, (\d+) bytes, first at \+(\d+) and last at \+(\d+) ", str(e.value))
        assert hit and 510 <= int(hit.group(1)) <= 512 and int(hit.group(2)) <= 1 and int(hit.group(3)) >= 510


@pytest.mark.parametrize("where", ["input", "front", "rear"])
def test_a_one_byte_write_to_an_input_or_its_surround_is_caught(where):
    g = Guarded("cpu")
    g.inp(np.zeros(8, np.float32), name="quiet")
    x = g.inp(np.arange(40, dtype=np.float64).reshape(5, 8), surround=0xFF, name="victim")
    base, lo, hi = raw(g)
    pos = {"input": lo + 13, "front": lo - 1, "rear": base.numel() - 1}[where]
    flip(base, pos)
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert "victim" in msg and "quiet" not in msg and "1 bytes" in msg
    if where == "input":
        assert "input changed" in msg and "first at +13 " in msg and "last at +13 " in msg
        assert x.reshape(-1)[1] != 1.0
    elif where == "front":
        assert "front surround" in msg and "first at -1 " in msg
    else:
        assert "rear surround" in msg and f"first at +{GUARD - 1} " in msg


def test_first_and_last_offset_of_a_longer_overrun():
    g = Guarded("cpu")
    g.out((100,), torch.uint8, name="victim")
    base, lo, hi = raw(g)
    base[hi + 3:hi + 40] = base[hi + 3:hi + 40] ^ 0xFF
    with pytest.raises(AssertionError) as e:
        g.check()
    assert "37 bytes, first at +3 and last at +39 " in str(e.value)
