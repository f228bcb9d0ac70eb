"""Guarded buffers: outputs, workspaces and inputs of a C entry placed between 64 KiB guards inside one
larger uint8 allocation each, so a test sees *where* a call writes and *what else* it reads.

    g = Guarded(device)
    out = g.out((b, H, W), torch.float32)           # 256-byte aligned view, patterned guards around it
    ws = g.workspace(nbytes)                        # exactly nbytes, the same guards
    x = g.inp(array, surround=0xFF)                 # the array between two runs of one byte
    ... call the entry with x.data_ptr(), out.data_ptr(), ws.data_ptr() ...
    g.check()                                       # guards, inputs and surrounds bit-identical

Why 64 KiB: it is more than one whole block's widest store (1024 lanes x 16 bytes), so an overrun of one
block still lands inside the buffer's own allocation: it is seen and cannot fault.  The guard bytes
follow (131 i + 7) & 0xFF of their position i in the allocation, so a kernel that writes any
constant over them (0, 0xFF, a NaN) changes all but one byte in 256.  A plain module: no fixture,
works on CPU tensors too (tests/test_guarded.py)."""
import numpy as np
import torch

GUARD = 64 * 1024
ALIGN = 256


def pattern(lo, hi, device):
    """The guard pattern of positions [lo, hi) of an allocation."""
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    return ((131 * i + 7) & 0xFF).to(torch.uint8)


class _Buf:
    def __init__(self, name, kind, base, start, nbytes, expect):
        self.name, self.kind, self.base, self.start, self.nbytes, self.expect = name, kind, base, start, nbytes, expect


class Guarded:
    def __init__(self, device):
        self.device = torch.device(device)
        self.bufs = []

    def _base(self, nbytes, offset):
        """A uint8 allocation with room for guard + padding to ALIGN + offset + nbytes + guard, and the
        view's first byte in it."""
        base = torch.empty(GUARD + ALIGN + offset + nbytes + GUARD, dtype=torch.uint8, device=self.device)
        start = GUARD + (-(base.data_ptr() + GUARD)) % ALIGN + offset
        return base[:start + nbytes + GUARD], start

    def _view(self, base, start, shape, dtype):
        size = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64)) * size
        if (base.data_ptr() + start) % size:
            raise ValueError(f"a {dtype} view needs an offset that is a multiple of its element size")
        return base[start:start + n].view(dtype).reshape(shape)

    def out(self, shape, dtype, fill=0xCD, offset=0, name=None):
        """A view of `shape` and `dtype` whose bytes all hold `fill`, 256-byte aligned plus `offset` bytes."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        base, start = self._base(nbytes, offset)
        base[:start] = pattern(0, start, self.device)
        base[start + nbytes:] = pattern(start + nbytes, base.numel(), self.device)
        base[start:start + nbytes] = fill
        expect = (base[:start].clone(), base[start + nbytes:].clone())
        self.bufs.append(_Buf(name or f"out{len(self.bufs)}", "out", base, start, nbytes, expect))
        return self._view(base, start, shape, dtype)

    def workspace(self, nbytes, fill=0x00, name=None):
        """Exactly `nbytes` bytes (uint8), every one holding `fill`."""
        return self.out((int(nbytes),), torch.uint8, fill=fill, name=name or f"workspace{len(self.bufs)}")

    def inp(self, array, surround=0x00, name=None):
        """`array` (numpy) on the device between two 64 KiB runs of the byte `surround`: it starts 256-byte
        aligned and ends on the last byte before the rear run."""
        a = np.ascontiguousarray(array)
        nbytes = a.nbytes
        base, start = self._base(nbytes, 0)
        base[:] = surround
        base[start:start + nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(self.device)
        self.bufs.append(_Buf(name or f"inp{len(self.bufs)}", "inp", base, start, nbytes, base.clone()))
        return self._view(base, start, a.shape, torch.from_numpy(a.reshape(-1)[:0].copy()).dtype)

    def check(self):
        """Synchronise; every guard equals its pattern and every input and its surround what was placed."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        errors = []
        for b in self.bufs:
            end = b.start + b.nbytes
            if b.kind == "out":
                sides = [("front guard", b.base[:b.start], b.expect[0], -b.start),
                         ("rear guard", b.base[end:], b.expect[1], 0)]
            else:
                sides = [("front surround", b.base[:b.start], b.expect[:b.start], -b.start),
                         ("input", b.base[b.start:end], b.expect[b.start:end], 0),
                         ("rear surround", b.base[end:], b.expect[end:], 0)]
            for side, got, want, origin in sides:
                hit = torch.nonzero(got != want).flatten()
                if hit.numel():
                    lo, hi = int(hit[0]) + origin, int(hit[-1]) + origin
                    rel = "its first byte" if side.startswith("front") else \
                        "the input's first byte" if side == "input" else "the first byte after it"
                    errors.append(f"{b.name} ({b.nbytes} bytes): {side} changed, {hit.numel()} bytes, first at "
                                  f"{lo:+d} and last at {hi:+d} from {rel}")
        assert not errors, "memory contract broken:\n  " + "\n  ".join(errors)

