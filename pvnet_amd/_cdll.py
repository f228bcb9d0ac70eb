"""What every ctypes binding of this package shares: loading a library once, and turning a status
code of the C ABI into an exception.

No CPU fallback anywhere: a library that is missing is an error.  ``python -m pvnet_amd.build`` (or
``__graft_entry__.build()``) builds them all next to this file.
"""
from __future__ import annotations

import ctypes
import os
import threading

# the status codes every public header defines (PV_OK is 0); anything else is a HIP error
PV_EINVAL, PV_EWORKSPACE, PV_EALIGN = -1, -2, -3
_ERR = {PV_EINVAL: "invalid argument", PV_EWORKSPACE: "workspace missing or too small",
        PV_EALIGN: "pointer not aligned as documented"}


def loader(path: str, signatures):
    """A load() for the library at `path`: the first call opens it and applies `signatures`, a list
    of (name, restype, argtypes); every call returns that one ctypes.CDLL."""
    lib = None
    lock = threading.Lock()

    def load():
        """Load the library once (raises if it is absent: no fallback path)."""
        nonlocal lib
        if lib is not None:
            return lib
        with lock:
            if lib is None:
                if not os.path.exists(path):
                    raise RuntimeError(f"{os.path.basename(path)} not found at {path}; "
                                       "build it with `python -m pvnet_amd.build`")
                L = ctypes.CDLL(path)
                for name, res, args in signatures:
                    fn = getattr(L, name)
                    fn.restype = res
                    fn.argtypes = args
                lib = L
        return lib
    return load


def checker(error):
    """A check(code, what) that raises `error` for a status code other than PV_OK."""
    def check(code: int, what: str):
        if code != 0:
            raise error(f"{what} failed: {_ERR.get(code, 'HIP error')} (code {code})")
    return check
