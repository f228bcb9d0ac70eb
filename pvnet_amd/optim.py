"""The mixed-precision optimiser step on the device (include/pvoptim.h, libpvoptim.so).

    opt = Optimizer(net.named_parameters(), "adam", lr=1e-3, max_norm=10.0)
    loss = pvnet_loss(...)[0]
    opt.scale_loss(loss).backward()
    opt.step()                      # one C call: non-finite check, unscale, clip, update, f16 copy, zeroed grads

``step()`` reads nothing back: whether the step happens, the clip coefficient and the next loss scale
are decided on the device, so a whole training step can be captured into a ``torch.cuda.graph``.  The
optimiser keeps f32 master weights for f16 parameters (an f32 parameter is its own master), the moments,
and one persistent gradient buffer per parameter, which it assigns to ``p.grad``: autograd accumulates
into it in place and the step zeroes it.  No CPU fallback: without libpvoptim.so or a ROCm device the
calls raise.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _optim_lib as P

ALGORITHMS = {"adam": P.PV_OPT_ADAM, "adamw": P.PV_OPT_ADAMW, "sgd": P.PV_OPT_SGD}
_KIND = {torch.float32: P.PV_OPT_F32, torch.float16: P.PV_OPT_F16}


def _fail(msg):
    raise RuntimeError(msg)


def _need_device(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        _fail(f"{what} must be a tensor on a ROCm device (there is no CPU path)")


def upload(struct_array, device):
    """The bytes of a ctypes array as a uint8 device tensor (at least 8 bytes, so it has an address)."""
    raw = bytearray(bytes(struct_array)) or bytearray(8)
    return torch.frombuffer(raw, dtype=torch.uint8).to(device)


def make_table(entries, algorithm, device):
    """``entries``: one (master, model or None, grad, m, v or None) per parameter, device tensors.
    Returns (table, chunks, n_chunks): the two device arrays of pv_optim_step and the chunk count."""
    lib = P.load()
    tab = (P.OptTensor * max(len(entries), 1))()
    for i, (master, model, grad, m, v) in enumerate(entries):
        tab[i] = P.OptTensor(master.data_ptr(), model.data_ptr() if model is not None else None, grad.data_ptr(),
                             m.data_ptr(), v.data_ptr() if v is not None else None, master.numel(), _KIND[grad.dtype], 0)
    n = lib.pv_optim_plan(tab, len(entries), algorithm, None, 0)
    if n < 0:
        P.check(int(n), "pv_optim_plan")
    chunks = (P.OptChunk * max(n, 1))()
    P.check(min(int(lib.pv_optim_plan(tab, len(entries), algorithm, chunks, n)), 0), "pv_optim_plan")
    return upload(tab, device), upload(chunks, device), int(n)


def make_state(device, lr, scale=1.0):
    """A fresh pv_optim_state as a uint8 device tensor: step 0, both running products 1."""
    return upload((P.OptState * 1)(P.OptState(1.0, 1.0, 0, lr, scale, 0, 0.0, 0, 0)), device)


def state_views(state):
    """The fields of a pv_optim_state tensor as 0-dim views of it."""
    S = P.OptState
    out = {}
    for name, dtype in (("b1pow", torch.float64), ("b2pow", torch.float64), ("step", torch.int64), ("lr", torch.float32),
                        ("scale", torch.float32), ("growth_tracker", torch.int32), ("grad_norm", torch.float32),
                        ("found_inf", torch.int32), ("skipped", torch.int32)):
        f = getattr(S, name)
        out[name] = state[f.offset:f.offset + f.size].view(dtype)[0]
    return out


class Optimizer:
    """Adam, AdamW or SGD with momentum over ``params`` (tensors, or (name, tensor) pairs as
    ``named_parameters()`` gives), with loss scaling, a global-norm clip and the skipped step of an
    overflowed gradient inside the one device call of ``step()``."""

    def __init__(self, params, algorithm="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0,
                 max_norm=None, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
                 zero_grads=True):
        if algorithm not in ALGORITHMS:
            _fail(f"algorithm must be one of {sorted(ALGORITHMS)}, not {algorithm!r}")
        items = [p if isinstance(p, tuple) else (f"parameter {i}", p) for i, p in enumerate(params)]
        if not items:
            _fail("params is empty")
        for name, p in items:
            _need_device(p, f"params: {name}")
            if p.dtype not in _KIND or not p.is_contiguous():
                _fail(f"params: {name} must be a contiguous float32 or float16 tensor")
        if len({p.device for _, p in items}) != 1:
            _fail("params must be on one device")
        betas = tuple(float(b) for b in betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            _fail("betas must be two values in [0, 1)")
        for what, val, ok in (("lr", lr, lambda x: x >= 0), ("eps", eps, lambda x: x > 0),
                              ("weight_decay", weight_decay, lambda x: x >= 0), ("momentum", momentum, lambda x: x >= 0),
                              ("init_scale", init_scale, lambda x: x > 0), ("growth_factor", growth_factor, lambda x: x >= 1),
                              ("backoff_factor", backoff_factor, lambda x: 0 < x <= 1)):
            if not (math.isfinite(val) and ok(val)):
                _fail(f"{what} is out of range: {val}")
        if max_norm is not None and math.isnan(max_norm):
            _fail("max_norm is NaN")
        if int(growth_interval) != growth_interval or growth_interval < 0:
            _fail("growth_interval must be an integer >= 0")
        self.algorithm = algorithm
        self.names = [n for n, _ in items]
        self.params = [p for _, p in items]
        self.device = self.params[0].device
        self.desc = P.OptDesc(ALGORITHMS[algorithm], betas[0], betas[1], eps, weight_decay, momentum,
                              max_norm if max_norm is not None else 0.0, growth_factor, backoff_factor,
                              int(growth_interval), 1 if zero_grads else 0, 0)
        with torch.no_grad():
            self.masters = [p.data if p.dtype == torch.float32 else p.data.float() for p in self.params]
            self.m = [torch.zeros_like(w) for w in self.masters]
            self.v = [torch.zeros_like(w) for w in self.masters] if algorithm != "sgd" else [None] * len(self.masters)
            self.grads = [torch.zeros_like(p.data) for p in self.params]
        for p, g in zip(self.params, self.grads):
            p.grad = g
        self.state = make_state(self.device, lr, init_scale)
        self._views = state_views(self.state)
        self._build()

    def _build(self):
        entries = [(w, p.data if p.dtype == torch.float16 else None, g, m, v)
                   for w, p, g, m, v in zip(self.masters, self.params, self.grads, self.m, self.v)]
        self._table, self._chunks, self._n_chunks = make_table(entries, self.desc.algorithm, self.device)
        need = P.load().pv_optim_workspace_size(self._n_chunks)
        self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        self._ws_off = (-self._ws.data_ptr()) % 256
        self._ws_bytes = need
        self._grad_ptrs = [g.data_ptr() for g in self.grads]

    def scale_loss(self, loss):
        """``loss`` times the device-side loss scale, which is not read back."""
        return loss * self._views["scale"].to(loss.dtype)

    def _check_grads(self):
        changed = False
        for i, (p, ptr) in enumerate(zip(self.params, self._grad_ptrs)):
            g = p.grad
            if g is not None and g.data_ptr() == ptr:
                continue
            if torch.cuda.is_current_stream_capturing():
                _fail(f"the gradient of {self.names[i]} is {'missing' if g is None else 'no longer the buffer in the table'}: "
                      "the table cannot be rebuilt while a graph is captured")
            if g is None:               # set_to_none: the persistent buffer again, holding zeros
                self.grads[i].zero_()
                p.grad = self.grads[i]
            else:
                if g.dtype != p.dtype or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                    _fail(f"the gradient of {self.names[i]} must be contiguous and of the parameter's shape, kind and device")
                self.grads[i] = g
            changed = True
        if changed:
            self._build()

    def step(self):
        """One pv_optim_step on the current stream."""
        self._check_grads()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
        P.check(P.load().pv_optim_step(ctypes.byref(self.desc), self._table.data_ptr(), len(self.params),
                                       self._chunks.data_ptr(), self._n_chunks, self.state.data_ptr(),
                                       self._ws.data_ptr() + self._ws_off, self._ws_bytes, stream), "pv_optim_step")

    def zero_grad(self):
        """Zero the gradient buffers in place (``step()`` already does with ``zero_grads``)."""
        for g in self.grads:
            g.zero_()

    def set_lr(self, value):
        """An asynchronous write of the state's learning rate."""
        self._views["lr"].fill_(float(value))

    def stats(self):
        """grad_norm, found_inf, skipped, scale and step of the state as 0-dim device tensors (views:
        they show the last step once it has run)."""
        return {k: self._views[k] for k in ("grad_norm", "found_inf", "skipped", "scale", "step")}

    def state_dict(self):
        return {"algorithm": self.algorithm, "master": [w.clone() for w in self.masters], "m": [m.clone() for m in self.m],
                "v": [v.clone() if v is not None else None for v in self.v], "state": self.state.clone()}

    def load_state_dict(self, sd):
        if sd["algorithm"] != self.algorithm or len(sd["master"]) != len(self.masters):
            _fail("the state is another optimiser's")
        with torch.no_grad():
            for dst, src in zip((*self.masters, *self.m, *self.v), (*sd["master"], *sd["m"], *sd["v"])):
                if dst is not None:
                    dst.copy_(src)
            for p, w in zip(self.params, self.masters):
                if p.dtype == torch.float16:
                    p.data.copy_(w)
            self.state.copy_(sd["state"])
