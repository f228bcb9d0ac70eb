"""Drop-in for ``lib/ransac_voting_gpu_layer/ransac_voting_gpu.py`` (RV): the
voting layers the inference pipeline calls, with the reference's signatures.

``ransac_voting_layer_v3`` (RV:520-604) and
``estimate_voting_distribution_with_mean`` (RV:333-406) /
``estimate_voting_distribution`` (RV:263-331) run the whole batch on the
device in a fixed sequence of HIP kernels (libpvvote.so, one C-ABI call):
no per-image Python loop, no host synchronisation, graph-capturable.

Behaviour kept from the reference:
  * foreground = ``mask.byte() != 0`` for v3 (RV:533), ``mask == 1`` for EVD
    (RV:340); fewer than ``min_num`` pixels -> zeros (RV:537-540); more than
    ``max_num`` -> Bernoulli(max_num/fg) downsampling (RV:543-546);
  * row-major compaction, coords = (col, row) (RV:548-552);
  * ``idxs`` drawn once per call (RV:553): every iteration of the reference's
    ``while True`` loop re-creates the same hypotheses, so its best-so-far
    state is final after the first pass and the loop only repeats identical
    work (RV:558-582).  The device pipeline runs that pass once; the
    iteration count the loop would take is reported in ``_diag['iters']``;
  * first-index argmax, strict-greater best update (RV:568-575);
  * least squares on the winner's inliers with ``b_inv``'s batch-wide
    identity fallback when any keypoint's matrix is singular (RV:503-518).

Not in the reference: the ``*_multi`` layers take a multi-object frame -- one
label map (or the network's ``C+1`` logits) and the keypoints of every class
-- where the reference loops over the classes with ``mask[bi] == k + 1``
(RV:273, RV:340); one call, the same kernel sequence.

Differences (documented in DESIGN.md): the random draws come from a counter
RNG seeded from torch's CPU generator, not from torch's device RNG (which
cannot be reproduced anyway); fp32 least-squares sums are accumulated in fp64
(the reference's fp32 order is unspecified).
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import torch

from . import _lib

__all__ = ["ransac_voting_layer_v3", "ransac_voting_layer_v5", "ransac_motion_voting",
           "estimate_voting_distribution_with_mean",
           "estimate_voting_distribution",
           "b_inv", "ransac_voting_layer_v3_from_network", "VotingWorkspace",
           "ransac_voting_layer_v3_multi", "ransac_voting_layer_v3_multi_from_network",
           "estimate_voting_distribution_with_mean_multi"]

_MASK_KIND = {torch.int64: _lib.PV_MASK_I64, torch.uint8: _lib.PV_MASK_U8, torch.bool: _lib.PV_MASK_U8,
              torch.int32: _lib.PV_MASK_I32}
_SEG_KIND = {torch.float32: _lib.PV_MASK_SEG_F32, torch.float16: _lib.PV_MASK_SEG_F16}
_VERTEX_KIND = {torch.float32: _lib.PV_VERTEX_F32, torch.float16: _lib.PV_VERTEX_F16}


def _draw_seed() -> int:
    # torch's default CPU generator: reproducible under torch.manual_seed, no device sync
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


class VotingWorkspace:
    """Device scratch for the pipelines, reused across calls of the same shape
    (needed for hipGraph capture: no allocation inside the captured region).

    A pipeline call zeroes and rewrites its workspace, so two calls in flight
    on different streams must not share one.

    * An explicit workspace (``_workspace=``, ``per_stream=False``) holds one
      call at a time: an eager call on a stream other than the one its
      previous call ran on raises ``RuntimeError`` if that call is still in
      flight (an event recorded after each call), so two threads handing one
      workspace to their own streams get an error, not a race.  The check is
      host-side: it cannot see a ``wait_stream`` that orders the two streams,
      so a caller that orders them itself passes ``check_streams=False``.
      Inside a
      graph capture there is no check (the call runs when the graph is
      replayed): a workspace captured into a graph belongs to that graph, and
      two graphs that may replay at the same time need one each.  Growing
      inside a capture raises: warm the workspace up (one eager call of the
      same shape) before capturing.
    * The default workspace (used when ``_workspace`` is omitted,
      ``per_stream=True``) keeps one buffer per (device, stream) for eager
      calls, and inside a capture takes a fresh buffer from the capturing
      graph's private memory pool for every call: each captured graph owns
      its scratch, so graphs captured on one shared stream (torch.cuda.graph
      without ``stream=``) can replay concurrently.

    A buffer that grows is released with ``record_stream`` for every stream
    that used it, so the caching allocator never hands it out while a kernel
    can still touch it.  Thread-safe (one lock per workspace)."""

    def __init__(self, per_stream: bool = False, check_streams: bool = True):
        self._buf = {}
        self._streams = {}
        self._per_stream = per_stream
        self._check = check_streams
        self._lock = threading.Lock()
        self._owner = {}       # explicit: key -> [stream handle of the last call, busy, event after it]

    def _key(self, device, stream):
        return (str(device), stream.cuda_stream) if self._per_stream else (str(device),)

    def get(self, device, nbytes: int) -> torch.Tensor:
        stream = torch.cuda.current_stream(device)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and self._per_stream:
            # the default workspace inside a capture: the graph's own (private pool)
            return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        key = self._key(device, stream)
        with self._lock:
            own = None
            if not self._per_stream and not capturing:
                own = self._owner.setdefault(key, [stream.cuda_stream, False, None])
                if self._check and own[0] != stream.cuda_stream and \
                        (own[1] or (own[2] is not None and not own[2].query())):
                    raise RuntimeError("VotingWorkspace is in use by a call in flight on another stream: give each "
                                       "stream (each launching thread) its own workspace")
            buf = self._buf.get(key)
            if buf is None or buf.numel() < nbytes:
                if capturing:
                    raise RuntimeError("VotingWorkspace would allocate during graph capture: make one eager call of "
                                       "the same shape with this workspace (_workspace=...) before capturing")
                if buf is not None:
                    for st in self._streams.get(key, ()):
                        buf.record_stream(st)
                buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
                self._buf[key] = buf
                self._streams[key] = set()
            self._streams[key].add(stream)
            if own is not None:
                # busy only once the buffer is in hand: a failed allocation leaves the workspace free
                own[0], own[1] = stream.cuda_stream, True
            return buf

    def done(self, device) -> None:
        """After the library call that used get()'s buffer was queued (or
        failed): an event on its stream marks when the workspace is free."""
        if self._per_stream or torch.cuda.is_current_stream_capturing():
            return
        stream = torch.cuda.current_stream(device)
        with self._lock:
            own = self._owner.get(self._key(device, stream))
            if own is None or own[0] != stream.cuda_stream:
                return
            if own[2] is None:
                own[2] = torch.cuda.Event()
            own[2].record(stream)
            own[1] = False


_default_ws = VotingWorkspace(per_stream=True)


def _desc(mask, vertex, seg=False):
    if not (isinstance(vertex, torch.Tensor) and vertex.is_cuda):
        raise RuntimeError("vertex must be a CUDA tensor")
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda):
        raise RuntimeError("mask must be a CUDA tensor")
    if vertex.dim() != 5 or vertex.shape[4] != 2:
        raise RuntimeError("vertex must be [b,h,w,vn,2]")
    b, h, w, vn, _ = vertex.shape
    if vertex.dtype not in _VERTEX_KIND:
        raise RuntimeError(f"vertex dtype {vertex.dtype} not supported (float32/float16)")
    if mask.device != vertex.device:
        raise RuntimeError("mask and vertex must be on the same device")
    d = _lib.ImageDesc()
    d.mask = mask.data_ptr()
    if seg:
        if mask.dim() != 4 or mask.shape[1] != 2 or tuple(mask.shape[2:]) != (h, w) or mask.shape[0] != b:
            raise RuntimeError("seg_pred must be [b,2,h,w]")
        if mask.dtype not in _SEG_KIND:
            raise RuntimeError(f"seg_pred dtype {mask.dtype} not supported")
        d.mask_kind = _SEG_KIND[mask.dtype]
        for i in range(4):
            d.mask_strides[i] = mask.stride(i)
    else:
        if tuple(mask.shape) != (b, h, w):
            raise RuntimeError(f"mask must be [b,h,w] = {(b, h, w)}, got {tuple(mask.shape)}")
        if mask.dtype not in _MASK_KIND:
            raise RuntimeError(f"mask dtype {mask.dtype} not supported")
        d.mask_kind = _MASK_KIND[mask.dtype]
        for i in range(3):
            d.mask_strides[i] = mask.stride(i)
    d.vertex = vertex.data_ptr()
    d.vertex_kind = _VERTEX_KIND[vertex.dtype]
    for i in range(5):
        d.vertex_strides[i] = vertex.stride(i)
    d.b, d.H, d.W, d.vn = b, h, w, vn
    return d


def _params(round_hyp_num, inlier_thresh, confidence=0.99, max_iter=100, min_num=100, max_num=30000, seed=None,
            idxs=None, keep=None, min_hyp_num=0, topk=0):
    p = _lib.VoteParams()
    p.round_hyp_num = int(round_hyp_num)
    p.inlier_thresh = float(inlier_thresh)
    p.confidence = float(confidence)
    p.max_iter = int(max_iter)
    p.min_num = int(min_num)
    p.max_num = int(max_num)
    p.seed = _draw_seed() if seed is None else int(seed) & (2 ** 64 - 1)
    p.idxs = idxs.data_ptr() if idxs is not None else None
    p.keep = keep.data_ptr() if keep is not None else None
    p.min_hyp_num = int(min_hyp_num)
    p.topk = int(topk)
    return p


def _lead(d):
    """(leading dimensions of a descriptor's per-image arrays, their product)."""
    return ((d.b,), d.b) if d.ncls == 0 else ((d.b, d.ncls), d.b * d.ncls)


def _aux(x, dtype, device, shape, name):
    if x is None:
        return None
    x = torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()
    if tuple(x.shape) != tuple(shape):
        raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(x.shape)}")
    return x


def _v3(d, mask, vertex, round_hyp_num, inlier_thresh, confidence, max_iter, min_num, max_num, _idxs, _keep, _diag,
        _seed, _workspace, out=None, conf_thresh=None):
    dev = vertex.device
    h, w, vn = d.H, d.W, d.vn
    # the leading dimensions of every per-image array: (b,), or (b, classes) for a multi-object descriptor
    lead, nimg = _lead(d)
    idxs = _aux(_idxs, torch.int32, dev, (*lead, round_hyp_num, vn, 2), "_idxs")
    keep = _aux(_keep, torch.uint8, dev, (*lead, h, w), "_keep")
    prm = _params(round_hyp_num, inlier_thresh, confidence, max_iter, min_num, max_num, _seed, idxs, keep)
    L = _lib.load()
    nbytes = L.pv_v3_workspace_size(nimg, h, w, vn, round_hyp_num)
    work = _workspace or _default_ws
    if out is None:
        out = torch.empty((*lead, vn, 2), dtype=torch.float32, device=dev)
    diag = None
    dt = {}
    if _diag is not None:
        dt = dict(hyp=torch.empty((*lead, round_hyp_num, vn, 2), dtype=torch.float32, device=dev),
                  counts=torch.empty((*lead, vn, round_hyp_num), dtype=torch.int32, device=dev),
                  win_idx=torch.empty((*lead, vn), dtype=torch.int32, device=dev),
                  win_ratio=torch.empty((*lead, vn), dtype=torch.float32, device=dev),
                  tn=torch.empty(lead, dtype=torch.int32, device=dev),
                  iters=torch.empty(lead, dtype=torch.int32, device=dev),
                  ata=torch.empty((*lead, vn, 2, 2), dtype=torch.float32, device=dev),
                  atb=torch.empty((*lead, vn, 2), dtype=torch.float32, device=dev))
        diag = _lib.V3Diag(**{k: v.data_ptr() for k, v in dt.items()})
    conf = None if conf_thresh is None else torch.empty((*lead, vn), dtype=torch.float32, device=dev)
    ws = work.get(dev, nbytes)
    with torch.cuda.device(dev):
        try:
            if conf_thresh is None:
                code = L.pv_ransac_voting_v3(ctypes.byref(d), ctypes.byref(prm), out.data_ptr(), ws.data_ptr(), nbytes,
                                             ctypes.byref(diag) if diag is not None else None,
                                             torch.cuda.current_stream(dev).cuda_stream)
            else:
                code = L.pv_ransac_voting_v5(ctypes.byref(d), ctypes.byref(prm), float(conf_thresh), out.data_ptr(),
                                             conf.data_ptr(), ws.data_ptr(), nbytes,
                                             ctypes.byref(diag) if diag is not None else None,
                                             torch.cuda.current_stream(dev).cuda_stream)
        finally:
            work.done(dev)
    _lib.check(code, "ransac_voting_layer_v3" if conf_thresh is None else "ransac_voting_layer_v5")
    if _diag is not None:
        _diag.update(dt)
    # keep the inputs alive until the kernels that read them have been queued
    del mask, idxs, keep
    return out if conf is None else (out, conf)


def ransac_voting_layer_v3(mask, vertex, round_hyp_num, inlier_thresh=0.99, confidence=0.99, max_iter=100,
                           min_num=100, max_num=30000, *, _idxs=None, _keep=None, _diag=None, _seed=None,
                           _workspace=None):
    """RV:520-604.  mask [b,h,w] (int64/int32/uint8/bool), vertex [b,h,w,vn,2]
    (f32 or f16, any strides -- e.g. the permuted view of vertex_pred) ->
    f32 [b,vn,2] on the same device.

    Test hooks (keyword-only, not in the reference): ``_idxs`` [b,hn,vn,2]
    pixel pairs instead of the RNG, ``_keep`` [b,h,w] downsampling mask,
    ``_diag`` dict filled with intermediate device tensors, ``_seed``."""
    d = _desc(mask, vertex)
    return _v3(d, mask, vertex, round_hyp_num, inlier_thresh, confidence, max_iter, min_num, max_num, _idxs,
               _keep, _diag, _seed, _workspace)


def ransac_voting_layer_v5(mask, vertex, round_hyp_num, inlier_thresh=0.999, confidence=0.99, max_iter=20,
                           min_num=5, max_num=100, *, _idxs=None, _keep=None, _diag=None, _seed=None,
                           _workspace=None):
    """RV:769-864 (the uncertainty eval wrapper's layer, TRAIN:123): v3 with
    v5's defaults, returning (points f32 [b,vn,2], confidence f32 [b,vn]) --
    each refined keypoint's inlier ratio at 0.999 (RV:856-858)."""
    d = _desc(mask, vertex)
    return _v3(d, mask, vertex, round_hyp_num, inlier_thresh, confidence, max_iter, min_num, max_num, _idxs,
               _keep, _diag, _seed, _workspace, conf_thresh=0.999)


def ransac_motion_voting(mask, vertex):
    """RV:966-987: mask [b,h,w], vertex [b,h,w,vn,2] holding offsets ->
    f32 [b,vn,2], the foreground mean of vertex + (col, row) (zeros for an
    empty mask), in one HIP kernel."""
    d = _desc(mask, vertex)
    out = torch.empty((d.b, d.vn, 2), dtype=torch.float32, device=vertex.device)
    with torch.cuda.device(vertex.device):
        code = _lib.load().pv_ransac_motion_voting(ctypes.byref(d), out.data_ptr(),
                                                   torch.cuda.current_stream(vertex.device).cuda_stream)
    _lib.check(code, "ransac_motion_voting")
    return out


def ransac_voting_layer_v3_from_network(seg_pred, vertex_pred, round_hyp_num, inlier_thresh=0.99, confidence=0.99,
                                        max_iter=100, min_num=100, max_num=30000, *, _idxs=None, _keep=None,
                                        _diag=None, _seed=None, _workspace=None, out=None):
    """EvalWrapper (DEMO:46-55) fused: network outputs seg_pred [b,2,h,w] and
    vertex_pred [b,2vn,h,w] straight in -- the argmax and the permute/view are
    done inside the compaction kernel (no int64 mask, no strided copy)."""
    b, c, h, w = vertex_pred.shape
    vertex = vertex_pred.permute(0, 2, 3, 1).view(b, h, w, c // 2, 2)
    d = _desc(seg_pred, vertex, seg=True)
    return _v3(d, seg_pred, vertex, round_hyp_num, inlier_thresh, confidence, max_iter, min_num, max_num, _idxs,
               _keep, _diag, _seed, _workspace, out=out)


def _evd_common(mask, vertex, round_hyp_num, min_hyp_num, inlier_thresh, min_num, max_num, topk, _idxs, _keep,
                _seed, _workspace, d=None):
    if d is None:
        d = _desc(mask, vertex)
    dev = vertex.device
    rounds = int(np.ceil(min_hyp_num / round_hyp_num))
    nh = rounds * round_hyp_num
    lead, nimg = _lead(d)
    idxs = _aux(_idxs, torch.int32, dev, (*lead, nh, d.vn, 2), "_idxs")
    keep = _aux(_keep, torch.uint8, dev, (*lead, d.H, d.W), "_keep")
    prm = _params(round_hyp_num, inlier_thresh, 0.99, 100, min_num, max_num, _seed, idxs, keep,
                  min_hyp_num=min_hyp_num, topk=topk)
    L = _lib.load()
    nbytes = L.pv_v3_workspace_size(nimg, d.H, d.W, d.vn, nh)
    return d, prm, nbytes, (idxs, keep), _workspace or _default_ws


def estimate_voting_distribution_with_mean(mask, vertex, mean, round_hyp_num=256, min_hyp_num=4096, topk=128,
                                           inlier_thresh=0.99, min_num=20, max_num=30000, output_hyp=False, *,
                                           _idxs=None, _keep=None, _seed=None, _workspace=None):
    """RV:333-406 -> (mean, cov [b,vn,2,2]).  ``_idxs`` is [b, rounds*round_hyp_num, vn, 2]."""
    d, prm, nbytes, keepalive, work = _evd_common(mask, vertex, round_hyp_num, min_hyp_num, inlier_thresh, min_num,
                                                  max_num, topk, _idxs, _keep, _seed, _workspace)
    dev = vertex.device
    mean_c = mean.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(mean_c.shape) != (d.b, d.vn, 2):
        raise RuntimeError("mean must be [b,vn,2]")
    cov = torch.empty((d.b, d.vn, 2, 2), dtype=torch.float32, device=dev)
    ws = work.get(dev, nbytes)
    with torch.cuda.device(dev):
        try:
            code = _lib.load().pv_estimate_voting_distribution_with_mean(
                ctypes.byref(d), ctypes.byref(prm), mean_c.data_ptr(), cov.data_ptr(), ws.data_ptr(), nbytes,
                torch.cuda.current_stream(dev).cuda_stream)
        finally:
            work.done(dev)
    _lib.check(code, "estimate_voting_distribution_with_mean")
    return mean, cov


def estimate_voting_distribution(mask, vertex, round_hyp_num=256, min_hyp_num=4096, topk=128, inlier_thresh=0.99,
                                 min_num=5, max_num=30000, *, _idxs=None, _keep=None, _seed=None, _workspace=None):
    """RV:263-331 -> (mean [b,vn,2], cov [b,vn,2,2]); topk ties lowest index first."""
    d, prm, nbytes, keepalive, work = _evd_common(mask, vertex, round_hyp_num, min_hyp_num, inlier_thresh, min_num,
                                                  max_num, topk, _idxs, _keep, _seed, _workspace)
    dev = vertex.device
    mean = torch.empty((d.b, d.vn, 2), dtype=torch.float32, device=dev)
    cov = torch.empty((d.b, d.vn, 2, 2), dtype=torch.float32, device=dev)
    ws = work.get(dev, nbytes)
    with torch.cuda.device(dev):
        try:
            code = _lib.load().pv_estimate_voting_distribution(
                ctypes.byref(d), ctypes.byref(prm), mean.data_ptr(), cov.data_ptr(), ws.data_ptr(), nbytes,
                torch.cuda.current_stream(dev).cuda_stream)
        finally:
            work.done(dev)
    _lib.check(code, "estimate_voting_distribution")
    return mean, cov


# --------------------------------------------------------------------------
# multi-object frames: one label map, the keypoints of every class in one call
# (the reference loops over the classes with mask[bi] == k + 1, RV:273, RV:340)
# --------------------------------------------------------------------------
_LABEL_KIND = {torch.int64: _lib.PV_MASK_I64, torch.uint8: _lib.PV_MASK_U8, torch.int32: _lib.PV_MASK_I32}


def _desc_multi(label, vertex, class_num, seg=False):
    """The descriptor of a multi-object call.  Shapes and dtypes are checked
    first (on any device), then that the tensors are on one ROCm device."""
    if not (isinstance(vertex, torch.Tensor) and isinstance(label, torch.Tensor)):
        raise RuntimeError("label and vertex must be tensors")
    class_num = int(class_num)
    if not 1 <= class_num <= 64:
        raise RuntimeError(f"class_num must be in [1, 64], got {class_num}")
    if vertex.dim() != 5 or vertex.shape[4] != 2:
        raise RuntimeError("vertex must be [b,h,w,class_num*vn,2]")
    b, h, w, ch, _ = vertex.shape
    if ch == 0 or ch % class_num != 0:
        raise RuntimeError(f"vertex has {ch} keypoint channels, not divisible by class_num = {class_num}")
    if ch // class_num > 64:
        raise RuntimeError("at most 64 keypoints per class")
    if vertex.dtype not in _VERTEX_KIND:
        raise RuntimeError(f"vertex dtype {vertex.dtype} not supported (float32/float16)")
    if seg:
        if label.dim() != 4 or label.shape[1] != class_num + 1 or (label.shape[0], *label.shape[2:]) != (b, h, w):
            raise RuntimeError(f"seg_pred must be [b,class_num+1,h,w] = {(b, class_num + 1, h, w)}, "
                               f"got {tuple(label.shape)}")
        if label.dtype not in _SEG_KIND:
            raise RuntimeError(f"seg_pred dtype {label.dtype} not supported")
    else:
        if tuple(label.shape) != (b, h, w):
            raise RuntimeError(f"label must be [b,h,w] = {(b, h, w)}, got {tuple(label.shape)}")
        if label.dtype not in _LABEL_KIND:
            raise RuntimeError(f"label dtype {label.dtype} not supported (int64/int32/uint8)")
    if not vertex.is_cuda:
        raise RuntimeError("vertex must be a CUDA tensor")
    if not label.is_cuda:
        raise RuntimeError(("seg_pred" if seg else "label") + " must be a CUDA tensor")
    if label.device != vertex.device:
        raise RuntimeError("label and vertex must be on the same device")
    d = _lib.ImageDesc()
    d.mask = label.data_ptr()
    d.mask_kind = (_SEG_KIND if seg else _LABEL_KIND)[label.dtype]
    for i in range(label.dim()):
        d.mask_strides[i] = label.stride(i)
    d.vertex = vertex.data_ptr()
    d.vertex_kind = _VERTEX_KIND[vertex.dtype]
    for i in range(5):
        d.vertex_strides[i] = vertex.stride(i)
    d.b, d.H, d.W, d.vn, d.ncls = b, h, w, ch // class_num, class_num
    return d


def ransac_voting_layer_v3_multi(label, vertex, class_num, round_hyp_num, inlier_thresh=0.99, confidence=0.99,
                                 max_iter=100, min_num=100, max_num=30000, *, _idxs=None, _keep=None, _diag=None,
                                 _seed=None, _workspace=None):
    """``ransac_voting_layer_v3`` for every class of a multi-object frame in
    one call: label [b,h,w] (int64/int32/uint8; a pixel belongs to class c iff
    its label equals c + 1, 0 and labels above class_num to none), vertex
    [b,h,w,class_num*vn,2] (f32 or f16, any strides; class c's keypoints are
    channels [c*vn, (c+1)*vn)) -> f32 [b,class_num,vn,2]: what v3 gives for
    ``label == c + 1`` and that slice of vertex, zeros for a class with fewer
    than ``min_num`` pixels.

    Test hooks: ``_idxs`` [b,class_num,hn,vn,2], ``_keep`` [b,class_num,h,w],
    ``_diag`` (tensors with leading [b,class_num]), ``_seed``."""
    d = _desc_multi(label, vertex, class_num)
    return _v3(d, label, vertex, round_hyp_num, inlier_thresh, confidence, max_iter, min_num, max_num, _idxs,
               _keep, _diag, _seed, _workspace)


def ransac_voting_layer_v3_multi_from_network(seg_pred, vertex_pred, class_num, round_hyp_num, inlier_thresh=0.99,
                                              confidence=0.99, max_iter=100, min_num=100, max_num=30000, *,
                                              _idxs=None, _keep=None, _diag=None, _seed=None, _workspace=None,
                                              out=None):
    """The multi-object network's outputs straight in: seg_pred
    [b,class_num+1,h,w] logits and vertex_pred [b,2*class_num*vn,h,w] (f32 or
    f16, any strides).  The argmax over the channels (torch.argmax: first
    maximum, NaN is the maximum) and the permute/view are done inside the
    kernels -> f32 [b,class_num,vn,2]."""
    if not (isinstance(vertex_pred, torch.Tensor) and vertex_pred.dim() == 4):
        raise RuntimeError("vertex_pred must be [b,2*class_num*vn,h,w]")
    b, c, h, w = vertex_pred.shape
    if c % 2 != 0:
        raise RuntimeError(f"vertex_pred has {c} channels, not 2*class_num*vn")
    vertex = vertex_pred.permute(0, 2, 3, 1).unflatten(3, (c // 2, 2))
    d = _desc_multi(seg_pred, vertex, class_num, seg=True)
    if out is not None and (tuple(out.shape) != (b, d.ncls, d.vn, 2) or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != vertex.device):
        raise RuntimeError("out must be a contiguous f32 [b,class_num,vn,2] tensor on the inputs' device")
    return _v3(d, seg_pred, vertex, round_hyp_num, inlier_thresh, confidence, max_iter, min_num, max_num, _idxs,
               _keep, _diag, _seed, _workspace, out=out)


def estimate_voting_distribution_with_mean_multi(label, vertex, mean, class_num, round_hyp_num=256,
                                                 min_hyp_num=4096, topk=128, inlier_thresh=0.99, min_num=20,
                                                 max_num=30000, *, _idxs=None, _keep=None, _seed=None,
                                                 _workspace=None):
    """``estimate_voting_distribution_with_mean`` for every class of a
    multi-object frame: label and vertex as ``ransac_voting_layer_v3_multi``,
    mean [b,class_num,vn,2] -> (mean, cov [b,class_num,vn,2,2]).  ``_idxs`` is
    [b,class_num,rounds*round_hyp_num,vn,2]."""
    d = _desc_multi(label, vertex, class_num)
    d, prm, nbytes, keepalive, work = _evd_common(label, vertex, round_hyp_num, min_hyp_num, inlier_thresh, min_num,
                                                  max_num, topk, _idxs, _keep, _seed, _workspace, d=d)
    dev = vertex.device
    if not isinstance(mean, torch.Tensor) or tuple(mean.shape) != (d.b, d.ncls, d.vn, 2):
        raise RuntimeError("mean must be [b,class_num,vn,2]")
    mean_c = mean.to(device=dev, dtype=torch.float32).contiguous()
    cov = torch.empty((d.b, d.ncls, d.vn, 2, 2), dtype=torch.float32, device=dev)
    ws = work.get(dev, nbytes)
    with torch.cuda.device(dev):
        try:
            code = _lib.load().pv_estimate_voting_distribution_with_mean(
                ctypes.byref(d), ctypes.byref(prm), mean_c.data_ptr(), cov.data_ptr(), ws.data_ptr(), nbytes,
                torch.cuda.current_stream(dev).cuda_stream)
        finally:
            work.done(dev)
    _lib.check(code, "estimate_voting_distribution_with_mean_multi")
    return mean, cov


def b_inv(b_mat: torch.Tensor) -> torch.Tensor:
    """RV:503-518 with the semantics of the pinned torch (gesv present):
    batched inverse, or the identity for the WHOLE batch when any matrix is
    singular (the reference's bare ``except``)."""
    eye = b_mat.new_ones(b_mat.size(-1)).diag().expand_as(b_mat)
    try:
        return torch.linalg.solve(b_mat, eye)
    except RuntimeError:       # torch.linalg.LinAlgError subclasses RuntimeError
        return eye
