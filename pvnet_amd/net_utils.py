"""PVNet's training objective on the device (include/pvloss.h): what the reference computes in
``lib/utils/net_utils.py`` and ``tools/train_linemod.py``.

* :func:`pvnet_loss`               per-image cross-entropy of the segmentation, mask-weighted
  smooth-L1 of the vector field, and the precision / recall counts, for ``class_num`` objects in one
  label map; differentiable in both predictions
* :func:`smooth_l1_loss`           the reference's function of that name (``class_num = 1``)
* :func:`compute_precision_recall` the reference's function of that name (``class_num = 1``)

The inputs are what the network emits (``seg_pred [b, class_num+1, H, W]``, ``vertex_pred
[b, 2*class_num*vn, H, W]``) and what :func:`pvnet_amd.render.render_ground_truth` makes (a label
map, class c = label c + 1, and a vector field in either of its layouts).  The backward recomputes
from the inputs: no per-element gradient is kept between the two passes.  Nothing synchronises and
nothing is read back, so a training step can be captured into a graph.  No CPU fallback: without
libpvloss.so or a ROCm device the calls raise.

Difference from the reference: an element of the vector field whose weight is 0 (the
background, another class's channels, a label outside 1..class_num) contributes exactly 0 and gets
gradient exactly 0 whatever it holds, NaN and inf included; the reference multiplies by the weight,
so a NaN there spreads.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _loss_lib
from .ransac_voting_gpu import VotingWorkspace

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own

_KIND = {torch.float32: _loss_lib.PV_LOSS_F32, torch.float16: _loss_lib.PV_LOSS_F16}
_LABEL_KIND = {torch.int64: _loss_lib.PV_LOSS_LABEL_I64, torch.uint8: _loss_lib.PV_LOSS_LABEL_U8,
               torch.int32: _loss_lib.PV_LOSS_LABEL_I32}


def _field_view(t, name, b, H, W, class_num, vn=None):
    """-> (the logical [b, H, W, class_num*vn, 2] view of a field in either layout, vn)."""
    if not isinstance(t, torch.Tensor) or t.dtype not in _KIND or t.dim() not in (4, 5):
        raise RuntimeError(f"{name} must be a float32 / float16 tensor, [b, 2*class_num*vn, H, W] or [b, H, W, class_num*vn, 2]")
    if t.dim() == 4:
        ok = tuple(t.shape[0:1] + t.shape[2:]) == (b, H, W) and t.shape[1] >= 2 * class_num and t.shape[1] % (2 * class_num) == 0
        n = int(t.shape[1]) // (2 * class_num)
    else:
        ok = tuple(t.shape[:3]) == (b, H, W) and t.shape[4] == 2 and t.shape[3] >= class_num and t.shape[3] % class_num == 0
        n = int(t.shape[3]) // class_num
    if not ok or (vn is not None and n != vn):
        want = "vn" if vn is None else str(vn)
        raise RuntimeError(f"{name} has shape {list(t.shape)}; expected [{b}, 2*{class_num}*{want}, {H}, {W}] or "
                           f"[{b}, {H}, {W}, {class_num}*{want}, 2]")
    view = t if t.dim() == 5 else t.permute(0, 2, 3, 1).unflatten(3, (class_num * n, 2))
    return view, n


def _check(seg, vertex, label, target, class_num, sigma):
    """Shapes and kinds first, devices last; -> (b, H, W, class_num, vn, vertex view, target view, sigma)."""
    class_num = int(class_num)
    if not 1 <= class_num <= _loss_lib.PV_LOSS_MAX_CLASSES:
        raise RuntimeError(f"class_num must be in 1..{_loss_lib.PV_LOSS_MAX_CLASSES}")
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise RuntimeError("sigma must be a positive number")
    if not isinstance(label, torch.Tensor) or label.dim() != 3 or label.dtype not in _LABEL_KIND:
        raise RuntimeError("label must be a uint8 / int32 / int64 [b, H, W] tensor")
    b, H, W = (int(s) for s in label.shape)
    if H < 1 or W < 1:
        raise RuntimeError("label must have at least one pixel per image")
    if seg is None and vertex is None:
        raise RuntimeError("at least one of the two predictions is needed")
    if seg is not None:
        if not isinstance(seg, torch.Tensor) or seg.dtype not in _KIND or tuple(seg.shape) != (b, class_num + 1, H, W):
            raise RuntimeError(f"seg_pred must be a float32 / float16 tensor of shape [{b}, {class_num + 1}, {H}, {W}]")
    vv = tv = None
    vn = 1
    if vertex is not None:
        vv, vn = _field_view(vertex, "vertex_pred", b, H, W, class_num)
        tv, _ = _field_view(target, "vertex_target", b, H, W, class_num, vn)
    tensors = [t for t in (seg, vertex, label, target) if t is not None]
    if any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError("the predictions, the label map and the target must live on the ROCm device (no CPU path)")
    if any(t.device != label.device for t in tensors):
        raise RuntimeError("the predictions, the label map and the target must be on one device")
    return b, H, W, class_num, vn, vv, tv, sigma


def _desc(seg, vv, tv, label, b, H, W, class_num, vn, sigma):
    d = _loss_lib.LossDesc()
    d.label, d.label_kind = label.data_ptr(), _LABEL_KIND[label.dtype]
    for i in range(3):
        d.label_strides[i] = label.stride(i)
    if seg is not None:
        d.seg, d.seg_kind = seg.data_ptr(), _KIND[seg.dtype]
        for i in range(4):
            d.seg_strides[i] = seg.stride(i)
    if vv is not None:
        d.vertex, d.vertex_kind, d.target, d.target_kind = vv.data_ptr(), _KIND[vv.dtype], tv.data_ptr(), _KIND[tv.dtype]
        for i in range(5):
            d.vertex_strides[i] = vv.stride(i)
            d.target_strides[i] = tv.stride(i)
    d.b, d.H, d.W, d.ncls, d.vn, d.sigma = b, H, W, class_num, vn, sigma
    return d


class _Loss(torch.autograd.Function):
    """(seg | None, vertex | None, label, target | None) -> (loss_seg, loss_vertex, fg, counts); the
    loss of an absent term is 0."""

    @staticmethod
    def forward(ctx, seg, vertex, label, target, class_num, sigma):
        b, H, W, ncls, vn, vv, tv, sigma = _check(seg, vertex, label, target, class_num, sigma)
        dev = label.device
        loss_seg = torch.zeros((b,), dtype=torch.float32, device=dev)
        loss_vertex = torch.zeros((b,), dtype=torch.float32, device=dev)
        fg = torch.zeros((b,), dtype=torch.int64, device=dev)
        counts = torch.zeros((b, ncls, 3), dtype=torch.int64, device=dev)
        if b > 0:
            L = _loss_lib.load()
            need = int(L.pv_loss_workspace_size(b, H, W, ncls))
            if need == 0:
                raise RuntimeError("bad sizes for libpvloss.so's workspace")
            ws = _ws.get(dev, need)
            d = _desc(seg, vv, tv, label, b, H, W, ncls, vn, sigma)
            o = _loss_lib.LossOut(loss_seg.data_ptr(), loss_vertex.data_ptr(), fg.data_ptr(), counts.data_ptr())
            with torch.cuda.device(dev):
                _loss_lib.check(L.pv_loss_forward(ctypes.byref(d), ctypes.byref(o), ws.data_ptr(), ws.numel(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "pv_loss_forward")
        ctx.save_for_backward(seg, vertex, label, target, fg)
        ctx.args = (ncls, sigma)
        # a loss whose prediction is absent or wants no gradient carries none either
        constant = [loss for loss, pred, i in ((loss_seg, seg, 0), (loss_vertex, vertex, 1))
                    if pred is None or not ctx.needs_input_grad[i]]
        ctx.mark_non_differentiable(fg, counts, *constant)
        return loss_seg, loss_vertex, fg, counts

    @staticmethod
    def backward(ctx, g_seg, g_vertex, _g_fg, _g_counts):
        seg, vertex, label, target, fg = ctx.saved_tensors
        ncls, sigma = ctx.args
        want_seg = seg is not None and ctx.needs_input_grad[0]
        want_vertex = vertex is not None and ctx.needs_input_grad[1]
        if not (want_seg or want_vertex):
            return None, None, None, None, None, None
        seg_in, vertex_in = (seg if want_seg else None), (vertex if want_vertex else None)
        b, H, W, ncls, vn, vv, tv, sigma = _check(seg_in, vertex_in, label, target if want_vertex else None, ncls, sigma)
        dev = label.device
        d = _desc(seg_in, vv, tv, label, b, H, W, ncls, vn, sigma)
        g = _loss_lib.LossGrad()
        grad_seg = grad_vertex = None
        if want_seg:
            g_seg = g_seg.to(torch.float32).contiguous()
            grad_seg = torch.empty_like(seg)
            g.g_seg, g.grad_seg = g_seg.data_ptr(), grad_seg.data_ptr()
            for i in range(4):
                g.grad_seg_strides[i] = grad_seg.stride(i)
        if want_vertex:
            g_vertex = g_vertex.to(torch.float32).contiguous()
            grad_vertex = torch.empty_like(vertex)
            gv, _ = _field_view(grad_vertex, "grad_vertex", b, H, W, ncls, vn)
            g.g_vertex, g.grad_vertex, g.fg = g_vertex.data_ptr(), grad_vertex.data_ptr(), fg.data_ptr()
            for i in range(5):
                g.grad_vertex_strides[i] = gv.stride(i)
        if b > 0:
            with torch.cuda.device(dev):
                _loss_lib.check(_loss_lib.load().pv_loss_backward(ctypes.byref(d), ctypes.byref(g),
                                                                  torch.cuda.current_stream(dev).cuda_stream),
                                "pv_loss_backward")
        return grad_seg, grad_vertex, None, None, None, None


def _stats(fg, counts):
    tp, fp, fn = counts[..., 0], counts[..., 1], counts[..., 2]
    tpf, fpf, fnf = tp.to(torch.float32), fp.to(torch.float32), fn.to(torch.float32)
    return {"fg": fg, "tp": tp, "fp": fp, "fn": fn,
            "precision": (tpf + 1) / (tpf + fpf + 1), "recall": (tpf + 1) / (tpf + fnf + 1)}


def pvnet_loss(seg_pred: torch.Tensor, vertex_pred: torch.Tensor, label: torch.Tensor, vertex_target: torch.Tensor,
               class_num: int = 1, sigma: float = 1.0):
    """The two terms of PVNet's objective, per image -> ``(loss_seg [b], loss_vertex [b], stats)``.

    seg_pred       [b, class_num+1, H, W] logits, float32 or float16, any strides
    vertex_pred    [b, 2*class_num*vn, H, W] (what the network emits) or [b, H, W, class_num*vn, 2]
    label          [b, H, W] uint8 / int32 / int64; class c = label c + 1, 0 the background; a label
                   outside 0..class_num is ignored by the cross-entropy (the mean still divides by
                   H*W) and is not foreground
    vertex_target  the ground-truth field in either layout of ``vertex_field``, float32 or float16
    sigma          the smooth-L1's sigma (> 0)

    ``loss_seg[i]`` is the mean over pixels of the cross-entropy; ``loss_vertex[i]`` is the smooth-L1
    summed over the foreground pixels' own channels, divided by ``2*vn*fg_i + 1e-3``.  Both are
    float32 and differentiable in the predictions; the gradients have the predictions' dtype.  A
    float16 gradient of a mean over H*W pixels is subnormal at full frames: scale the loss, as in any
    float16 training.  ``stats`` holds ``fg`` int64 [b] and, per class [b, class_num], ``tp``, ``fp``,
    ``fn`` (int64; the prediction is the arg-max of the logits, a tie going to the lowest index),
    ``precision = (tp+1)/(tp+fp+1)`` and ``recall = (tp+1)/(tp+fn+1)``; none of them carries a
    gradient."""
    if seg_pred is None or vertex_pred is None or vertex_target is None:
        raise RuntimeError("pvnet_loss takes both predictions and the target")
    loss_seg, loss_vertex, fg, counts = _Loss.apply(seg_pred, vertex_pred, label, vertex_target, class_num, sigma)
    return loss_seg, loss_vertex, _stats(fg, counts)


def smooth_l1_loss(vertex_pred: torch.Tensor, vertex_targets: torch.Tensor, vertex_weights: torch.Tensor,
                   sigma: float = 1.0, normalize: bool = True, reduce: bool = True):
    """The reference's ``smooth_l1_loss`` for one object: ``vertex_weights`` [b, 1, H, W] is the mask,
    non-zero meaning foreground.  Per image the sum over the foreground divided by
    ``2*vn*fg + 1e-3``; ``reduce`` takes the mean over the batch.  ``normalize=False`` is not built."""
    if not normalize:
        raise NotImplementedError("smooth_l1_loss(normalize=False) is not built: only the normalised form is")
    if not isinstance(vertex_weights, torch.Tensor) or vertex_weights.dim() != 4 or vertex_weights.shape[1] != 1:
        raise RuntimeError("vertex_weights must be a [b, 1, H, W] tensor")
    label = (vertex_weights[:, 0] != 0).to(torch.uint8)
    _, loss, _, _ = _Loss.apply(None, vertex_pred, label, vertex_targets, 1, sigma)
    return loss.mean() if reduce else loss


def compute_precision_recall(scores: torch.Tensor, target: torch.Tensor, reduce: bool = False):
    """The reference's ``compute_precision_recall`` for one object: ``scores`` [b, 2, H, W] logits,
    ``target`` [b, H, W] the mask (uint8 / int32 / int64) -> ``(precision [b], recall [b])``, or their
    means with ``reduce``."""
    _, _, fg, counts = _Loss.apply(scores, None, target, None, 1, 1.0)
    st = _stats(fg, counts)
    precision, recall = st["precision"][:, 0], st["recall"][:, 0]
    return (precision.mean(), recall.mean()) if reduce else (precision, recall)
