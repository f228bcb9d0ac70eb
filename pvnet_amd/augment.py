"""Training augmentation on the device (include/pvaugment.h): what the reference's
``LineModDatasetRealAug`` does on the host, image by image, as one affine map and one colour jitter
per image of a batch.

* :func:`label_stats` counts a label map's foreground and finds its centroid sums and box.
* :func:`random_params` draws one map and one jitter per image -> :class:`AugmentParams`.
* :func:`apply` warps the u8 image (bilinear) and the label map (nearest), replaces the background,
  runs brightness, contrast, saturation and hue in that order and normalises to the network's input.
* :func:`transform_keypoints` moves 2-D keypoints with the forward map.
* :func:`augment_ground_truth` chains them and ``render.vertex_field``: its result is what ``PVNet``
  and ``pvnet_loss`` take.

The map is a rotation about the foreground's centroid, a scale, and a shift of the centroid to a
drawn target: ``rotate_instance``, ``crop_resize_instance_v1`` and ``crop_or_padding_to_fixed_size``
folded into one resampling.  It is a different parametrisation, not a replay of the reference's
random stream.  Blur, noise and occlusion pasting are ``pvnet_amd.compose``'s (include/pvcompose.h);
flips and file reading are not in this package.

Nothing is read back and nothing synchronises, so a call can be captured into a graph; the draws
depend on a device ``state`` = (seed, first sample index) that the caller advances.  No CPU
fallback: without libpvaugment.so or a ROCm device the calls raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _augment_lib as _A
from .ransac_voting_gpu import VotingWorkspace

_ws = VotingWorkspace(per_stream=True)      # one scratch buffer per (device, stream); a capture gets its own

_LABEL_KIND = {torch.int64: _A.PV_AUG_LABEL_I64, torch.uint8: _A.PV_AUG_LABEL_U8, torch.int32: _A.PV_AUG_LABEL_I32}
_OUT_KIND = {torch.float32: _A.PV_AUG_F32, torch.float16: _A.PV_AUG_F16}
_STEPS = {"brightness": _A.PV_AUG_BRIGHTNESS, "contrast": _A.PV_AUG_CONTRAST, "saturation": _A.PV_AUG_SATURATION,
          "hue": _A.PV_AUG_HUE}
ALL_STEPS = tuple(_STEPS)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_STATE_DTYPES = (torch.int64,) + ((torch.uint64,) if hasattr(torch, "uint64") else ())


class AugmentParams(NamedTuple):
    """fwd f64 [b, 2, 3]: what keypoints undergo (output = fwd (x, y, 1)); inv f64 [b, 2, 3]: its
    inverse, what the sampler uses; color f32 [b, 4] = (brightness, contrast, saturation factors, hue shift)."""
    fwd: torch.Tensor
    inv: torch.Tensor
    color: torch.Tensor


def _check_label(label):
    if not isinstance(label, torch.Tensor) or label.dim() != 3 or label.dtype not in _LABEL_KIND:
        raise RuntimeError("label must be a uint8 / int32 / int64 [b, H, W] tensor")
    b, H, W = (int(s) for s in label.shape)
    if not (1 <= H <= _A.PV_AUG_MAX_DIM and 1 <= W <= _A.PV_AUG_MAX_DIM):
        raise RuntimeError("label must have 1..2^20 rows and columns")
    return b, H, W


def _check_class_num(class_num):
    class_num = int(class_num)
    if not 1 <= class_num <= _A.PV_AUG_MAX_CLASSES:
        raise RuntimeError(f"class_num must be in 1..{_A.PV_AUG_MAX_CLASSES}")
    return class_num


def _check_out_size(out_size, default=None):
    if out_size is None:
        out_size = default
    try:
        Ho, Wo = (int(s) for s in out_size)
    except (TypeError, ValueError):
        raise RuntimeError("out_size must be (Ho, Wo)") from None
    if not (1 <= Ho <= _A.PV_AUG_MAX_DIM and 1 <= Wo <= _A.PV_AUG_MAX_DIM):
        raise RuntimeError("out_size must be (Ho, Wo) with both in 1..2^20")
    return Ho, Wo


def _pair(v, name, n=2):
    try:
        t = tuple(float(x) for x in v)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name} must be {n} numbers") from None
    if len(t) != n or any(x != x or x in (float("inf"), -float("inf")) for x in t):
        raise RuntimeError(f"{name} must be {n} finite numbers")
    return t


def _triple(v, name):
    if isinstance(v, (int, float)):
        v = (v, v, v)
    return _pair(v, name, 3)


def _need_device(t, name):
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be a device tensor (no CPU path)")
    return t.device


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def label_stats(label: torch.Tensor, class_num: int) -> torch.Tensor:
    """label [b, H, W] (uint8 / int32 / int64, any strides) -> int64 [b, 8] = (count of pixels with
    a label in 1..class_num, sum x, sum y, xmin, ymin, xmax, ymax, 0); the box of an image without
    foreground is (W, H, -1, -1).  Exact integers, whatever the order."""
    b, H, W = _check_label(label)
    class_num = _check_class_num(class_num)
    dev = _need_device(label, "label")
    stats = torch.empty((b, 8), dtype=torch.int64, device=dev)
    if b == 0:
        return stats
    d = _A.AugLabel(label.data_ptr(), (ctypes.c_int64 * 3)(*label.stride()), _LABEL_KIND[label.dtype], b, H, W)
    with torch.cuda.device(dev):
        _A.check(_A.load().pv_label_stats(ctypes.byref(d), class_num, stats.data_ptr(), _stream(dev)), "pv_label_stats")
    return stats


def random_params(label: torch.Tensor, class_num: int, out_size, state: torch.Tensor, rot_deg=(-30.0, 30.0),
                  scale=(0.8, 1.2), margin: float = 0.25, jitter=(0.1, 0.1, 0.05, 0.05)) -> AugmentParams:
    """One affine map and one colour jitter per image of ``label`` [b, H, W].

    out_size  (Ho, Wo) of the augmented frame
    state     device int64 (or uint64) [2] = (seed, first sample index), read and never written:
              image i uses sample index state[1] + i, so advance state[1] by b between calls
    rot_deg   the angle's range in degrees; scale: the scale's range; margin in [0, 0.5]: the
              foreground's centroid lands uniformly in [margin, 1 - margin] of the output frame
    jitter    (brightness, contrast, saturation, hue) half-widths, as torchvision's ColorJitter takes them

    The draws are include/pvaugment.h's counter-based generator; numpy reproduces them bit for bit."""
    b, H, W = _check_label(label)
    class_num = _check_class_num(class_num)
    Ho, Wo = _check_out_size(out_size)
    if not isinstance(state, torch.Tensor) or state.dtype not in _STATE_DTYPES or tuple(state.shape) != (2,) \
            or not state.is_contiguous():
        raise RuntimeError("state must be a contiguous int64 [2] tensor = (seed, first sample index)")
    rot, sc, jit = _pair(rot_deg, "rot_deg"), _pair(scale, "scale"), _pair(jitter, "jitter", 4)
    margin = float(margin)
    if not rot[0] <= rot[1]:
        raise RuntimeError("rot_deg must be (lo, hi) with lo <= hi")
    if not 0.0 < sc[0] <= sc[1]:
        raise RuntimeError("scale must be (lo, hi) with 0 < lo <= hi")
    if not 0.0 <= margin <= 0.5:
        raise RuntimeError("margin must be in [0, 0.5]")
    if any(not 0.0 <= j <= hi for j, hi in zip(jit, (1.0, 1.0, 1.0, 0.5))):
        raise RuntimeError("jitter must be (brightness, contrast, saturation) in [0, 1] and hue in [0, 0.5]")
    dev = _need_device(label, "label")
    if state.device != dev:
        raise RuntimeError("state must be on the label's device")
    stats = label_stats(label, class_num)
    fwd = torch.empty((b, 2, 3), dtype=torch.float64, device=dev)
    inv = torch.empty((b, 2, 3), dtype=torch.float64, device=dev)
    color = torch.empty((b, 4), dtype=torch.float32, device=dev)
    if b:
        r = _A.AugRanges((ctypes.c_double * 2)(*rot), (ctypes.c_double * 2)(*sc), margin, (ctypes.c_double * 4)(*jit),
                         b, H, W, Ho, Wo, 0)
        with torch.cuda.device(dev):
            _A.check(_A.load().pv_augment_params(ctypes.byref(r), stats.data_ptr(), state.data_ptr(), fwd.data_ptr(),
                                                 inv.data_ptr(), color.data_ptr(), _stream(dev)), "pv_augment_params")
    return AugmentParams(fwd, inv, color)


def apply(image: torch.Tensor, label: torch.Tensor, params: AugmentParams, background: torch.Tensor | None = None,
          fill=0, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32, out_size=None, out=None,
          steps=ALL_STEPS, channels_last: bool = False):
    """Warp, recolour and normalise a batch.

    image       uint8 [b, H, W, 3] device tensor, any strides (a [b, 3, H, W] tensor permuted is fine); one
                image of it, of the label map and of the background spans at most 2^31 - 1 elements
    label       uint8 / int32 / int64 [b, H, W], any strides
    params      :class:`AugmentParams` (only inv and color are used)
    background  optional uint8 [b, Ho, Wo, 3] or [1, Ho, Wo, 3] (shared): where the augmented label
                is 0 the colour is the background's pixel
    fill        the colour outside the source, 0..255: a number or three
    mean, std   the normalisation, on [0, 1] values
    dtype       float32 or float16 of the image returned
    out_size    (Ho, Wo); default (H, W)
    out         optional ``(image, label)`` to write into: [b, 3, Ho, Wo] of ``dtype`` and
                [b, Ho, Wo] of the label's dtype, any strides
    steps       which of "brightness", "contrast", "saturation", "hue" run (in that fixed order)
    channels_last  allocate the image in channels-last memory format

    Returns ``(image [b, 3, Ho, Wo], label [b, Ho, Wo])``.  The semantics are include/pvaugment.h's."""
    if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[3] != 3 or image.dtype != torch.uint8:
        raise RuntimeError("image must be a uint8 [b, H, W, 3] tensor")
    b, H, W = _check_label(label)
    if tuple(image.shape[:3]) != (b, H, W):
        raise RuntimeError(f"image must be a uint8 [b, H, W, 3] tensor matching the label's [{b}, {H}, {W}]")
    Ho, Wo = _check_out_size(out_size, (H, W))
    if not isinstance(params, AugmentParams) or not all(isinstance(t, torch.Tensor) for t in params):
        raise RuntimeError("params must be an AugmentParams of tensors")
    inv, color = params.inv, params.color
    if tuple(inv.shape) != (b, 2, 3) or inv.dtype != torch.float64 or tuple(color.shape) != (b, 4) \
            or color.dtype != torch.float32:
        raise RuntimeError("params must hold inv float64 [b, 2, 3] and color float32 [b, 4]")
    if background is not None:
        if not isinstance(background, torch.Tensor) or background.dtype != torch.uint8 or background.dim() != 4 \
                or background.shape[0] not in (1, b) or tuple(background.shape[1:]) != (Ho, Wo, 3):
            raise RuntimeError("background must be a uint8 [b or 1, Ho, Wo, 3] tensor")
    if dtype not in _OUT_KIND:
        raise RuntimeError("dtype must be float32 or float16")
    fill3, mean3, std3 = _triple(fill, "fill"), _triple(mean, "mean"), _triple(std, "std")
    if any(not 0.0 <= f <= 255.0 for f in fill3):
        raise RuntimeError("fill must be in 0..255")
    if any(not s > 0.0 for s in std3):
        raise RuntimeError("std must be positive")
    steps = (steps,) if isinstance(steps, str) else tuple(steps)
    if any(s not in _STEPS for s in steps):
        raise RuntimeError(f"steps must be among {ALL_STEPS}")
    flags = 0
    for s in steps:
        flags |= _STEPS[s]
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out) \
                or tuple(out[0].shape) != (b, 3, Ho, Wo) or out[0].dtype != dtype \
                or tuple(out[1].shape) != (b, Ho, Wo) or out[1].dtype != label.dtype:
            raise RuntimeError(f"out must be (image {dtype} [b, 3, Ho, Wo], label {label.dtype} [b, Ho, Wo])")
    for t, name in ((image, "image"), (label, "label"), (background, "background")):
        if t is not None and sum((n - 1) * st for n, st in zip(t.shape[1:], t.stride()[1:])) > 2 ** 31 - 1:
            raise RuntimeError(f"one image of {name} must span at most 2^31 - 1 elements")
    dev = _need_device(image, "image")
    for t, name in ((label, "label"), (inv, "params"), (color, "params"), (background, "background"),
                    *(((out[0], "out"), (out[1], "out")) if out is not None else ())):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} must be on the image's device")
    if out is None:
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        out_image = torch.empty((b, 3, Ho, Wo), dtype=dtype, device=dev, memory_format=fmt)
        out_label = torch.empty((b, Ho, Wo), dtype=label.dtype, device=dev)
    else:
        out_image, out_label = out
    if b == 0:
        return out_image, out_label
    inv, color = inv.contiguous(), color.contiguous()
    d = _A.AugDesc()
    d.image, d.label, d.inv, d.color = image.data_ptr(), label.data_ptr(), inv.data_ptr(), color.data_ptr()
    d.background = None if background is None else background.data_ptr()
    d.out_image, d.out_label = out_image.data_ptr(), out_label.data_ptr()
    for i in range(4):
        d.image_strides[i] = image.stride(i)
        d.out_image_strides[i] = out_image.stride(i)
        if background is not None:
            d.background_strides[i] = background.stride(i) if (i or background.shape[0] == b) else 0
    for i in range(3):
        d.label_strides[i] = label.stride(i)
        d.out_label_strides[i] = out_label.stride(i)
        d.fill[i], d.mean[i], d.std[i] = fill3[i], mean3[i], std3[i]
    d.label_kind, d.out_kind, d.flags = _LABEL_KIND[label.dtype], _OUT_KIND[dtype], flags
    d.b, d.H, d.W, d.Ho, d.Wo = b, H, W, Ho, Wo
    L = _A.load()
    ws_ptr, ws_bytes = None, 0
    if flags & _A.PV_AUG_CONTRAST:
        ws = _ws.get(dev, int(L.pv_augment_workspace_size(b, Ho, Wo)))
        ws_ptr, ws_bytes = ws.data_ptr(), ws.numel()
    with torch.cuda.device(dev):
        _A.check(L.pv_augment_apply(ctypes.byref(d), ws_ptr, ws_bytes, _stream(dev)), "pv_augment_apply")
    return out_image, out_label


def transform_keypoints(keypoints_2d: torch.Tensor, fwd: torch.Tensor) -> torch.Tensor:
    """keypoints_2d [b, ..., 2], fwd f64 [b, 2, 3] -> f64 [b, ..., 2]: fwd (x, y, 1), in float64 on
    the tensors' device (x right, y down)."""
    if not isinstance(keypoints_2d, torch.Tensor) or keypoints_2d.dim() < 2 or keypoints_2d.shape[-1] != 2:
        raise RuntimeError("keypoints_2d must be a [b, ..., 2] tensor")
    if not isinstance(fwd, torch.Tensor) or fwd.dim() != 3 or tuple(fwd.shape) != (keypoints_2d.shape[0], 2, 3):
        raise RuntimeError("fwd must be [b, 2, 3]")
    if keypoints_2d.device != fwd.device:
        raise RuntimeError("keypoints_2d and fwd must be on the same device")
    kp = keypoints_2d.to(torch.float64)
    M = fwd.to(torch.float64).reshape(fwd.shape[0], *([1] * (kp.dim() - 2)), 2, 3)
    x, y = kp[..., 0], kp[..., 1]
    return torch.stack([(M[..., 0, 0] * x + M[..., 0, 1] * y) + M[..., 0, 2],
                        (M[..., 1, 0] * x + M[..., 1, 1] * y) + M[..., 1, 2]], -1)


def augment_ground_truth(image: torch.Tensor, label: torch.Tensor, keypoints_2d: torch.Tensor, class_num: int,
                         state: torch.Tensor, out_size=None, background: torch.Tensor | None = None,
                         rot_deg=(-30.0, 30.0), scale=(0.8, 1.2), margin: float = 0.25,
                         jitter=(0.1, 0.1, 0.05, 0.05), fill=0, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                         dtype=torch.float32, vertex_dtype=torch.float32, layout: str = "network",
                         steps=ALL_STEPS, channels_last: bool = False):
    """One augmented training batch from a decoded one, with no host round trip.

    image         uint8 [b, H, W, 3]; label [b, H, W]; keypoints_2d [b, class_num, vn, 2]
    state         device int64 [2] = (seed, first sample index); advance state[1] by b per call
    layout        of the vector field, as ``render.vertex_field`` takes it ("network": what
                  ``pvnet_loss`` compares the network's output with; "bhwk2": what the voting layers take)

    Returns ``(image [b, 3, Ho, Wo], label [b, Ho, Wo], vertex, keypoints_2d f64 [b, class_num, vn, 2])``:
    the vector field is ``render.vertex_field`` of the augmented label and the transformed keypoints."""
    from . import render
    b, H, W = _check_label(label)
    class_num = _check_class_num(class_num)
    if not isinstance(keypoints_2d, torch.Tensor) or keypoints_2d.dim() != 4 or \
            tuple(keypoints_2d.shape[:2]) != (b, class_num) or keypoints_2d.shape[3] != 2 or keypoints_2d.shape[2] < 1:
        raise RuntimeError(f"keypoints_2d must be [b, class_num, vn, 2] = [{b}, {class_num}, vn, 2]")
    Ho, Wo = _check_out_size(out_size, (H, W))
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or tuple(image.shape) != (b, H, W, 3):
        raise RuntimeError(f"image must be a uint8 [b, H, W, 3] tensor matching the label's [{b}, {H}, {W}]")
    # the devices before the first launch: random_params would otherwise have run when apply rejects
    dev = _need_device(image, "image")
    if label.device != dev or keypoints_2d.device != dev:
        raise RuntimeError("label and keypoints_2d must be on the image's device")
    params = random_params(label, class_num, (Ho, Wo), state, rot_deg, scale, margin, jitter)
    img, lab = apply(image, label, params, background, fill, mean, std, dtype, (Ho, Wo), None, steps, channels_last)
    kp = transform_keypoints(keypoints_2d, params.fwd)
    vertex = render.vertex_field(lab, kp, class_num, dtype=vertex_dtype, layout=layout)
    return img, lab, vertex, kp
