"""Multi-object training frames composed on the device (include/pvcompose.h): the reference's "fuse"
synthesis, random erasing, Gaussian blur and additive noise, from a bank of single-object frames to a
batch of u8 frames with a label map.

* :func:`make_picks` says which bank frame goes into which slot of which output frame, as which class.
* :func:`random_placement` draws one integer shift per slot, erasers inside the objects' boxes and one
  blur size and noise amplitude per frame -> :class:`Placement`.
* :func:`compose` pastes the slots over a background, later slots over earlier ones, applies the
  erasers and counts each slot's visible pixels.
* :func:`finish` blurs and adds noise.
* :func:`shift_keypoints`, :func:`shift_camera` and :func:`visible_fraction` carry the ground truth along.
* :func:`compose_ground_truth` chains them and ``render.vertex_field``: its image, label map and
  keypoints are what ``augment.augment_ground_truth`` takes, its label map and field what ``pvnet_loss``
  and the multi-object voting take.

It is not a replay of the reference's random stream, only of its family of operations.  Flips and file
reading are not here.  Nothing is read back and nothing synchronises, so a call can be captured into a
graph; the draws depend on a device ``state`` = (seed, first sample index) that the caller advances, and
their draw numbers are disjoint from the augmentation's, so one state drives both.  No CPU fallback:
without libpvcompose.so or a ROCm device the calls raise.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from . import _compose_lib as _C

_LABEL_KIND = {torch.int64: _C.PV_CMP_LABEL_I64, torch.uint8: _C.PV_CMP_LABEL_U8, torch.int32: _C.PV_CMP_LABEL_I32}
_STATE_DTYPES = (torch.int64,) + ((torch.uint64,) if hasattr(torch, "uint64") else ())
_MAX = _C.PV_CMP_MAX_DIM


class Placement(NamedTuple):
    """shift i32 [b, S, 2] = (dx, dy) per slot; erase i32 [b, E, 4] = inclusive boxes in output
    coordinates; ksel i32 [b]: the blur is (2 ksel + 1) wide; amp f32 [b]: the noise amplitude."""
    shift: torch.Tensor
    erase: torch.Tensor
    ksel: torch.Tensor
    amp: torch.Tensor


def blur_kernels():
    """f32 [5][5]: row j holds the half-kernel of the (2 j + 1)-tap Gaussian with cv2's sigma for
    sigma = 0, 0.3 ((k - 1) / 2 - 1) + 0.8, normalised in f64; entries past t = j are 0."""
    rows = []
    for j in range(5):
        sigma = 0.3 * (j - 1) + 0.8
        g = [math.exp(-(t * t) / (2.0 * sigma * sigma)) for t in range(-j, j + 1)]
        total = math.fsum(g)
        rows.append([g[j + t] / total if t <= j else 0.0 for t in range(5)])
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


_KERNELS = None


def _kernels():
    global _KERNELS
    if _KERNELS is None:
        _KERNELS = blur_kernels().tolist()
    return _KERNELS


def _need_device(t, name):
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be a device tensor (no CPU path)")
    return t.device


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _check_size(size, name):
    try:
        h, w = (int(s) for s in size)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name} must be two integers") from None
    if not (1 <= h <= _MAX and 1 <= w <= _MAX):
        raise RuntimeError(f"{name} must be two integers in 1..2^15")
    return h, w


def _check_class_num(class_num):
    class_num = int(class_num)
    if not 1 <= class_num <= _C.PV_CMP_MAX_CLASSES:
        raise RuntimeError(f"class_num must be in 1..{_C.PV_CMP_MAX_CLASSES}")
    return class_num


def _check_pick(pick):
    if not isinstance(pick, torch.Tensor) or pick.dim() != 3 or pick.shape[2] != 8 or pick.dtype != torch.int32 \
            or not 1 <= pick.shape[1] <= _C.PV_CMP_MAX_SLOTS:
        raise RuntimeError(f"pick must be an int32 [b, S, 8] tensor with S in 1..{_C.PV_CMP_MAX_SLOTS}")
    return int(pick.shape[0]), int(pick.shape[1])


def _check_shift(shift, b, S):
    if not isinstance(shift, torch.Tensor) or shift.dtype != torch.int32 or tuple(shift.shape) != (b, S, 2):
        raise RuntimeError(f"shift must be an int32 [b, S, 2] = [{b}, {S}, 2] tensor")


def _check_state(state):
    if not isinstance(state, torch.Tensor) or state.dtype not in _STATE_DTYPES or tuple(state.shape) != (2,) \
            or not state.is_contiguous():
        raise RuntimeError("state must be a contiguous int64 [2] tensor = (seed, first sample index)")


def _pair(v, name):
    try:
        t = tuple(float(x) for x in v)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name} must be 2 numbers") from None
    if len(t) != 2 or any(not math.isfinite(x) for x in t):
        raise RuntimeError(f"{name} must be 2 finite numbers")
    return t


def _frame_span(t):
    return sum((n - 1) * st for n, st in zip(t.shape[1:], t.stride()[1:]))


def make_picks(src: torch.Tensor, cls: torch.Tensor, bank_stats: torch.Tensor | None = None, src_label=1) -> torch.Tensor:
    """-> pick int32 [b, S, 8] = (src, src_label, cls, x0, y0, x1, y1, 0).  Plain torch, on ``src``'s device.

    src         integer [b, S]: the bank frame of each slot; a value outside the bank makes the slot dead
    cls         integer [b, S] (or broadcastable to it): the class the slot's pixels get, 1..class_num
    bank_stats  optional int64 [N, 8], ``augment.label_stats`` of the bank's label map: the box is its
                columns 3:7 (an empty box for a frame without foreground); without it the full frame
    src_label   the bank label that marks the object: a number, or integer [b, S]"""
    if not isinstance(src, torch.Tensor) or src.dim() != 2 or src.dtype.is_floating_point or src.dtype == torch.bool \
            or not 1 <= src.shape[1] <= _C.PV_CMP_MAX_SLOTS:
        raise RuntimeError(f"src must be an integer [b, S] tensor with S in 1..{_C.PV_CMP_MAX_SLOTS}")
    dev = src.device
    src = src.to(torch.int64)
    try:
        cls = torch.as_tensor(cls, device=dev).to(torch.int64).expand(src.shape)
        lab = torch.as_tensor(src_label, device=dev).to(torch.int64).expand(src.shape)
    except (RuntimeError, TypeError, ValueError):
        raise RuntimeError("cls and src_label must be integers broadcastable to src's [b, S]") from None
    if bank_stats is None:
        box = torch.tensor([0, 0, _MAX - 1, _MAX - 1], dtype=torch.int64, device=dev).expand(*src.shape, 4)
    else:
        if not isinstance(bank_stats, torch.Tensor) or bank_stats.dim() != 2 or bank_stats.shape[1] != 8 \
                or bank_stats.dtype != torch.int64 or bank_stats.shape[0] < 1 or bank_stats.device != dev:
            raise RuntimeError("bank_stats must be an int64 [N, 8] tensor on src's device")
        box = bank_stats[src.clamp(0, bank_stats.shape[0] - 1)][..., 3:7]
    zero = torch.zeros_like(src)
    return torch.cat([torch.stack([src, lab, cls], -1), box, zero[..., None]], -1).to(torch.int32)


def random_placement(pick: torch.Tensor, bank_size, out_size, state: torch.Tensor, margin: float = 0.25, erasers: int = 0,
                     erase_frac=(0.1, 0.4), blur_p: float = 0.5, noise=(0.0, 8.0),
                     class_num: int = _C.PV_CMP_MAX_CLASSES) -> Placement:
    """One shift per slot, ``erasers`` erasers and one blur size and noise amplitude per frame.

    pick        int32 [b, S, 8] (:func:`make_picks`)
    bank_size   (N, H, W) of the bank; out_size: (Ho, Wo) of the composed frame
    state       device int64 (or uint64) [2] = (seed, first sample index), read and never written: frame f
                uses sample index state[1] + f, so advance state[1] by b between calls
    margin      in [0, 0.5]: a box's centre lands uniformly in [margin, 1 - margin] of the output frame
    erasers     E in 0..8; eraser e lies inside the shifted box of slot e mod S and covers
                ``erase_frac`` = (lo, hi) of its width and height
    blur_p      the probability of a blur (3, 5, 7 or 9 taps with equal probability)
    noise       (lo, hi) of the noise amplitude in grey levels (the noise's standard deviation is 0.577 of it)
    class_num   slots whose class is outside 1..class_num are dead, as in :func:`compose`

    The draws are include/pvcompose.h's; numpy reproduces them bit for bit."""
    b, S = _check_pick(pick)
    try:
        N, H, W = (int(v) for v in bank_size)
    except (TypeError, ValueError):
        raise RuntimeError("bank_size must be (N, H, W)") from None
    if N < 1 or not (1 <= H <= _MAX and 1 <= W <= _MAX):
        raise RuntimeError("bank_size must be (N, H, W) with N >= 1 and H, W in 1..2^15")
    Ho, Wo = _check_size(out_size, "out_size")
    _check_state(state)
    class_num = _check_class_num(class_num)
    margin, blur_p, E = float(margin), float(blur_p), int(erasers)
    frac, nz = _pair(erase_frac, "erase_frac"), _pair(noise, "noise")
    if not 0.0 <= margin <= 0.5:
        raise RuntimeError("margin must be in [0, 0.5]")
    if not 0 <= E <= _C.PV_CMP_MAX_ERASE:
        raise RuntimeError(f"erasers must be in 0..{_C.PV_CMP_MAX_ERASE}")
    if not 0.0 < frac[0] <= frac[1] <= 1.0:
        raise RuntimeError("erase_frac must be (lo, hi) with 0 < lo <= hi <= 1")
    if not 0.0 <= blur_p <= 1.0:
        raise RuntimeError("blur_p must be in [0, 1]")
    if not 0.0 <= nz[0] <= nz[1]:
        raise RuntimeError("noise must be (lo, hi) with 0 <= lo <= hi")
    dev = _need_device(pick, "pick")
    if state.device != dev:
        raise RuntimeError("state must be on pick's device")
    pick = pick.contiguous()
    shift = torch.empty((b, S, 2), dtype=torch.int32, device=dev)
    erase = torch.empty((b, E, 4), dtype=torch.int32, device=dev)
    ksel = torch.empty((b,), dtype=torch.int32, device=dev)
    amp = torch.empty((b,), dtype=torch.float32, device=dev)
    if b:
        r = _C.CmpRanges(margin, (ctypes.c_double * 2)(*frac), blur_p, (ctypes.c_double * 2)(*nz),
                         b, N, H, W, Ho, Wo, S, E, class_num, 0)
        with torch.cuda.device(dev):
            _C.check(_C.load().pv_compose_params(ctypes.byref(r), pick.data_ptr(), state.data_ptr(), shift.data_ptr(),
                                                 erase.data_ptr() if E else None, ksel.data_ptr(), amp.data_ptr(),
                                                 _stream(dev)), "pv_compose_params")
    return Placement(shift, erase, ksel, amp)


def compose(bank_image: torch.Tensor, bank_label: torch.Tensor, pick: torch.Tensor, shift: torch.Tensor, class_num: int,
            out_size, background: torch.Tensor | None = None, fill=0, erase: torch.Tensor | None = None,
            want_instance: bool = False, out=None):
    """Paste the picked objects into b frames.

    bank_image  uint8 [N, H, W, 3] device tensor, any strides (a [N, 3, H, W] tensor permuted is fine)
    bank_label  uint8 / int32 / int64 [N, H, W], any strides
    pick, shift int32 [b, S, 8] and [b, S, 2]
    background  optional uint8 [b, Ho, Wo, 3] or [1, Ho, Wo, 3] (shared), else ``fill``: a number or three, 0..255
    erase       optional int32 [b, E, 4], E <= 8
    out         optional ``(image, label)`` to write into: uint8 [b, Ho, Wo, 3] and [b, Ho, Wo] of the bank
                label's dtype, any strides

    Returns ``(image uint8 [b, Ho, Wo, 3], label [b, Ho, Wo], instance or None, visible int32 [b, S])``:
    instance is s + 1 where slot s shows, visible[f, s] the number of such pixels.  The semantics are
    include/pvcompose.h's."""
    if not isinstance(bank_image, torch.Tensor) or bank_image.dim() != 4 or bank_image.shape[3] != 3 \
            or bank_image.dtype != torch.uint8:
        raise RuntimeError("bank_image must be a uint8 [N, H, W, 3] tensor")
    if not isinstance(bank_label, torch.Tensor) or bank_label.dim() != 3 or bank_label.dtype not in _LABEL_KIND:
        raise RuntimeError("bank_label must be a uint8 / int32 / int64 [N, H, W] tensor")
    N, H, W = (int(s) for s in bank_label.shape)
    if tuple(bank_image.shape[:3]) != (N, H, W) or N < 1 or not (1 <= H <= _MAX and 1 <= W <= _MAX):
        raise RuntimeError("bank_image must be a uint8 [N, H, W, 3] tensor matching bank_label, N >= 1 and H, W in 1..2^15")
    b, S = _check_pick(pick)
    _check_shift(shift, b, S)
    class_num = _check_class_num(class_num)
    if bank_label.dtype == torch.uint8 and class_num > 255:
        raise RuntimeError("class_num must be at most 255 with uint8 labels")
    Ho, Wo = _check_size(out_size, "out_size")
    if background is not None:
        if not isinstance(background, torch.Tensor) or background.dtype != torch.uint8 or background.dim() != 4 \
                or background.shape[0] not in (1, b) or tuple(background.shape[1:]) != (Ho, Wo, 3):
            raise RuntimeError("background must be a uint8 [b or 1, Ho, Wo, 3] tensor")
    fill3 = (fill,) * 3 if isinstance(fill, (int, float)) else tuple(fill)
    if len(fill3) != 3 or any(not isinstance(v, (int, float)) or v != int(v) or not 0 <= v <= 255 for v in fill3):
        raise RuntimeError("fill must be an integer in 0..255, or three")
    E = 0
    if erase is not None:
        if not isinstance(erase, torch.Tensor) or erase.dtype != torch.int32 or erase.dim() != 3 or erase.shape[0] != b \
                or erase.shape[2] != 4 or erase.shape[1] > _C.PV_CMP_MAX_ERASE:
            raise RuntimeError(f"erase must be an int32 [b, E, 4] tensor with E <= {_C.PV_CMP_MAX_ERASE}")
        E = int(erase.shape[1])
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out) \
                or tuple(out[0].shape) != (b, Ho, Wo, 3) or out[0].dtype != torch.uint8 \
                or tuple(out[1].shape) != (b, Ho, Wo) or out[1].dtype != bank_label.dtype:
            raise RuntimeError(f"out must be (image uint8 [b, Ho, Wo, 3], label {bank_label.dtype} [b, Ho, Wo])")
    for t, name in ((bank_image, "bank_image"), (bank_label, "bank_label"), (background, "background"),
                    *(((out[0], "out"), (out[1], "out")) if out is not None else ())):
        if t is not None and _frame_span(t) > 2 ** 31 - 1:
            raise RuntimeError(f"one frame of {name} must span at most 2^31 - 1 elements")
    dev = _need_device(bank_image, "bank_image")
    for t, name in ((bank_label, "bank_label"), (pick, "pick"), (shift, "shift"), (background, "background"), (erase, "erase"),
                    *(((out[0], "out"), (out[1], "out")) if out is not None else ())):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} must be on bank_image's device")
    if out is None:
        out_image = torch.empty((b, Ho, Wo, 3), dtype=torch.uint8, device=dev)
        out_label = torch.empty((b, Ho, Wo), dtype=bank_label.dtype, device=dev)
    else:
        out_image, out_label = out
    instance = torch.empty((b, Ho, Wo), dtype=bank_label.dtype, device=dev) if want_instance else None
    visible = torch.empty((b, S), dtype=torch.int32, device=dev)
    if b == 0:
        return out_image, out_label, instance, visible
    pick, shift = pick.contiguous(), shift.contiguous()
    d = _C.CmpDesc()
    d.image, d.label, d.pick, d.shift = bank_image.data_ptr(), bank_label.data_ptr(), pick.data_ptr(), shift.data_ptr()
    d.erase = erase.contiguous().data_ptr() if E else None
    d.background = None if background is None else background.data_ptr()
    d.out_image, d.out_label, d.visible = out_image.data_ptr(), out_label.data_ptr(), visible.data_ptr()
    d.out_instance = None if instance is None else instance.data_ptr()
    for i in range(4):
        d.image_strides[i] = bank_image.stride(i)
        d.out_image_strides[i] = out_image.stride(i)
        if background is not None:
            d.background_strides[i] = background.stride(i) if (i or background.shape[0] == b) else 0
    for i in range(3):
        d.label_strides[i] = bank_label.stride(i)
        d.out_label_strides[i] = out_label.stride(i)
        if instance is not None:
            d.out_instance_strides[i] = instance.stride(i)
        d.fill[i] = int(fill3[i])
    d.label_kind = _LABEL_KIND[bank_label.dtype]
    d.N, d.H, d.W, d.b, d.Ho, d.Wo, d.S, d.E, d.ncls = N, H, W, b, Ho, Wo, S, E, class_num
    with torch.cuda.device(dev):
        _C.check(_C.load().pv_compose_apply(ctypes.byref(d), _stream(dev)), "pv_compose_apply")
    return out_image, out_label, instance, visible


def finish(image: torch.Tensor, ksel: torch.Tensor, amp: torch.Tensor, state: torch.Tensor, out: torch.Tensor | None = None):
    """Blur frame f with the (2 ksel[f] + 1)-tap Gaussian (reflect-101 borders) and add amp[f] times the
    noise field of sample state[1] + f.

    image  uint8 [b, H, W, 3] device tensor, any strides; ksel int32 [b] (0..4, anything else is 0);
    amp float32 [b]; state as :func:`random_placement` takes it; out: optional uint8 [b, H, W, 3] that is
    not ``image``.  Returns the finished uint8 [b, H, W, 3]; ksel = 0 and amp = 0 copy the frame."""
    if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[3] != 3 or image.dtype != torch.uint8:
        raise RuntimeError("image must be a uint8 [b, H, W, 3] tensor")
    b = int(image.shape[0])
    H, W = _check_size(image.shape[1:3], "image's H and W")
    if not isinstance(ksel, torch.Tensor) or ksel.dtype != torch.int32 or tuple(ksel.shape) != (b,):
        raise RuntimeError("ksel must be an int32 [b] tensor")
    if not isinstance(amp, torch.Tensor) or amp.dtype != torch.float32 or tuple(amp.shape) != (b,):
        raise RuntimeError("amp must be a float32 [b] tensor")
    _check_state(state)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (b, H, W, 3):
            raise RuntimeError("out must be a uint8 [b, H, W, 3] tensor")
        if out.data_ptr() == image.data_ptr() and b:
            raise RuntimeError("out must not alias image")
    for t, name in ((image, "image"), (out, "out")):
        if t is not None and _frame_span(t) > 2 ** 31 - 1:
            raise RuntimeError(f"one frame of {name} must span at most 2^31 - 1 elements")
    dev = _need_device(image, "image")
    for t, name in ((ksel, "ksel"), (amp, "amp"), (state, "state"), (out, "out")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} must be on image's device")
    if out is None:
        out = torch.empty((b, H, W, 3), dtype=torch.uint8, device=dev)
    if b == 0:
        return out
    ksel, amp = ksel.contiguous(), amp.contiguous()
    d = _C.CmpFinish()
    d.image, d.out, d.ksel, d.amp, d.state = image.data_ptr(), out.data_ptr(), ksel.data_ptr(), amp.data_ptr(), state.data_ptr()
    for i in range(4):
        d.image_strides[i] = image.stride(i)
        d.out_strides[i] = out.stride(i)
    for j, row in enumerate(_kernels()):
        for t, v in enumerate(row):
            d.w[j][t] = v
    d.b, d.H, d.W = b, H, W
    with torch.cuda.device(dev):
        _C.check(_C.load().pv_compose_finish(ctypes.byref(d), _stream(dev)), "pv_compose_finish")
    return out


def _live(pick, bank_size, class_num):
    return (pick[..., 0] >= 0) & (pick[..., 0] < bank_size) & (pick[..., 2] >= 1) & (pick[..., 2] <= class_num)


def shift_keypoints(bank_keypoints: torch.Tensor, pick: torch.Tensor, shift: torch.Tensor, class_num: int):
    """bank_keypoints [N, vn, 2] (the keypoints of each bank frame's object) ->
    ``(keypoints f64 [b, class_num, vn, 2], present bool [b, class_num])``: the keypoints of class c in
    frame f are those of the last live slot of that class, moved by its shift (an integer shift is exact
    in float64); a class with no live slot gets 0 and present False.  Plain torch, no synchronisation."""
    if not isinstance(bank_keypoints, torch.Tensor) or bank_keypoints.dim() != 3 or bank_keypoints.shape[2] != 2 \
            or bank_keypoints.shape[0] < 1:
        raise RuntimeError("bank_keypoints must be a [N, vn, 2] tensor")
    b, S = _check_pick(pick)
    _check_shift(shift, b, S)
    class_num = _check_class_num(class_num)
    if pick.device != bank_keypoints.device or shift.device != bank_keypoints.device:
        raise RuntimeError("bank_keypoints, pick and shift must be on the same device")
    N, vn = int(bank_keypoints.shape[0]), int(bank_keypoints.shape[1])
    kp = bank_keypoints.to(torch.float64)
    live = _live(pick, N, class_num)
    out = torch.zeros((b, class_num, vn, 2), dtype=torch.float64, device=kp.device)
    present = torch.zeros((b, class_num), dtype=torch.bool, device=kp.device)
    classes = torch.arange(1, class_num + 1, device=kp.device)
    for s in range(S):
        moved = kp[pick[:, s, 0].to(torch.int64).clamp(0, N - 1)] + shift[:, s].to(torch.float64)[:, None, :]   # [b, vn, 2]
        hit = live[:, s, None] & (pick[:, s, 2, None] == classes[None])                                          # [b, class_num]
        out = torch.where(hit[:, :, None, None], moved[:, None], out)
        present = present | hit
    return out, present


def shift_camera(K: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """K [3, 3] (or [b, 3, 3]), shift [b, S, 2] -> f64 [b, S, 3, 3]: the camera under which the pose of a
    slot's source frame still holds after the shift, (cx + dx, cy + dy)."""
    if not isinstance(K, torch.Tensor) or K.dim() not in (2, 3) or tuple(K.shape[-2:]) != (3, 3):
        raise RuntimeError("K must be a [3, 3] or [b, 3, 3] tensor")
    if not isinstance(shift, torch.Tensor) or shift.dim() != 3 or shift.shape[2] != 2:
        raise RuntimeError("shift must be a [b, S, 2] tensor")
    b, S = int(shift.shape[0]), int(shift.shape[1])
    if K.dim() == 3 and K.shape[0] != b:
        raise RuntimeError("K must be a [3, 3] or [b, 3, 3] tensor")
    if K.device != shift.device:
        raise RuntimeError("K and shift must be on the same device")
    out = (K.to(torch.float64) if K.dim() == 2 else K.to(torch.float64)[:, None]).expand(b, S, 3, 3).clone()
    out[..., 0, 2] += shift[..., 0].to(torch.float64)
    out[..., 1, 2] += shift[..., 1].to(torch.float64)
    return out


def visible_fraction(visible: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """visible [b, S] (:func:`compose`), counts [b, S] (the objects' pixel counts in their source
    frames, column 0 of ``label_stats`` at pick's src) -> f64 [b, S]; 0 where counts is 0."""
    if not isinstance(visible, torch.Tensor) or not isinstance(counts, torch.Tensor) or visible.dim() != 2 \
            or visible.shape != counts.shape:
        raise RuntimeError("visible and counts must be [b, S] tensors of one shape")
    c = counts.to(torch.float64)
    return torch.where(c > 0, visible.to(torch.float64) / c.clamp(min=1.0), torch.zeros_like(c))


def compose_ground_truth(bank_image: torch.Tensor, bank_label: torch.Tensor, bank_keypoints: torch.Tensor,
                         pick: torch.Tensor, class_num: int, out_size, state: torch.Tensor,
                         background: torch.Tensor | None = None, fill=0, margin: float = 0.25, erasers: int = 0,
                         erase_frac=(0.1, 0.4), blur_p: float = 0.5, noise=(0.0, 8.0), vertex_dtype=torch.float32,
                         layout: str = "network", want_instance: bool = False):
    """One composed training batch from a bank of single-object frames, with no host round trip.

    bank_image uint8 [N, H, W, 3]; bank_label [N, H, W]; bank_keypoints [N, vn, 2]; pick int32 [b, S, 8];
    state device int64 [2] = (seed, first sample index), advance state[1] by b per call; layout: of the
    vector field, as ``render.vertex_field`` takes it.

    Returns a dict: image uint8 [b, Ho, Wo, 3], label [b, Ho, Wo], vertex, keypoints_2d f64
    [b, class_num, vn, 2], present [b, class_num], instance (or None), visible int32 [b, S] and
    placement.  image, label and keypoints_2d are what ``augment.augment_ground_truth`` takes; label and
    vertex what ``pvnet_loss`` and the voting layers take."""
    from . import render
    if not isinstance(bank_label, torch.Tensor) or bank_label.dim() != 3:
        raise RuntimeError("bank_label must be a uint8 / int32 / int64 [N, H, W] tensor")
    N, H, W = (int(s) for s in bank_label.shape)
    b, S = _check_pick(pick)
    class_num = _check_class_num(class_num)
    if not isinstance(bank_keypoints, torch.Tensor) or bank_keypoints.dim() != 3 or bank_keypoints.shape[0] != N \
            or bank_keypoints.shape[2] != 2 or bank_keypoints.shape[1] < 1:
        raise RuntimeError(f"bank_keypoints must be [N, vn, 2] = [{N}, vn, 2]")
    # the devices before the first launch: random_placement would otherwise have run when compose rejects
    dev = _need_device(bank_image, "bank_image")
    if bank_label.device != dev or bank_keypoints.device != dev or pick.device != dev:
        raise RuntimeError("bank_label, bank_keypoints and pick must be on bank_image's device")
    place = random_placement(pick, (N, H, W), out_size, state, margin, erasers, erase_frac, blur_p, noise, class_num)
    image, label, instance, visible = compose(bank_image, bank_label, pick, place.shift, class_num, out_size, background, fill,
                                              place.erase if erasers else None, want_instance)
    image = finish(image, place.ksel, place.amp, state)
    kp, present = shift_keypoints(bank_keypoints, pick, place.shift, class_num)
    vertex = render.vertex_field(label, kp, class_num, dtype=vertex_dtype, layout=layout)
    return dict(image=image, label=label, vertex=vertex, keypoints_2d=kp, present=present, instance=instance,
                visible=visible, placement=place)
