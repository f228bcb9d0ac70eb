#!/usr/bin/env python3
"""Time the training augmentation (include/pvaugment.h, pvnet_amd/augment.py): the draw of the parameters,
the apply call, and the whole ``augment_ground_truth``.

Shape: 32 x 480 x 640 u8 frames (random pixels, the disk masks and keypoints of ``synth.synthetic_batch``,
one object, vn = 9) to 480 x 640 fp16 with one background per image, every photometric step on.

Each call is captured into a hipGraph and replayed between two device events, enough replays per window
to fill --window seconds; the median of --rounds windows is reported.  The baseline is the same result
composed from torch ops on the same device and captured the same way: the statistics with tensor
reductions and the draws with ``torch.rand``; ``F.affine_grid`` + ``F.grid_sample`` (bilinear for the
image, nearest for the label map), the background by ``torch.where``, the jitter written with tensor ops in
the same fixed order, and the normalisation; for the whole chain the same ``render.vertex_field`` on both
sides.  The baseline's draws are torch's, so its parameters differ; for the agreement check it is run
once more on the device call's own matrices.

The compulsory bytes are computed from the shapes: image, label map and background read once, image and
label map written once (and the vector field written once, the augmented label read once more, for the
whole chain).  Needs the GPU; there is no fallback.

    python tools/augment_probe.py [--rounds 5] [--window 0.3] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pvnet_amd import augment as AU  # noqa: E402
from pvnet_amd import render as RN  # noqa: E402
from pvnet_amd import synth  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, the part's specification
B, H, W, VN = 32, 480, 640, 9
ROT, SCALE, MARGIN, JITTER = (-30.0, 30.0), (0.8, 1.2), 0.25, (0.1, 0.1, 0.05, 0.05)


def timed(fn, stream, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps               # ms per call


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))


def graph_time(fn, stream, window, rounds):
    """Capture fn, replay it in windows of `window` seconds -> (ms per call over the rounds, replays per window,
    what the captured call returned)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        fn()                                         # warm-up: workspace, code objects
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            res = fn()
    t1 = timed(g.replay, stream, 2)
    reps = max(2, int(math.ceil(window * 1e3 / t1)))
    return [timed(g.replay, stream, reps) for _ in range(rounds)], reps, res


# ---- the composition from torch ops ------------------------------------------------------------------------
def torch_params(label, ncls, k):
    """-> (fwd, inv f64 [b, 2, 3], color f32 [b, 4]) with torch's own draws."""
    b, h, w = label.shape
    fg = ((label >= 1) & (label <= ncls)).to(torch.float64)
    cnt = fg.sum((1, 2))
    xs = torch.arange(w, device=label.device, dtype=torch.float64)
    ys = torch.arange(h, device=label.device, dtype=torch.float64)
    has = cnt > 0
    safe = torch.where(has, cnt, torch.ones_like(cnt))
    cx = torch.where(has, (fg.sum(1) * xs).sum(1) / safe, torch.full_like(cnt, (w - 1) / 2))
    cy = torch.where(has, (fg.sum(2) * ys).sum(1) / safe, torch.full_like(cnt, (h - 1) / 2))
    u = torch.rand((b, 8), device=label.device, dtype=torch.float64)         # the default generator: capturable
    theta = (ROT[0] + u[:, 0] * (ROT[1] - ROT[0])) * (math.pi / 180.0)
    s = SCALE[0] + u[:, 1] * (SCALE[1] - SCALE[0])
    tx = (MARGIN + u[:, 2] * (1 - 2 * MARGIN)) * (w - 1)
    ty = (MARGIN + u[:, 3] * (1 - 2 * MARGIN)) * (h - 1)
    a, q = s * torch.cos(theta), s * torch.sin(theta)
    f02, f12 = tx - (a * cx - q * cy), ty - (q * cx + a * cy)
    fwd = torch.stack([torch.stack([a, -q, f02], 1), torch.stack([q, a, f12], 1)], 1)
    d = a * a + q * q
    ia, iq = a / d, q / d
    inv = torch.stack([torch.stack([ia, iq, -(ia * f02 + iq * f12)], 1), torch.stack([-iq, ia, iq * f02 - ia * f12], 1)], 1)
    color = (k["one"] + k["jitter"] * (2 * u[:, 4:] - 1)).float()
    return fwd, inv, color


def _grey(c):
    return (0.299 * c[:, 0] + 0.587 * c[:, 1] + 0.114 * c[:, 2])[:, None]


def _hue(c, eta):
    r, g, b = c.unbind(1)
    maxc, minc = c.max(1).values, c.min(1).values
    rng = maxc - minc
    flat = rng == 0
    safe = torch.where(flat, torch.ones_like(rng), rng)
    s = rng / torch.where(maxc == 0, torch.ones_like(maxc), maxc)
    rc, gc, bc = (maxc - r) / safe, (maxc - g) / safe, (maxc - b) / safe
    h = torch.where(r == maxc, bc - gc, torch.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc)) / 6.0
    h = h - torch.floor(h) + eta[:, None, None]
    h = h - torch.floor(h)
    h6 = h * 6.0
    fi = torch.floor(h6)
    f = h6 - fi
    v = maxc
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    sec = fi.long() % 6
    rr = torch.stack([v, q, p, p, t, v], 0).gather(0, sec[None])[0]
    gg = torch.stack([t, v, v, q, p, p], 0).gather(0, sec[None])[0]
    bb = torch.stack([p, p, t, v, v, q], 0).gather(0, sec[None])[0]
    return torch.stack([rr, gg, bb], 1)


def torch_apply(image_chw, label, inv, color, background_chw, k):
    """image_chw u8 [b, 3, H, W], background_chw u8 [b, 3, H, W] -> (f16 [b, 3, H, W], label)."""
    b, _, h, w = image_chw.shape
    theta = (k["n_in"] @ torch.cat([inv, k["row"].expand(b, 1, 3)], 1) @ k["n_out_inv"])[:, :2].float()
    grid = F.affine_grid(theta, (b, 3, h, w), align_corners=True)
    c = F.grid_sample(image_chw.float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    lab = F.grid_sample(label[:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=True)[:, 0]
    lab = lab.to(label.dtype)
    c = torch.where((lab == 0)[:, None], background_chw.float(), c) * (1.0 / 255.0)
    beta, kappa, sigma, eta = (color[:, k][:, None, None, None] for k in range(4))
    c = (beta * c).clamp(0, 1)
    m = _grey(c).mean((1, 2, 3), keepdim=True)
    c = (kappa * c + (1 - kappa) * m).clamp(0, 1)
    c = (sigma * c + (1 - sigma) * _grey(c)).clamp(0, 1)
    c = _hue(c, color[:, 3])
    return ((c - k["mean"]) * k["rstd"]).half(), lab


def constants(dev, h, w):
    """What the composition needs on the device, made outside the captured region."""
    f64 = dict(device=dev, dtype=torch.float64)
    # pixel coordinates -> the normalised ones of align_corners=True: theta = n_in inv n_out_inv
    return dict(n_in=torch.tensor([[2.0 / (w - 1), 0, -1], [0, 2.0 / (h - 1), -1], [0, 0, 1]], **f64),
                n_out_inv=torch.tensor([[(w - 1) / 2.0, 0, (w - 1) / 2.0], [0, (h - 1) / 2.0, (h - 1) / 2.0], [0, 0, 1]], **f64),
                row=torch.tensor([[[0.0, 0.0, 1.0]]], **f64), jitter=torch.tensor(JITTER, **f64),
                one=torch.tensor([1.0, 1.0, 1.0, 0.0], **f64),
                mean=torch.tensor(AU.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1),
                rstd=1.0 / torch.tensor(AU.IMAGENET_STD, device=dev).view(1, 3, 1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("augment_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    f = synth.synthetic_batch(B, dtype=np.float16)
    label = torch.from_numpy(f["mask"].astype(np.uint8)).to(dev)
    kp = torch.from_numpy(f["keypoints"][:, None]).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    image = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    background = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    image_chw = image.permute(0, 3, 1, 2).contiguous()
    background_chw = background.permute(0, 3, 1, 2).contiguous()
    state = torch.tensor([2024, 0], dtype=torch.int64, device=dev)
    k = constants(dev, H, W)
    prm = AU.random_params(label, 1, (H, W), state, ROT, SCALE, MARGIN, JITTER)

    px = B * H * W
    apply_bytes = px * 3 + px + px * 3 + px * 3 * 2 + px                  # image, label, background in; f16 image, label out
    params_bytes = px                                                      # the label map once
    whole_bytes = params_bytes + apply_bytes + px + px * 2 * VN * 4        # + the label again, the f32 field out
    rec = dict(device=torch.cuda.get_device_name(dev), b=B, H=H, W=W, vn=VN, out_dtype="float16", rounds=a.rounds,
               window_s=a.window, hbm_peak_bytes_per_s=HBM_PEAK,
               compulsory_bytes=dict(params=params_bytes, apply=apply_bytes, augment_ground_truth=whole_bytes))

    def dev_params():
        return AU.random_params(label, 1, (H, W), state, ROT, SCALE, MARGIN, JITTER)

    def dev_apply():
        return AU.apply(image, label, prm, background=background, dtype=torch.float16)

    def dev_whole():
        return AU.augment_ground_truth(image, label, kp, 1, state, background=background, rot_deg=ROT, scale=SCALE,
                                       margin=MARGIN, jitter=JITTER, dtype=torch.float16)

    def t_params():
        return torch_params(label, 1, k)

    def t_apply():
        return torch_apply(image_chw, label, prm.inv, prm.color, background_chw, k)

    def t_whole():
        fwd, inv, color = torch_params(label, 1, k)
        img, lab = torch_apply(image_chw, label, inv, color, background_chw, k)
        k2 = AU.transform_keypoints(kp, fwd)
        return img, lab, RN.vertex_field(lab, k2, 1, layout="network"), k2

    res = {}
    for key, fn, nbytes in (("params", dev_params, params_bytes), ("apply", dev_apply, apply_bytes),
                            ("augment_ground_truth", dev_whole, whole_bytes), ("params_torch", t_params, None),
                            ("apply_torch", t_apply, None), ("augment_ground_truth_torch", t_whole, None)):
        ts, reps, res[key] = graph_time(fn, stream, a.window, a.rounds)
        rec[key] = dict(ms_per_call=stats(ts), replays_per_window=reps)
        if nbytes is not None:
            rate = nbytes / (rec[key]["ms_per_call"]["median"] * 1e-3)
            rec[key].update(compulsory_bytes_per_s=rate, fraction_of_hbm_peak=rate / HBM_PEAK)
        print(key, json.dumps(rec[key]), flush=True)
    for key in ("params", "apply", "augment_ground_truth"):
        rec[key + "_torch_over_device"] = rec[key + "_torch"]["ms_per_call"]["median"] / rec[key]["ms_per_call"]["median"]
    # the two apply calls ran on the same matrices: the labels agree except where torch's normalised grid
    # rounds a tie the other way, the images to the f16 output's resolution
    torch.cuda.synchronize()
    d_img, d_lab = res["apply"]
    t_img, t_lab = res["apply_torch"]
    rec["apply_label_mismatch_fraction_from_torch"] = float((d_lab != t_lab).float().mean())
    same = (d_lab == t_lab)[:, None].expand_as(d_img)
    diff = (d_img.float() - t_img.float()).abs()[same]
    rec["apply_image_difference_from_torch"] = dict(max=float(diff.max()), mean=float(diff.mean()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
