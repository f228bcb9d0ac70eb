#!/usr/bin/env python3
"""Time the training loss (include/pvloss.h, pvnet_amd/net_utils.py): the forward alone, and the forward
with the backward.

Shapes:

  configs2  32 x 480 x 640, fp16, one object, vn = 9: the frames of ``synth.synthetic_batch`` (a disk of
            about 10 % of the pixels, the noisy field as the prediction), the label map and the ground
            truth field from ``render.vertex_field``;
  multi     8 x 480 x 640, fp16, three objects (three disks, about 20 % of the pixels), vn = 9; the
            prediction is the ground truth plus noise over the whole frame.

Everything is in the network's layout.  Each call is captured into a hipGraph and replayed between two
device events, enough replays per window to fill --window seconds; the median of --rounds windows is
reported.  The baseline is the same objective composed from torch ops on the same device as the
reference composes it (F.cross_entropy and its view-mean; the smooth-L1 with the weights multiplied in,
in float32), with its autograd backward, captured and timed the same way; it does not compute the
precision / recall counts, which the device forward includes.

The achieved bytes/s are the compulsory bytes over the time: seg and label once, the foreground pixels'
own channels of vertex and target once, and for the backward the same again plus both gradients written
once.  Needs the GPU; there is no fallback.

    python tools/loss_probe.py [--rounds 5] [--window 0.3] [--out FILE]
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
from pvnet_amd import net_utils as NU  # noqa: E402
from pvnet_amd import render as RN  # noqa: E402
from pvnet_amd import synth  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, the part's specification
H, W, VN = 480, 640, 9


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


def torch_objective(seg, ver, lab, tgt, ncls, vn, sigma=1.0):
    """The reference's composition for the network layout, per image: (loss_seg [b], loss_vertex [b])."""
    b = seg.shape[0]
    lab = lab.long()
    loss_seg = F.cross_entropy(seg.float(), lab, reduction="none").view(b, -1).mean(1)
    cls = torch.arange(2 * ncls * vn, device=seg.device) // (2 * vn) + 1
    w = (lab[:, None] == cls[None, :, None, None]).float()
    sigma2 = sigma * sigma
    d = w * (ver.float() - tgt.float())
    ad = d.abs()
    quad = (ad < 1.0 / sigma2).detach().float()
    in_loss = d * d * (0.5 * sigma2) * quad + (ad - 0.5 / sigma2) * (1.0 - quad)
    fg = ((lab >= 1) & (lab <= ncls)).view(b, -1).sum(1).float()
    return loss_seg, in_loss.view(b, -1).sum(1) / (2 * vn * fg + 1e-3)


def make_configs2(dev, b=32):
    f = synth.synthetic_batch(b, dtype=np.float16)
    label = torch.from_numpy(f["mask"].astype(np.uint8)).to(dev)
    kp = torch.from_numpy(f["keypoints"][:, None]).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    seg = torch.from_numpy(f["seg"]).to(dev)
    seg = (seg.float() * 2 + torch.randn(seg.shape, device=dev, generator=gen)).half()
    return dict(name="configs2", b=b, ncls=1, seg=seg, ver=torch.from_numpy(f["vertex"]).to(dev), label=label,
                tgt=RN.vertex_field(label, kp, 1, dtype=torch.float16, layout="network"))


def make_multi(dev, b=8, ncls=3):
    rng = np.random.default_rng(2)
    lab = np.zeros((b, H, W), np.uint8)
    for i in range(b):
        for c, (cx, r) in enumerate(((110.0, 60.0), (320.0, 97.5), (530.0, 80.0))):
            lab[i][synth.disk_mask(H, W, (cx + rng.uniform(-8, 8), 240.0 + rng.uniform(-60, 60)), r)] = c + 1
    label = torch.from_numpy(lab).to(dev)
    kp = torch.from_numpy(rng.uniform([60.0, 60.0], [580.0, 420.0], (b, ncls, VN, 2))).to(dev)
    tgt = RN.vertex_field(label, kp, ncls, dtype=torch.float16, layout="network")
    gen = torch.Generator(device=dev).manual_seed(3)
    ver = (tgt.float() + 0.1 * torch.randn(tgt.shape, device=dev, generator=gen)).half()
    onehot = F.one_hot(label.long(), ncls + 1).permute(0, 3, 1, 2).float()
    seg = (3 * onehot + torch.randn(onehot.shape, device=dev, generator=gen)).half()
    return dict(name="multi", b=b, ncls=ncls, seg=seg, ver=ver, label=label, tgt=tgt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loss_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("loss_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    rec = dict(device=torch.cuda.get_device_name(dev), H=H, W=W, vn=VN, dtype="float16", rounds=a.rounds,
               window_s=a.window, hbm_peak_bytes_per_s=HBM_PEAK, shapes=[])
    for make in (make_configs2, make_multi):
        s = make(dev)
        b, ncls = s["b"], s["ncls"]
        seg, ver = s["seg"].requires_grad_(), s["ver"].requires_grad_()
        label, tgt = s["label"], s["tgt"]
        fg = int(((label >= 1) & (label <= ncls)).sum())
        es = seg.element_size()
        fwd_bytes = seg.numel() * es + label.numel() * label.element_size() + fg * 2 * VN * (es + tgt.element_size())
        bwd_bytes = fwd_bytes + (seg.numel() + ver.numel()) * es
        r = dict(shape=s["name"], b=b, ncls=ncls, foreground_fraction=fg / label.numel(),
                 compulsory_bytes=dict(forward=fwd_bytes, forward_backward=fwd_bytes + bwd_bytes))

        def dev_fwd():
            with torch.no_grad():
                return NU.pvnet_loss(seg, ver, label, tgt, ncls)[:2]

        def dev_both():
            ls, lv, _ = NU.pvnet_loss(seg, ver, label, tgt, ncls)
            return (ls, lv, *torch.autograd.grad([ls.sum() + lv.sum()], [seg, ver]))

        def torch_fwd():
            with torch.no_grad():
                return torch_objective(seg, ver, label, tgt, ncls, VN)

        def torch_both():
            ls, lv = torch_objective(seg, ver, label, tgt, ncls, VN)
            return (ls, lv, *torch.autograd.grad([ls.sum() + lv.sum()], [seg, ver]))

        res = {}
        for key, fn, nbytes in (("forward", dev_fwd, fwd_bytes), ("forward_backward", dev_both, fwd_bytes + bwd_bytes),
                                ("forward_torch", torch_fwd, None), ("forward_backward_torch", torch_both, None)):
            ts, reps, res[key] = graph_time(fn, stream, a.window, a.rounds)
            r[key] = dict(ms_per_call=stats(ts), replays_per_window=reps)
            if nbytes is not None:
                rate = nbytes / (r[key]["ms_per_call"]["median"] * 1e-3)
                r[key].update(compulsory_bytes_per_s=rate, fraction_of_hbm_peak=rate / HBM_PEAK)
        for key in ("forward", "forward_backward"):
            r[key + "_torch_over_device"] = r[key + "_torch"]["ms_per_call"]["median"] / r[key]["ms_per_call"]["median"]
        # the two sides agree (float32 sums against float64 sums of float32 terms; float16 gradients)
        torch.cuda.synchronize()
        d, t = ([x.detach() for x in res[k]] for k in ("forward_backward", "forward_backward_torch"))
        r["max_relative_loss_difference_from_torch"] = float(max(((d[i] - t[i]).abs() / t[i].abs().clamp_min(1e-30)).max()
                                                                 for i in range(2)))
        r["max_gradient_difference_from_torch"] = float(max((d[i].float() - t[i].float()).abs().max() for i in (2, 3)))
        r["max_gradient_magnitude"] = float(max(t[i].float().abs().max() for i in (2, 3)))
        print(json.dumps(r), flush=True)
        rec["shapes"].append(r)
        del res, s, seg, ver, label, tgt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
