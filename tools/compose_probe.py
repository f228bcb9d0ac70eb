#!/usr/bin/env python3
"""Time the frame composition (include/pvcompose.h, pvnet_amd/compose.py): ``compose``, ``finish`` at each
kernel size, and the chain params -> compose -> finish.

Shape: a bank of 64 frames of 480 x 640 (random pixels, one ellipse of label 1 per frame), b = 32 output
frames of 480 x 640 with S = 4 slots and E = 2 erasers, u8 labels, one background per frame.

Each call is captured into a hipGraph and replayed between two device events, enough replays per window
to fill --window seconds; the median of --rounds windows is reported (tools/augment_probe.py's method).
The baseline is the same result composed from torch ops on the same device and captured the same way: a
slot loop of gathers and ``torch.where`` for the paste, comparisons for the erasers, and for the finish a
reflect pad and two depthwise ``conv2d`` passes with the same weights plus four ``torch.rand`` fields for
the noise.  The numpy restatement (tests/compose_ref.py) is timed once on the host, the finish on 2 frames.

Algorithmic bytes, from the shapes and the counted result: compose reads the background (3 B) and writes
image and label (3 + 1 B) per output pixel, and reads label and colour (1 + 3 B) per pixel a slot shows;
finish reads and writes the image (3 + 3 B per pixel).  Needs the GPU; there is no fallback.

    python tools/compose_probe.py [--rounds 5] [--window 0.3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pvnet_amd import compose as CP  # noqa: E402
from tests import compose_ref as CR  # noqa: E402
from tools.augment_probe import graph_time, stats  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, the part's specification
N, B, H, W, S, E = 64, 32, 480, 640, 4, 2
KW = dict(margin=0.25, erasers=E, erase_frac=(0.1, 0.4), blur_p=0.5, noise=(0.0, 8.0), class_num=S)


def make_bank(rng):
    y, x = np.mgrid[:H, :W]
    label = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        cx, cy = rng.uniform(200, 440), rng.uniform(160, 320)
        rx, ry = rng.uniform(50, 110), rng.uniform(40, 90)
        label[i] = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1.0
    return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), label


# ---- the composition from torch ops ------------------------------------------------------------------------
def torch_compose(bank_image, bank_label, pick, shift, erase, background, k):
    """The same image, label and instance maps from gathers and torch.where, slot by slot."""
    b = pick.shape[0]
    img, lab = background.clone(), torch.zeros((b, H, W), dtype=torch.uint8, device=pick.device)
    inst = torch.zeros_like(lab)
    for s in range(S):
        src = pick[:, s, 0].long()
        live = (src >= 0) & (src < N) & (pick[:, s, 2] >= 1) & (pick[:, s, 2] <= S)
        yy = k["y"] - shift[:, s, 1].long()[:, None, None]                  # [b, H, 1]
        xx = k["x"] - shift[:, s, 0].long()[:, None, None]                  # [b, 1, W]
        box = pick[:, s, 3:7].long()[:, :, None, None]
        ok = live[:, None, None] & (xx >= box[:, 0].clamp(min=0)) & (xx <= box[:, 2].clamp(max=W - 1)) & \
            (yy >= box[:, 1].clamp(min=0)) & (yy <= box[:, 3].clamp(max=H - 1))
        sc, yc, xc = src.clamp(0, N - 1)[:, None, None], yy.clamp(0, H - 1), xx.clamp(0, W - 1)
        hit = ok & (bank_label[sc, yc, xc] == pick[:, s, 1, None, None].to(torch.uint8))
        img = torch.where(hit[..., None], bank_image[sc, yc, xc], img)
        lab = torch.where(hit, pick[:, s, 2, None, None].to(torch.uint8), lab)
        inst = torch.where(hit, k["slot"][s], inst)
    for e in range(E):
        q = erase[:, e].long()[:, :, None, None]
        gone = (k["x"] >= q[:, 0]) & (k["x"] <= q[:, 2]) & (k["y"] >= q[:, 1]) & (k["y"] <= q[:, 3])
        img = torch.where(gone[..., None], k["zero"], img)
        lab = torch.where(gone, k["zero"], lab)
        inst = torch.where(gone, k["zero"], inst)
    visible = torch.stack([(inst == s + 1).sum((1, 2)) for s in range(S)], 1).to(torch.int32)
    return img, lab, inst, visible


def torch_finish(image_chw, j, amp, k):
    """image_chw u8 [b, 3, H, W] -> u8: reflect pad, two depthwise passes, four uniform fields for the noise."""
    c = image_chw.float()
    if j:
        c = F.conv2d(F.pad(c, (j, j, 0, 0), mode="reflect"), k["wh"][j], groups=3)
        c = F.conv2d(F.pad(c, (0, 0, j, j), mode="reflect"), k["wv"][j], groups=3)
    t = (torch.rand((4, *c.shape), device=c.device).sum(0) - 2.0) * (65535.0 / 65536.0)
    return (c + amp[:, None, None, None] * t).clamp(0, 255).round().to(torch.uint8)


def constants(dev):
    w = CP.blur_kernels()
    full = {j: torch.cat([w[j, 1:j + 1].flip(0), w[j, :j + 1]]).to(dev) for j in range(1, 5)}
    return dict(y=torch.arange(H, device=dev)[None, :, None], x=torch.arange(W, device=dev)[None, None, :],
                slot=[torch.tensor(s + 1, dtype=torch.uint8, device=dev) for s in range(S)],
                zero=torch.tensor(0, dtype=torch.uint8, device=dev),
                wh={j: v.view(1, 1, 1, -1).repeat(3, 1, 1, 1) for j, v in full.items()},
                wv={j: v.view(1, 1, -1, 1).repeat(3, 1, 1, 1) for j, v in full.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "compose_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("compose_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    rng = np.random.default_rng(1)
    bank_image_np, bank_label_np = make_bank(rng)
    bank_image, bank_label = torch.from_numpy(bank_image_np).to(dev), torch.from_numpy(bank_label_np).to(dev)
    background = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    from pvnet_amd import augment as AU
    bank_stats = AU.label_stats(bank_label, 1)
    src = torch.from_numpy(rng.integers(0, N, (B, S))).to(dev)
    cls = torch.arange(1, S + 1, device=dev)[None].expand(B, S)
    pick = CP.make_picks(src, cls, bank_stats)
    state = torch.tensor([2024, 0], dtype=torch.int64, device=dev)
    k = constants(dev)
    pl = CP.random_placement(pick, (N, H, W), (H, W), state, **KW)
    composed = CP.compose(bank_image, bank_label, pick, pl.shift, S, (H, W), background=background, erase=pl.erase,
                          want_instance=True)
    torch.cuda.synchronize()
    shown = int(composed[3].sum())
    px = B * H * W
    compose_bytes = px * (3 + 3 + 1 + 1) + shown * (1 + 3)                 # + the instance map, which this run writes
    finish_bytes = px * 6
    rec = dict(device=torch.cuda.get_device_name(dev), bank=N, b=B, H=H, W=W, S=S, E=E, label_dtype="uint8",
               rounds=a.rounds, window_s=a.window, hbm_peak_bytes_per_s=HBM_PEAK, pixels_shown_by_slots=shown,
               algorithmic_bytes=dict(compose=compose_bytes, finish=finish_bytes, chain=compose_bytes + finish_bytes))
    image_chw = composed[0].permute(0, 3, 1, 2).contiguous()
    amp = torch.full((B,), 4.0, device=dev)

    def dev_compose():
        return CP.compose(bank_image, bank_label, pick, pl.shift, S, (H, W), background=background, erase=pl.erase,
                          want_instance=True)

    def dev_chain():
        p = CP.random_placement(pick, (N, H, W), (H, W), state, **KW)
        img, lab, inst, vis = CP.compose(bank_image, bank_label, pick, p.shift, S, (H, W), background=background,
                                         erase=p.erase, want_instance=True)
        return CP.finish(img, p.ksel, p.amp, state), lab, inst, vis

    def t_chain():
        img, lab, inst, vis = torch_compose(bank_image, bank_label, pick, pl.shift, pl.erase, background, k)
        return torch_finish(img.permute(0, 3, 1, 2), 2, amp, k), lab, inst, vis

    runs = [("compose", dev_compose, compose_bytes),
            ("compose_torch", lambda: torch_compose(bank_image, bank_label, pick, pl.shift, pl.erase, background, k), None)]
    for j in range(5):
        ks = torch.full((B,), j, dtype=torch.int32, device=dev)
        runs.append((f"finish_k{2 * j + 1}", lambda ks=ks: CP.finish(composed[0], ks, amp, state), finish_bytes))
        runs.append((f"finish_k{2 * j + 1}_torch", lambda j=j: torch_finish(image_chw, j, amp, k), None))
    runs.append(("finish_copy", lambda: CP.finish(composed[0], torch.zeros_like(pl.ksel), torch.zeros_like(amp), state), finish_bytes))
    runs += [("chain", dev_chain, compose_bytes + finish_bytes), ("chain_torch_k5", t_chain, None)]
    res = {}
    for key, fn, nbytes in runs:
        ts, reps, res[key] = graph_time(fn, stream, a.window, a.rounds)
        rec[key] = dict(ms_per_call=stats(ts), replays_per_window=reps)
        if nbytes is not None:
            rate = nbytes / (rec[key]["ms_per_call"]["median"] * 1e-3)
            rec[key].update(algorithmic_bytes_per_s=rate, fraction_of_hbm_peak=rate / HBM_PEAK)
        print(key, json.dumps(rec[key]), flush=True)
    for key in ["compose"] + [f"finish_k{2 * j + 1}" for j in range(5)]:
        rec[key + "_torch_over_device"] = rec[key + "_torch"]["ms_per_call"]["median"] / rec[key]["ms_per_call"]["median"]
    rec["chain_torch_over_device"] = rec["chain_torch_k5"]["ms_per_call"]["median"] / rec["chain"]["ms_per_call"]["median"]
    # agreement: the torch paste gives the same maps; its blur the same image to the last rounding (amp = 0)
    torch.cuda.synchronize()
    rec["compose_mismatches_from_torch"] = [int((x != y).sum()) for x, y in zip(res["compose"], res["compose_torch"])]
    zero = torch.zeros_like(amp)
    d = CP.finish(composed[0][:4], torch.full((4,), 2, dtype=torch.int32, device=dev), zero[:4], state)
    t = torch_finish(image_chw[:4], 2, zero[:4], k).permute(0, 2, 3, 1)
    rec["finish_k5_max_difference_from_torch_grey_levels"] = int((d.int() - t.int()).abs().max())
    # the numpy restatement, on the host
    pick_np, shift_np, erase_np = pick.cpu().numpy(), pl.shift.cpu().numpy(), pl.erase.cpu().numpy()
    t0 = time.perf_counter()
    ref = CR.compose(bank_image_np, bank_label_np, pick_np, shift_np, S, H, W, background.cpu().numpy(), (0, 0, 0), erase_np)
    rec["compose_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    rec["compose_equals_numpy"] = all(bool(np.array_equal(g.cpu().numpy(), r)) for g, r in zip(composed, ref))
    t0 = time.perf_counter()
    ref_f = CR.finish(ref[0][:2], np.full(2, 2, np.int32), np.full(2, 4.0, np.float32), 2024, 0)
    rec["finish_k5_numpy_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / 2
    got_f = CP.finish(composed[0][:2], torch.full((2,), 2, dtype=torch.int32, device=dev), amp[:2], state)
    rec["finish_equals_numpy"] = bool(np.array_equal(got_f.cpu().numpy(), ref_f))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
