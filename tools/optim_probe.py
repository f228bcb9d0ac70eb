#!/usr/bin/env python3
"""Time the optimiser step (include/pvoptim.h, pvnet_amd/optim.py) on ``PVNet()``'s real parameter list.

Configurations: the f16 network (f16 model and gradients, f32 masters) and the f32 network (the parameters
are the masters, f32 gradients), each with Adam, AdamW and SGD, loss scaling and a global-norm clip on.

Each step is timed two ways: captured into a hipGraph and replayed between two device events, and as
back-to-back eager calls, enough per window to fill --window seconds; the median of --rounds windows is
reported.  The baseline is the torch composition of the same step on an f32 copy of the parameters --
``GradScaler.unscale_`` + ``clip_grad_norm_`` + ``GradScaler.step(torch.optim.Adam)`` +
``GradScaler.update`` + ``zero_grad(set_to_none=False)`` -- once with ``fused=True`` and once with
``foreach=True``, timed as back-to-back eager calls in windows that alternate with the device step's (its
``step`` reads ``found_inf`` on the host with foreach, so it is not captured).

The bytes are computed from the shapes: the norm pass reads every gradient once; the update reads gradient,
master, m and v and writes master, m, v, the f16 model when there is one, and the zeroed gradient.  The three
kernels' own times come from torch.profiler over a few eager steps (when the profiler gives device events);
the apply kernel's bytes over its time is its share of the HBM roofline.  Needs the GPU; there is no fallback.

    python tools/optim_probe.py [--rounds 5] [--window 0.2] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pvnet_amd import optim as O  # noqa: E402
from pvnet_amd.network import PVNet  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, the part's specification
MAX_NORM = 10.0
SCALE = 1024.0


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


def reps_for(fn, stream, window):
    timed(fn, stream, 3)                             # warm-up: code objects, allocator
    return max(2, int(math.ceil(window * 1e3 / timed(fn, stream, 5))))


def kernel_times(fn, steps=10):
    """Mean device time in ms of each pvoptim kernel over `steps` eager steps, or None without device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for key in ("k_optim_stats", "k_optim_decide", "k_optim_apply"):
                if key in ev.key:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    out[key] = out.get(key, 0.0) + float(total) / ev.count * 1e-3
        return out if len(out) == 3 else None
    except Exception as e:                           # a profiler without device support: the step time alone
        print("kernel times unavailable:", repr(e), flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of steps per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("optim_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    torch.manual_seed(0)
    net = PVNet()
    shapes = [tuple(p.shape) for p in net.parameters()]
    n_total = sum(int(np.prod(s)) for s in shapes)
    rec = dict(device=torch.cuda.get_device_name(dev), network="PVNet()", tensors=len(shapes), parameters=n_total,
               chunk=O.P.PV_OPT_CHUNK, rounds=a.rounds, window_s=a.window, hbm_peak_bytes_per_s=HBM_PEAK,
               max_norm=MAX_NORM, scale=SCALE, torch_version=torch.__version__, configs=[])

    # ---- the torch compositions, on an f32 copy
    def torch_form(**kw):
        ps = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in net.parameters()]
        for p in ps:
            p.grad = torch.zeros_like(p)
        opt = torch.optim.Adam(ps, lr=1e-3, **kw)
        scaler = torch.amp.GradScaler("cuda", init_scale=SCALE, growth_interval=2000)
        scaler.scale(torch.zeros((), device=dev))    # creates the device-side scale that unscale_ asks for

        def step():
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
            scaler.step(opt)
            scaler.update()
            opt.zero_grad(set_to_none=False)
        return step

    torch_steps = {"torch_fused": torch_form(fused=True), "torch_foreach": torch_form(foreach=True)}
    torch_reps = {k: reps_for(fn, stream, a.window) for k, fn in torch_steps.items()}
    torch_ms = {k: [] for k in torch_steps}

    for kind in ("f16", "f32"):
        for alg in ("adam", "adamw", "sgd"):
            src = net.half() if kind == "f16" else net.float()
            named = [(n, torch.nn.Parameter(p.detach().clone().to(dev))) for n, p in src.named_parameters()]
            opt = O.Optimizer(named, alg, lr=1e-3, weight_decay=0.01 if alg != "adam" else 0.0, momentum=0.9,
                              max_norm=MAX_NORM, init_scale=SCALE)
            gs = 2 if kind == "f16" else 4
            moments = 1 if alg == "sgd" else 2
            model = 2 if kind == "f16" else 0
            b_stats = gs * n_total
            b_apply = (gs + 4 + 4 * moments) * n_total + (4 + 4 * moments + model + gs) * n_total
            r = dict(kind=kind, algorithm=alg, chunks=opt._n_chunks, bytes=dict(stats=b_stats, apply=b_apply, step=b_stats + b_apply),
                     bytes_per_parameter=(b_stats + b_apply) / n_total)
            # captured
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(stream):
                opt.step()
                stream.synchronize()
                with torch.cuda.graph(g, stream=stream):
                    opt.step()
            reps_g = reps_for(g.replay, stream, a.window)
            reps_e = reps_for(opt.step, stream, a.window)
            ms_g, ms_e = [], []
            for _ in range(a.rounds):                 # the forms alternate inside one call
                ms_g.append(timed(g.replay, stream, reps_g))
                ms_e.append(timed(opt.step, stream, reps_e))
                if alg == "adam":
                    for k, fn in torch_steps.items():
                        torch_ms[k].append(timed(fn, stream, torch_reps[k]))
            r["graph_replay"] = dict(ms_per_step=stats(ms_g), steps_per_window=reps_g)
            r["eager"] = dict(ms_per_step=stats(ms_e), steps_per_window=reps_e)
            rate = (b_stats + b_apply) / (r["graph_replay"]["ms_per_step"]["median"] * 1e-3)
            r["graph_replay"].update(bytes_per_s=rate, fraction_of_hbm_peak=rate / HBM_PEAK)
            kt = kernel_times(opt.step)
            if kt:
                r["kernels_ms"] = kt
                r["apply_bytes_per_s"] = b_apply / (kt["k_optim_apply"] * 1e-3)
                r["apply_fraction_of_hbm_peak"] = r["apply_bytes_per_s"] / HBM_PEAK
                r["small_launches_share_of_kernel_time"] = (kt["k_optim_stats"] + kt["k_optim_decide"]) / sum(kt.values())
            st = opt.stats()
            r["state_after"] = dict(step=int(st["step"]), skipped=int(st["skipped"]), scale=float(st["scale"]))
            print(json.dumps(r), flush=True)
            rec["configs"].append(r)
            del opt, named, g
            torch.cuda.empty_cache()
    rec["torch"] = {k: dict(ms_per_step=stats(v), steps_per_window=torch_reps[k]) for k, v in torch_ms.items()}
    for r in rec["configs"]:
        if r["algorithm"] == "adam":
            for k in torch_steps:
                t = rec["torch"][k]["ms_per_step"]["median"]
                r[k + "_over_device_eager"] = t / r["eager"]["ms_per_step"]["median"]
                r[k + "_over_device_graph"] = t / r["graph_replay"]["ms_per_step"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
