#!/usr/bin/env python3
"""Time model preparation: ``farthest_points`` (k = 8) and ``diameter`` (include/pvmodel.h).

Tables:

  linemod  13 models of 10,242 vertices (the bumpy ellipsoid at level 5, each scaled differently): every
           model is sampled by one block from LDS;
  ycb      21 models of 10,242 / 40,962 / 163,842 vertices (icospheres of levels 5 to 7, seven of each,
           each scaled differently): the per-step form beside the block form, and 2 x 10^11 pairs.

Per table each call is captured into a hipGraph and replayed between two device events, enough replays per
window to fill --window seconds; the median of --rounds windows is reported.  The baseline is the same work
composed from torch ops on the same device in float64, captured and timed the same way: for the sampling a
per-model loop of subtract / square / sum / minimum / argmax (5 k launches a model), for the diameter a
chunked ``torch.cdist(...).max()`` (it materialises the n^2 distances, --cdist-mib of them at a time).  For
the linemod table the numpy restatement (tests/model_ref.py) runs on the host as well: one model, once,
times the number of models.  Needs the GPU; there is no fallback.

    python tools/model_prep_probe.py [--rounds 5] [--window 0.3] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pvnet_amd import models as MO  # noqa: E402
from pvnet_amd import render as RN  # noqa: E402
from tests import model_ref as M  # noqa: E402
from tests import render_ref as R  # noqa: E402

K_PICKS = 8


def make_tables():
    rng = np.random.default_rng(0)
    v, f = R.bumpy_ellipsoid(5)
    linemod = [((v * rng.uniform(0.6, 1.8, 3)).astype(np.float32), f) for _ in range(13)]
    ycb = []
    for level in (5, 6, 7):
        v, f = R.icosphere(level, 0.05)
        ycb += [((v * rng.uniform(0.6, 1.8, 3)).astype(np.float32), f) for _ in range(7)]
    return {"linemod": linemod, "ycb": ycb}


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


def torch_fps(verts, k):
    """One model, float64, nothing read back -> idx i64 [k]."""
    c = verts.mean(0)
    pick = [torch.argmax(((verts - c) ** 2).sum(1), 0, keepdim=True)]
    dist = ((verts - verts.index_select(0, pick[0])) ** 2).sum(1)
    for _ in range(1, k):
        pick.append(torch.argmax(dist, 0, keepdim=True))
        dist = torch.minimum(dist, ((verts - verts.index_select(0, pick[-1])) ** 2).sum(1))
    return torch.cat(pick)


def torch_diameter(verts, rows):
    best = torch.zeros((), dtype=torch.float64, device=verts.device)
    for a in range(0, verts.shape[0], rows):
        best = torch.maximum(best, torch.cdist(verts[a:a + rows], verts).max())
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of replays per timed window")
    ap.add_argument("--cdist-mib", type=int, default=256, help="MiB of float64 distances torch.cdist makes at a time")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "model_prep_probe.json"))
    a = ap.parse_args()
    built = make_tables()
    plan = {name: dict(models=len(ms), vertices=[int(m[0].shape[0]) for m in ms],
                       pairs=int(sum(m[0].shape[0] * (m[0].shape[0] + 1) // 2 for m in ms))) for name, ms in built.items()}
    print("plan:", json.dumps({k: dict(models=v["models"], total=sum(v["vertices"]), pairs=v["pairs"]) for k, v in plan.items()}),
          flush=True)
    if not torch.cuda.is_available():
        raise RuntimeError("model_prep_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    rec = dict(device=torch.cuda.get_device_name(dev), k=K_PICKS, rounds=a.rounds, window_s=a.window,
               cdist_mib=a.cdist_mib, tables=[])
    for name, meshes in built.items():
        table = RN.MeshTable(meshes, device=dev)
        v64 = [torch.from_numpy(m[0]).to(dev).to(torch.float64) for m in meshes]
        rows = [max(1, (a.cdist_mib << 20) // 8 // v.shape[0]) for v in v64]
        r = dict(table=name, **plan[name])

        ts, reps, (idx, _) = graph_time(lambda: MO.farthest_points(table, K_PICKS), stream, a.window, a.rounds)
        r["farthest_points"] = dict(ms_per_call=stats(ts), replays_per_window=reps)
        ts, reps, tidx = graph_time(lambda: torch.stack([torch_fps(v, K_PICKS) for v in v64]), stream, a.window, a.rounds)
        r["farthest_points_torch"] = dict(ms_per_call=stats(ts), replays_per_window=reps,
                                          launches_about=5 * K_PICKS * len(meshes))
        r["farthest_points_torch_over_device"] = r["farthest_points_torch"]["ms_per_call"]["median"] / \
            r["farthest_points"]["ms_per_call"]["median"]
        r["farthest_points_indices_differing_from_torch"] = int((idx.to(torch.int64) != tidx).sum())

        ts, reps, diam = graph_time(lambda: MO.diameter(table), stream, a.window, a.rounds)
        ms = float(np.median(ts))
        r["diameter"] = dict(ms_per_call=stats(ts), replays_per_window=reps, pairs_per_s=plan[name]["pairs"] / (ms * 1e-3))
        ts, reps, tdiam = graph_time(lambda: torch.stack([torch_diameter(v, n) for v, n in zip(v64, rows)]), stream,
                                     a.window, min(a.rounds, 3))
        r["diameter_torch"] = dict(ms_per_call=stats(ts), replays_per_window=reps)
        r["diameter_torch_over_device"] = r["diameter_torch"]["ms_per_call"]["median"] / ms
        r["diameter_max_relative_difference_from_torch"] = float(((diam - tdiam).abs() / diam).max())

        if name == "linemod":
            v0 = M.widen(meshes[0][0])
            t0 = time.perf_counter()
            h = M.farthest_points(v0, K_PICKS)
            t_fps = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            hd = M.diameter(v0)
            t_d = (time.perf_counter() - t0) * 1e3
            r["numpy_one_model_ms"] = dict(farthest_points=t_fps, diameter=t_d)
            r["numpy_table_extrapolated_ms"] = dict(farthest_points=t_fps * len(meshes), diameter=t_d * len(meshes))
            r["numpy_model0_agrees"] = bool((idx[0].cpu().numpy() == h["idx"]).all() and float(diam[0]) == hd)
        print(json.dumps(r), flush=True)
        rec["tables"].append(r)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
