#!/usr/bin/env python3
"""Time the ground-truth side: ``render_labels`` and ``vertex_field`` (include/pvrender.h).

Scenes: 32 frames of 480 x 640 with the LINEMOD camera, 1 and 3 instances per frame, of

  sphere  an icosphere subdivided to 20,480 triangles, 10 cm across, 0.7-1.0 m away (a LINEMOD-sized
          mesh: triangles of a pixel or less, one lane each);
  box     12 triangles, 20 cm across, 0.7-0.9 m away (triangles of about 10^4 pixels, a wave each).

Per scene, ``render_labels`` (label + inst + depth) is captured into a hipGraph and replayed between
two device events, enough replays per window to fill --window seconds; the median of --rounds windows is
reported as microseconds per frame and triangles per second.  ``vertex_field`` is timed the same way on the
3-sphere scene's label map at 18 channels (2 classes x 9 keypoints), for the contiguous layout in f32 and
f16 and the network's layout in f32; its bound is the HBM write of the output (it reads one byte per pixel
and writes 144), so the share reported is bytes written / time over the 8.0 TB/s peak (6.29 TB/s is what a
float4 copy reaches on this part).  The only baseline there is is the numpy restatement
(tests/render_ref.py) on the host: one frame of each scene, once, times the number of frames.
Needs the GPU; there is no fallback.

    python tools/render_probe.py [--b 32] [--rounds 5] [--window 0.3] [--out FILE]
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
from pvnet_amd import render as RN  # noqa: E402
from pvnet_amd.synth import LINEMOD_K  # noqa: E402
from tests import render_ref as R  # noqa: E402

H, W = 480, 640
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12


def make_scene(kind, b, ninst, seed=0):
    """-> (models, poses f64 [b, ninst, 3, 4], model_id [ninst])."""
    rng = np.random.default_rng(seed + ninst)
    if kind == "sphere":
        models, near, far, spread = [R.icosphere(5, 0.05), R.bumpy_ellipsoid(5)], 0.7, 1.0, 0.08
    else:
        models, near, far, spread = [R.box(0.1, 0.1, 0.1), R.box(0.1, 0.08, 0.06)], 0.7, 0.9, 0.12
    poses = np.array([[R.pose(R.random_rotation(rng), [rng.uniform(-spread, spread), rng.uniform(-spread, spread),
                                                       rng.uniform(near, far)]) for _ in range(ninst)] for _ in range(b)])
    return models, poses, np.arange(ninst) % 2


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
    """Capture fn, replay it in windows of `window` seconds -> (ms per call over the rounds, replays per window)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        fn()                                         # warm-up: workspace, code objects
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            fn()
    t1 = timed(g.replay, stream, 2)
    reps = max(2, int(math.ceil(window * 1e3 / t1)))
    return [timed(g.replay, stream, reps) for _ in range(rounds)], reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_probe.json"))
    a = ap.parse_args()
    scenes = [(kind, n) for kind in ("sphere", "box") for n in (1, 3)]
    built = {s: make_scene(s[0], a.b, s[1]) for s in scenes}
    plan = {f"{k}x{n}": dict(triangles_per_frame=int(sum(len(built[(k, n)][0][m][1]) for m in built[(k, n)][2])))
            for k, n in scenes}
    print("plan:", json.dumps(plan), flush=True)

    if not torch.cuda.is_available():
        raise RuntimeError("render_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    K = torch.from_numpy(LINEMOD_K).to(dev)
    rec = dict(device=torch.cuda.get_device_name(dev), b=a.b, H=H, W=W, rounds=a.rounds, window_s=a.window,
               hbm_peak_bytes_per_s=HBM_PEAK, hbm_float4_copy_bytes_per_s=HBM_COPY, render=[], vertex_field=[])
    field_label = None
    for kind, n in scenes:
        models, poses, mid = built[(kind, n)]
        table = RN.MeshTable(models, device=dev)
        tp = torch.from_numpy(poses).to(dev)
        tm = torch.from_numpy(mid).to(device=dev, dtype=torch.int32)
        tl = tm + 1
        out = {"label": torch.empty((a.b, H, W), dtype=torch.uint8, device=dev),
               "inst": torch.empty((a.b, H, W), dtype=torch.int32, device=dev),
               "depth": torch.empty((a.b, H, W), dtype=torch.float32, device=dev)}

        def render():
            return RN.render_labels(table, tp, tm, tl, K, H, W, out=out)

        ts, reps = graph_time(render, stream, a.window, a.rounds)
        torch.cuda.synchronize()
        label = out["label"].cpu().numpy()
        tris = plan[f"{kind}x{n}"]["triangles_per_frame"]
        t0 = time.perf_counter()
        host = R.render(models, [(int(m), int(m) + 1, poses[0, j]) for j, m in enumerate(mid)], LINEMOD_K, H, W)
        t_np = (time.perf_counter() - t0) * 1e3
        ms = float(np.median(ts))
        r = dict(scene=kind, instances_per_frame=n, triangles_per_frame=tris, replays_per_window=reps,
                 ms_per_call=stats(ts), us_per_frame=ms * 1e3 / a.b, triangles_per_s=tris * a.b / (ms * 1e-3),
                 foreground_pixels_per_frame=float(np.count_nonzero(label)) / a.b,
                 numpy_ms_one_frame=t_np, numpy_ms_batch_extrapolated=t_np * a.b, numpy_batch_over_device=t_np * a.b / ms,
                 frame0_label_pixels_differing_from_numpy=int(np.count_nonzero(label[0] != host["label"])))
        print(json.dumps(r), flush=True)
        rec["render"].append(r)
        if (kind, n) == ("sphere", 3):
            field_label = out["label"].clone()

    # the vector field on the 3-sphere scene's label map: 2 classes x 9 keypoints = 18 channels
    ncls, vn = 2, 9
    kp = torch.from_numpy(np.random.default_rng(1).uniform([0.0, 0.0], [W, H], size=(a.b, ncls, vn, 2))).to(dev)
    for layout, dtype in (("bhwk2", torch.float32), ("bhwk2", torch.float16), ("network", torch.float32)):
        es = 4 if dtype == torch.float32 else 2
        shape = (a.b, H, W, ncls * vn, 2) if layout == "bhwk2" else (a.b, 2 * ncls * vn, H, W)
        buf = torch.empty(shape, dtype=dtype, device=dev)

        def field():
            return RN.vertex_field(field_label, kp, ncls, dtype=dtype, layout=layout, out=buf)

        ts, reps = graph_time(field, stream, a.window, a.rounds)
        ms = float(np.median(ts))
        nbytes = buf.numel() * es
        r = dict(layout=layout, dtype=str(dtype).replace("torch.", ""), channels=ncls * vn, replays_per_window=reps,
                 ms_per_call=stats(ts), us_per_frame=ms * 1e3 / a.b, bytes_written=nbytes,
                 write_bytes_per_s=nbytes / (ms * 1e-3), share_of_hbm_peak=nbytes / (ms * 1e-3) / HBM_PEAK,
                 share_of_float4_copy_rate=nbytes / (ms * 1e-3) / HBM_COPY)
        print(json.dumps(r), flush=True)
        rec["vertex_field"].append(r)
    torch.cuda.synchronize()
    lab0 = field_label[0].cpu().numpy()
    t0 = time.perf_counter()
    R.vertex_field(lab0, kp[0].cpu().numpy())
    t_np = (time.perf_counter() - t0) * 1e3
    rec["vertex_field_numpy_ms_one_frame"] = t_np
    rec["vertex_field_numpy_ms_batch_extrapolated"] = t_np * a.b
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
