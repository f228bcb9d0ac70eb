#!/usr/bin/env python3
"""Time the colour render: ``shade.render_color`` (include/pvshade.h) beside ``render.render_labels``.

Scene: 32 frames of 480 x 640 with the LINEMOD camera, 1 and 8 instances per frame of an icosphere
subdivided to 20,480 triangles with random vertex colours, 10 cm across, 0.7-1.0 m away (a
LINEMOD-sized mesh: triangles of a pixel or less), shaded flat and smooth.

Per case three times:

  render_color   image + label, captured into a hipGraph and replayed between two device events, enough
                 replays per window to fill --window seconds; the median of --rounds windows;
  render_labels  label alone on the same meshes, poses and camera, timed the same way: the yardstick,
                 existing code doing strictly less work (no face index in the key, no shading pass);
  numpy          the restatement (tests/shade_ref.py) on frame 0 of the 1-instance cases, once.

Needs the GPU; there is no fallback.

    python tools/shade_probe.py [--b 32] [--rounds 5] [--window 0.3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from pvnet_amd import render as RN  # noqa: E402
from pvnet_amd import shade as SH  # noqa: E402
from pvnet_amd.synth import LINEMOD_K  # noqa: E402
from render_probe import graph_time, stats  # noqa: E402
from tests import render_ref as R  # noqa: E402
from tests import shade_ref as S  # noqa: E402

H, W = 480, 640


def make_scene(b, ninst, seed=0):
    """-> (model (verts, faces, colors), poses f64 [b, ninst, 3, 4])."""
    rng = np.random.default_rng(seed + ninst)
    v, f = R.icosphere(5, 0.05)
    colors = rng.integers(0, 256, size=(len(v), 3)).astype(np.uint8)
    poses = np.array([[R.pose(R.random_rotation(rng), [rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08),
                                                       rng.uniform(0.7, 1.0)]) for _ in range(ninst)] for _ in range(b)])
    return (v, f, colors), poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shade_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("shade_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    K = torch.from_numpy(LINEMOD_K).to(dev)
    lights = SH.random_lights(a.b, 1, device=dev)
    rec = dict(device=torch.cuda.get_device_name(dev), b=a.b, H=H, W=W, rounds=a.rounds, window_s=a.window, cases=[])
    for ninst in (1, 8):
        model, poses = make_scene(a.b, ninst)
        tp = torch.from_numpy(poses).to(dev)
        tm = torch.zeros((ninst,), dtype=torch.int32, device=dev)
        tl = tm + 1
        plain = RN.MeshTable([model[:2]], device=dev)
        lab_out = {"label": torch.empty((a.b, H, W), dtype=torch.uint8, device=dev)}

        def labels():
            return RN.render_labels(plain, tp, tm, tl, K, H, W, want=("label",), out=lab_out)

        ts_lab, reps_lab = graph_time(labels, stream, a.window, a.rounds)
        ms_lab = float(np.median(ts_lab))
        flat = SH.ColorMeshTable([model], device=dev)
        for smooth in (False, True):
            table = flat.with_smooth_normals() if smooth else flat
            out = {"image": torch.empty((a.b, H, W, 3), dtype=torch.uint8, device=dev),
                   "label": torch.empty((a.b, H, W), dtype=torch.uint8, device=dev)}

            def color():
                return SH.render_color(table, tp, tm, tl, K, H, W, lights=lights, want=("image", "label"), out=out)

            ts, reps = graph_time(color, stream, a.window, a.rounds)
            torch.cuda.synchronize()
            ms = float(np.median(ts))
            r = dict(instances_per_frame=ninst, shading="smooth" if smooth else "flat", triangles_per_frame=ninst * len(model[1]),
                     replays_per_window=reps, render_color_ms_per_call=stats(ts), render_color_us_per_frame=ms * 1e3 / a.b,
                     render_labels_ms_per_call=stats(ts_lab), render_labels_us_per_frame=ms_lab * 1e3 / a.b,
                     render_labels_replays_per_window=reps_lab, color_over_labels=ms / ms_lab,
                     foreground_pixels_per_frame=float(np.count_nonzero(out["label"].cpu().numpy())) / a.b,
                     label_maps_equal=bool(torch.equal(out["label"], lab_out["label"])))
            if ninst == 1:
                normals = table.normals.cpu().numpy() if smooth else None
                t0 = time.perf_counter()
                host = S.render([(*model, normals)], [(0, 1, poses[0, 0])], LINEMOD_K, H, W, lights[0].cpu().numpy())
                t_np = (time.perf_counter() - t0) * 1e3
                sure = ~host["contested"]
                r.update(numpy_ms_one_frame=t_np, numpy_batch_over_device=t_np * a.b / ms,
                         frame0_image_pixels_differing_from_numpy=int(np.count_nonzero(
                             (out["image"][0].cpu().numpy() != host["image"]).any(-1) & sure)),
                         frame0_contested_pixels=int(np.count_nonzero(host["contested"] & host["covered"])))
            print(json.dumps(r), flush=True)
            rec["cases"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
