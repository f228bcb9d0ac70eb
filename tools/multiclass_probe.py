#!/usr/bin/env python3
"""One multi-object voting call against the loop of per-class calls.

A 480 x 640 frame with C = 8 non-overlapping disks (one object each), vn = 9
keypoints per class, 512 hypotheses.  Two hipGraphs are captured:

  multi: one ransac_voting_layer_v3_multi call (label map + [1,h,w,C*vn,2]);
  loop:  for every class, ``label == c + 1`` made by torch and the existing
         ransac_voting_layer_v3 on it and the class's slice of the vertex
         tensor (a strided view: the layer reads it in place).

Each graph is replayed in windows of --replays replays between two device
events, the two graphs alternating, --rounds windows each.  Prints one JSON
line: the graphs' kernel nodes, the per-frame times (median and range over
the windows) and their ratio.  Needs the GPU; there is no fallback.

    python tools/multiclass_probe.py [--replays 200] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvnet_amd import _lib  # noqa: E402
from pvnet_amd import ransac_voting_gpu as rvg  # noqa: E402

H, W, C, VN, NH = 480, 640, 8, 9, 512


def make_frame(seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    label = np.zeros((H, W), np.int64)
    vertex = np.zeros((H, W, C * VN, 2), np.float32)
    kps = np.zeros((C, VN, 2), np.float32)
    for c in range(C):                      # a 4 x 2 grid of disks, radius 60..75: 11-18 thousand pixels each
        cx, cy, r = 80 + 160 * (c % 4), 120 + 240 * (c // 4), 60 + 5 * (c % 4)
        own = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        label[own] = c + 1
        kps[c] = np.stack([cx + rng.uniform(-r, r, VN), cy + rng.uniform(-r, r, VN)], 1)
        for v in range(VN):
            d = kps[c, v][None, None] - np.stack([xx, yy], -1).astype(np.float32)
            d = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-6)
            vertex[own, c * VN + v] = d[own]
    return label, vertex, kps


def capture(fn, stream):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        fn()                                # warm-up: workspaces allocated, code objects loaded
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            out = fn()
    return g, out


def window(g, stream, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        for _ in range(replays):
            g.replay()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / replays      # us per replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiclass_probe needs the GPU")
    dev = torch.device("cuda:0")
    label_h, vertex_h, kps = make_frame()
    label = torch.from_numpy(label_h).to(dev)[None]
    vertex = torch.from_numpy(vertex_h).to(dev)[None]
    ws_m, ws_l = rvg.VotingWorkspace(), rvg.VotingWorkspace()

    def multi():
        return rvg.ransac_voting_layer_v3_multi(label, vertex, C, NH, _seed=11, _workspace=ws_m)

    def loop():
        return [rvg.ransac_voting_layer_v3(label == c + 1, vertex[:, :, :, c * VN:(c + 1) * VN], NH, _seed=11 + c,
                                           _workspace=ws_l) for c in range(C)]

    s = torch.cuda.Stream()
    gm, om = capture(multi, s)
    gl, ol = capture(loop, s)
    for g in (gm, gl):                      # a few replays of each before the timed windows
        window(g, s, 20)
    tm, tl = [], []
    for _ in range(a.rounds):
        tm.append(window(gm, s, a.replays))
        tl.append(window(gl, s, a.replays))
    torch.cuda.synchronize()
    km = om.cpu().numpy()[0]
    kl = np.stack([o.cpu().numpy()[0] for o in ol])
    L = _lib.load()
    res = dict(probe="multiclass", shape=[H, W], classes=C, vn=VN, hn=NH, replays=a.replays, rounds=a.rounds,
               nodes_multi=L.pv_v3_kernel_launches(C, H, W, VN, NH),
               nodes_loop=C * (L.pv_v3_kernel_launches(1, H, W, VN, NH) + 1),     # + torch's label == c + 1
               multi_us=round(float(np.median(tm)), 2), multi_us_range=[round(min(tm), 2), round(max(tm), 2)],
               loop_us=round(float(np.median(tl)), 2), loop_us_range=[round(min(tl), 2), round(max(tl), 2)],
               loop_over_multi=round(float(np.median(tl) / np.median(tm)), 3),
               max_err_px_multi=round(float(np.abs(km - kps).max()), 4),
               max_err_px_loop=round(float(np.abs(kl - kps).max()), 4),
               build_config=L.pv_build_config().decode())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
