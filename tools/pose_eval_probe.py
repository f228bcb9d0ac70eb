#!/usr/bin/env python3
"""The fused pose metrics against the way a user would write ADD-S today.

b poses of one model of pn vertices (default b = 64; pn = 2048, 8192, 32768), metrics
ADD + ADD-S + PROJ + 5 cm 5 deg.  Per size, in one process and alternating round by round:

  fused: one ``pose_metrics`` call (two launches), captured into a hipGraph and replayed
         between two device events, enough replays per window to fill --window seconds;
  cdist: the same ADD-S written with torch -- both clouds transformed on the device, then
         ``torch.cdist(gt, pred).min(-1)`` in chunks of at most 2^26 distances (256 MB),
         which writes and re-reads b * pn^2 * 4 bytes in all;
  numpy: the chunked float32 numpy form on the host, for one pose (once per size).

Recorded per size: ms per call (median and range over the rounds), the pair rate, and the
share of the fp32 vector peak.  The operation count is the algorithm's, from the shapes:
b * pn^2 pairs of 9 fp32 vector operations (3 subtractions, 3 products, 2 sums, 1 minimum;
no fused multiply-add, the distance is defined with every operation rounded).  The kernel
moves 12 * pn bytes per pose from L2 and nothing else per pair, so vector issue is the bound
that applies: the peak is the MI355X's 157.3 TFLOP/s fp32 vector rate counted as
instructions, 78.65e12 lane operations a second.  Needs the GPU; there is no fallback.

    python tools/pose_eval_probe.py [--b 64] [--sizes 2048,8192,32768] [--rounds 5] [--out FILE]
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
from pvnet_amd import evaluation_utils as EV  # noqa: E402
from pvnet_amd.synth import LINEMOD_K  # noqa: E402

OPS_PER_PAIR = 9
PEAK_LANE_OPS = 157.3e12 / 2          # fp32 vector peak as instructions x lanes (an FMA counts two FLOP)
METRICS = ("add", "adds", "proj", "cmdeg")
CHUNK = 1 << 26                        # distances per cdist call


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def make_case(b, pn, seed=0):
    """A model of pn vertices on a 10 cm blob, b ground-truth poses about 0.9 m away and
    predictions a few degrees / millimetres off."""
    rng = np.random.default_rng(seed + pn)
    pts = (rng.standard_normal((pn, 3)) * 0.03).astype(np.float32)
    gt, pred = np.zeros((b, 3, 4)), np.zeros((b, 3, 4))
    for i in range(b):
        R = rodrigues(rng.standard_normal(3), rng.uniform(0, np.pi))
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.1)])
        gt[i] = np.concatenate([R, t[:, None]], 1)
        dR = rodrigues(rng.standard_normal(3), np.radians(rng.uniform(0.5, 8.0)))
        pred[i] = np.concatenate([dR @ R, (t + rng.standard_normal(3) * 0.004)[:, None]], 1)
    return pts, pred, gt


def pair_ops(b, pn):
    pairs = b * pn * pn
    return pairs, pairs * OPS_PER_PAIR


def adds_numpy(pts, pp, pg, chunk=256):
    """ADD-S of one pose on the host: float32, chunked."""
    g = (pts @ pg[:, :3].T.astype(np.float32) + pg[:, 3].astype(np.float32)).astype(np.float32)
    q = (pts @ pp[:, :3].T.astype(np.float32) + pp[:, 3].astype(np.float32)).astype(np.float32)
    tot = 0.0
    for s in range(0, len(g), chunk):
        d = g[s:s + chunk, None, :] - q[None, :, :]
        tot += float(np.sqrt((d * d).sum(-1).min(1)).sum(dtype=np.float64))
    return tot / len(g)


def adds_cdist(pts, pred, gt):
    """ADD-S of every pose with torch.cdist, chunked to CHUNK distances per call."""
    b, pn = pred.shape[0], pts.shape[0]
    g = torch.matmul(pts, gt[:, :, :3].transpose(1, 2)) + gt[:, None, :, 3]
    q = torch.matmul(pts, pred[:, :, :3].transpose(1, 2)) + pred[:, None, :, 3]
    out = torch.empty(b, dtype=torch.float32, device=pts.device)
    bc = max(1, CHUNK // (pn * pn))
    qc = min(pn, max(1, CHUNK // pn))
    for s in range(0, b, bc):
        acc = torch.zeros(min(bc, b - s), dtype=torch.float32, device=pts.device)
        for r in range(0, pn, qc):
            acc += torch.cdist(g[s:s + bc, r:r + qc], q[s:s + bc]).min(-1).values.sum(-1)
        out[s:s + bc] = acc / pn
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=64)
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of fused replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_eval_probe.json"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    cases = {pn: make_case(a.b, pn) for pn in sizes}
    plan = {pn: dict(zip(("pairs", "lane_ops"), pair_ops(a.b, pn))) for pn in sizes}
    print("plan:", json.dumps(plan), flush=True)

    if not torch.cuda.is_available():
        raise RuntimeError("pose_eval_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    K = torch.from_numpy(LINEMOD_K).to(dev)
    rec = dict(device=torch.cuda.get_device_name(dev), b=a.b, metrics=list(METRICS), ops_per_pair=OPS_PER_PAIR,
               peak_lane_ops_per_s=PEAK_LANE_OPS, bound="vector issue", rounds=a.rounds, sizes=[])
    for pn in sizes:
        pts, pred, gt = cases[pn]
        table = EV.ModelTable([(pts, 0.1, True)], dev)
        tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        tp32, tg32, pts32 = tp.float(), tg.float(), table.points
        out = torch.empty((a.b, 6), dtype=torch.float64, device=dev)

        def fused():
            return EV.pose_metrics(tp, tg, table, K, None, METRICS, out=out)

        def cdist():
            return adds_cdist(pts32, tp32, tg32)

        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            fused()                                  # warm-up: workspace, code objects
            ref_cd = cdist()                         # warm-up of the baseline, and its result
            stream.synchronize()
            with torch.cuda.graph(g, stream=stream):
                fused()
        t1 = timed(g.replay, stream, 2)
        reps = max(2, int(math.ceil(a.window * 1e3 / t1)))
        tf, tc = [], []
        for _ in range(a.rounds):                    # alternating, one process
            tf.append(timed(g.replay, stream, reps))
            tc.append(timed(cdist, stream, 1))
        torch.cuda.synchronize()
        adds = out[:, 1].cpu().numpy()
        t0 = time.perf_counter()
        host = adds_numpy(pts, pred[0], gt[0])
        t_np = (time.perf_counter() - t0) * 1e3
        pairs, ops = pair_ops(a.b, pn)
        ms = float(np.median(tf))
        r = dict(pn=pn, replays_per_window=reps, fused_ms=stats(tf), cdist_ms=stats(tc),
                 numpy_ms_one_pose=t_np, numpy_ms_batch_extrapolated=t_np * a.b,
                 pairs=pairs, pair_rate_per_s=pairs / (ms * 1e-3), lane_ops=ops,
                 share_of_fp32_vector_peak=ops / (ms * 1e-3) / PEAK_LANE_OPS,
                 cdist_over_fused=float(np.median(tc)) / ms, numpy_batch_over_fused=t_np * a.b / ms,
                 cdist_bytes_written_and_reread=2 * 4 * pairs,
                 adds_max_abs_diff_vs_cdist=float(np.abs(adds - ref_cd.cpu().numpy()).max()),
                 adds_abs_diff_vs_numpy_pose0=float(abs(adds[0] - host)))
        print(json.dumps(r), flush=True)
        rec["sizes"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
