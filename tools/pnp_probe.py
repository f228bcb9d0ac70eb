#!/usr/bin/env python3
"""The plain PnP three ways: timing and an accuracy census.

Timing, b = 1,024 images of pn = 9 and 21 keypoints (1 px noise), one process, alternating round
by round, each path captured into a hipGraph and replayed between two device events, enough
replays per window to fill --window seconds:

  epnp      ``pv_epnp`` alone (``pnp_batch(method="epnp")``)
  epnp_lm   ``pv_epnp`` -> ``pv_uncertainty_pnp_refine`` -> ``pv_rt6_to_Rt``
  p3p_lm    the existing ``pv_uncertainty_pnp`` at unit weights on the same inputs
  numpy     tests/epnp_ref.py on one core, --ref-images images, extrapolated to the batch

Census, --census poses per setting (9 and 21 points; 1 px and 3 px keypoint noise, and 1 px with
one gross outlier of --outlier px on a keypoint among 0..3): poses more than 15 degrees from the
truth for p3p_lm, epnp and epnp_lm.

Sign after the LM (CPU only, runs without a GPU): tests/epnp_ref.py with the control-axis sign
convention and with the flipped one, each followed by oracle.pnp.ceres_lm; the spread of the two
final poses, against the spread of the two EPnP poses before it.

    python tools/pnp_probe.py [--b 1024] [--rounds 5] [--census 1000] [--no-gpu] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import pnp as O  # noqa: E402
from tests import epnp_ref as E  # noqa: E402

K_LM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
SETTINGS = (("1px", 1.0, False), ("3px", 3.0, False), ("1px+outlier", 1.0, True))


def model(pn, rng):
    return E.cuboid_model() if pn == 9 else E.random_model(rng, pn)


def make_poses(n, pn, noise, outlier, seed, outlier_px=50.0):
    rng = np.random.default_rng(seed)
    p3 = model(pn, rng)
    Rt = np.stack([E.random_pose(rng, np.pi) for _ in range(n)])
    p2 = np.stack([E.project(Rt[i], p3, K_LM) for i in range(n)]) + noise * rng.standard_normal((n, pn, 2))
    if outlier:
        k = rng.integers(0, 4, n)
        ang = rng.uniform(0, 2 * np.pi, n)
        p2[np.arange(n), k] += outlier_px * np.stack([np.cos(ang), np.sin(ang)], 1)
    return p3, Rt, p2


def rot_deg(Ra, Rb):
    tr = np.einsum("bij,bij->b", Ra, Rb)
    return np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))


def sign_after_lm(n, pn=9):
    """EPnP under both sign conventions, then the LM: how far apart are the two results?"""
    out = []
    w = np.tile(np.array([1.0, 0.0, 1.0]), (pn, 1))
    for noise in (1.0, 3.0):
        p3, _, p2 = make_poses(n, pn, noise, False, seed=77)
        before, after = [], []
        for i in range(n):
            a, b = E.epnp(p3, p2[i], K_LM, sign=+1), E.epnp(p3, p2[i], K_LM, sign=-1)
            xa = O.ceres_lm(a["rt6"], p2[i], p3, w, K_LM)
            xb = O.ceres_lm(b["rt6"], p2[i], p3, w, K_LM)
            before.append(np.abs(a["Rt"] - b["Rt"]).max())
            Ra = np.concatenate([O.rodrigues_vec_to_mat(xa[:3]), xa[3:, None]], 1)
            Rb = np.concatenate([O.rodrigues_vec_to_mat(xb[:3]), xb[3:, None]], 1)
            after.append(np.abs(Ra - Rb).max())
        out.append(dict(pn=pn, noise_px=noise, poses=n, epnp_spread=stats(before), epnp_lm_spread=stats(after),
                        epnp_lm_spread_p90=float(np.percentile(after, 90))))
        print(json.dumps(out[-1]), flush=True)
    return out


def timed(fn, stream, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps               # ms per call


def gpu_part(a, rec):
    import torch
    from pvnet_amd import extend_utils as X
    if not torch.cuda.is_available():
        raise RuntimeError("the timing and the census need the GPU (no CPU path); --no-gpu runs the CPU part alone")
    dev = torch.device("cuda:0")
    rec["device"] = torch.cuda.get_device_name(dev)
    stream = torch.cuda.Stream(dev)
    K = torch.from_numpy(K_LM).to(dev)

    def paths(p2, p3):
        w = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64, device=dev).repeat(p2.shape[0], p2.shape[1], 1)
        return dict(epnp=lambda: X.pnp_batch(p2, p3, K, method="epnp"),
                    epnp_lm=lambda: X.pnp_batch(p2, p3, K, method="epnp_lm"),
                    p3p_lm=lambda: X.uncertainty_pnp_batch(p2, w, p3, K, mode="weights"))

    rec["timing"] = []
    for pn in (9, 21):
        p3n, _, p2n = make_poses(a.b, pn, 1.0, False, seed=pn)
        p2, p3 = torch.from_numpy(p2n).to(dev), torch.from_numpy(p3n).to(dev)
        fns = paths(p2, p3)
        graphs, reps, ms = {}, {}, {k: [] for k in fns}
        with torch.cuda.stream(stream):
            for k, fn in fns.items():
                fn()                                  # warm-up: code objects, the unit weights
                stream.synchronize()
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k], stream=stream):
                    fn()
        for k in fns:
            t1 = timed(graphs[k].replay, stream, 3)
            reps[k] = max(3, int(math.ceil(a.window * 1e3 / t1)))
        for _ in range(a.rounds):                    # alternating, one process
            for k in fns:
                ms[k].append(timed(graphs[k].replay, stream, reps[k]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.ref_images):
            E.epnp(p3n, p2n[i], K_LM)
        t_np = (time.perf_counter() - t0) * 1e3 / a.ref_images
        r = dict(pn=pn, b=a.b, replays_per_window=reps, ms_per_batch={k: stats(v) for k, v in ms.items()},
                 numpy_ms_per_image=t_np, numpy_ms_batch_extrapolated=t_np * a.b)
        print(json.dumps(r), flush=True)
        rec["timing"].append(r)

    rec["census"] = []
    for pn in (9, 21):
        for name, noise, outlier in SETTINGS:
            p3n, Rt, p2n = make_poses(a.census, pn, noise, outlier, seed=1000 + pn, outlier_px=a.outlier)
            p2, p3 = torch.from_numpy(p2n).to(dev), torch.from_numpy(p3n).to(dev)
            row = dict(pn=pn, setting=name, poses=a.census, over_15_deg={}, median_deg={})
            for k, fn in paths(p2, p3).items():
                d = rot_deg(fn().cpu().numpy()[:, :, :3], Rt[:, :, :3])
                row["over_15_deg"][k] = int((d > 15.0).sum())
                row["median_deg"][k] = float(np.median(d))
            print(json.dumps(row), flush=True)
            rec["census"].append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of replays per timed window")
    ap.add_argument("--census", type=int, default=1000)
    ap.add_argument("--outlier", type=float, default=50.0, help="size of the gross outlier, px")
    ap.add_argument("--ref-images", type=int, default=64)
    ap.add_argument("--sign-poses", type=int, default=60)
    ap.add_argument("--no-gpu", action="store_true", help="only the CPU part (sign after the LM)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pnp_probe.json"))
    a = ap.parse_args()
    rec = dict(b=a.b, rounds=a.rounds, outlier_px=a.outlier)
    rec["sign_after_lm"] = sign_after_lm(a.sign_poses)
    if not a.no_gpu:
        gpu_part(a, rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
