#!/usr/bin/env python3
"""The depth refinement on the device against the way a user would write it today.

b poses (default 256) of a mesh of 20,480 triangles at 480 x 640, each with its own sensor image (the
render at a ground truth a few millimetres and degrees away, 2 mm of noise, a tenth of the pixels
missing).  In one process, alternating round by round:

  fused: one ``pv_icp_iterate`` call (two launches) on maps rendered beforehand, captured into a
         hipGraph and replayed between two device events, enough replays per window to fill --window
         seconds; eps_rot = eps_trans = 0, so no pose converges and every block works every time;
  floor: the same call on 3 x 3 frames with min_count = 0: the two launches and k_solve's arithmetic with
         nothing to linearise.  fused - floor is charged to k_linearise together with k_solve's walk
         over the block partials (300 rows a pose at 480 x 640);
  torch: the same arithmetic as float64 torch ops on the same device, 32 poses at a time: the
         back-projection, the normals by slicing, the gates as masks, J^T J by einsum,
         ``torch.linalg.solve``, the Cayley update;
  numpy: tests/icp_ref.py on one pose (once).

and the chain a user calls: ``refine_depth`` with 8 rounds (render + iterate each), eager, and one
round of it; the renders are timed on their own.

Recorded: ms per call (median and range over the rounds), the bytes k_linearise has to move (4 per
pixel of the rendered map, 4 more per pixel it covers for the sensor's; the four neighbours come from
lines already fetched) and their share of 8 TB/s of HBM, and the agreement of the three.  Nothing here
has a target.  Needs the GPU; there is no fallback.

    python tools/icp_probe.py [--b 256] [--hw 480,640] [--rounds 5] [--out FILE]
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
from pvnet_amd import icp  # noqa: E402
from pvnet_amd.synth import LINEMOD_K  # noqa: E402

PEAK_HBM = 8.0e12
PAR = dict(icp.DEFAULTS, eps_rot=0.0, eps_trans=0.0)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def make_poses(rng, b, z=(0.35, 0.6), off_deg=(0.5, 3.0), off_t=0.004):
    gt, est = np.zeros((b, 3, 4)), np.zeros((b, 3, 4))
    for i in range(b):
        R = rodrigues(rng.standard_normal(3), rng.uniform(0, np.pi))
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(*z)])
        gt[i] = np.concatenate([R, t[:, None]], 1)
        dR = rodrigues(rng.standard_normal(3), np.radians(rng.uniform(*off_deg)))
        est[i] = np.concatenate([dR @ R, (t + rng.standard_normal(3) * off_t)[:, None]], 1)
    return est, gt


def torch_iterate(pose, ze, zt, K, p, chunk=32):
    """One step as a user would write it in float64 torch -> (new poses, cnt)."""
    b, H, W = ze.shape
    dev = ze.device
    xs = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    ys = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    ay = ((ys - K[1, 2]) / K[1, 1]).expand(H, W)
    ax = ((xs - K[0, 2]) - K[0, 1] * ay) / K[0, 0]
    out, cnts = torch.empty_like(pose), torch.empty(b, dtype=torch.int64, device=dev)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    for s in range(0, b, chunk):
        z, t = ze[s:s + chunk].double(), zt[s:s + chunk].double()
        P = torch.stack([z * ax, z * ay, z], -1)                                        # [c, H, W, 3]
        du = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
        dv = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
        m = torch.linalg.cross(du, dv)
        l2 = (m * m).sum(-1)
        n = m / l2.sqrt()[..., None]
        zc, tc, Pc = z[:, 1:-1, 1:-1], t[:, 1:-1, 1:-1], P[:, 1:-1, 1:-1]
        ok = torch.isfinite(zc) & (zc > 0) & torch.isfinite(tc) & (tc > 0) & torch.isfinite(l2) & (l2 > 0)
        for nb in (z[:, 1:-1, 2:], z[:, 1:-1, :-2], z[:, 2:, 1:-1], z[:, :-2, 1:-1]):
            ok &= torch.isfinite(nb) & (nb > 0) & ((nb - zc).abs() <= p["edge_max"])
        d = Pc - torch.stack([tc * ax[1:-1, 1:-1], tc * ay[1:-1, 1:-1], tc], -1)
        ok &= (d * d).sum(-1) <= p["dist_max"] ** 2
        J = torch.cat([torch.linalg.cross(Pc, n), n], -1)
        J = torch.where(ok[..., None], J, torch.zeros_like(J))
        e = torch.where(ok, (n * d).sum(-1), torch.zeros_like(zc))
        A = torch.einsum("bhwk,bhwl->bkl", J, J)
        g = torch.einsum("bhwk,bhw->bk", J, e)
        M = A + p["lam"] * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
        xi = -torch.linalg.solve_ex(M, g)[0]
        w, v = xi[:, :3], xi[:, 3:]
        rn, tn = w.norm(dim=1), v.norm(dim=1)
        k = torch.minimum(torch.ones_like(rn), torch.minimum(p["max_rot"] / rn, p["max_trans"] / tn))
        a = (k[:, None] * w) / 2
        q = (a * a).sum(1)[:, None, None]
        ax_ = torch.zeros((a.shape[0], 3, 3), dtype=torch.float64, device=dev)
        ax_[:, 0, 1], ax_[:, 0, 2], ax_[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
        ax_[:, 1, 2], ax_[:, 2, 0], ax_[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
        Cm = ((1 - q) * eye + 2 * a[:, :, None] * a[:, None, :] + 2 * ax_) / (1 + q)
        ps = pose[s:s + chunk]
        out[s:s + chunk, :, :3] = Cm @ ps[:, :, :3]
        out[s:s + chunk, :, 3] = (Cm @ ps[:, :, 3:])[..., 0] + k[:, None] * v
        cnts[s:s + chunk] = ok.sum((1, 2))
    return out, cnts


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
    med = float(np.median(xs))
    return dict(median=med, min=float(min(xs)), max=float(max(xs)), spread=float((max(xs) - min(xs)) / med))


def capture(fn, stream):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        fn()                                         # warm-up: workspace, code objects
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--hw", default="480,640")
    ap.add_argument("--level", type=int, default=5, help="subdivisions of the mesh: 20 * 4^level triangles")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of fused replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "icp_probe.json"))
    a = ap.parse_args()
    H, W = (int(v) for v in a.hw.split(","))
    if not torch.cuda.is_available():
        raise RuntimeError("icp_probe needs the GPU (no CPU path)")
    from pvnet_amd.render import MeshTable, render_labels
    from tests import icp_ref as R
    from tests import render_ref as RR
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    mesh = MeshTable([RR.bumpy_ellipsoid(level=a.level)], device=dev)
    Knp = LINEMOD_K * np.array([[W / 640.0], [H / 480.0], [1.0]])
    K = torch.from_numpy(Knp).to(dev)
    est, gt = make_poses(np.random.default_rng(1), a.b)
    te, tg = torch.from_numpy(est).to(dev), torch.from_numpy(gt).to(dev)
    mid = torch.zeros(a.b, dtype=torch.int32, device=dev)

    def render(poses):
        return torch.cat([render_labels(mesh, poses[s:s + 64, None], mid[s:s + 64, None], None, K, H, W, want=("depth",))["depth"]
                          for s in range(0, a.b, 64)])

    with torch.cuda.stream(stream):
        dG, dE = render(tg), render(te)
        gen = torch.Generator(device=dev).manual_seed(2)
        sensor = torch.where(torch.isfinite(dG), dG + 0.002 * torch.randn(dG.shape, generator=gen, device=dev), torch.full_like(dG, 0.9))
        sensor[torch.rand(dG.shape, generator=gen, device=dev) < 0.1] = 0.0
        sensor = sensor.contiguous()
        covered = int(torch.isfinite(dE).sum())
        stream.synchronize()
    t_render = stats([timed(lambda: render(te), stream, 1) for _ in range(a.rounds)])
    rec = dict(device=torch.cuda.get_device_name(dev), b=a.b, H=H, W=W, faces=mesh.max_faces, rounds=a.rounds,
               peak_hbm_bytes_per_s=PEAK_HBM, covered_pixels=covered, covered_share=covered / (a.b * H * W), render_ms=t_render)

    # ---- one call
    start = icp.new_state(te, neq=True)
    st = {k: v.clone() for k, v in start.items()}

    def reset():
        for k in st:
            st[k].copy_(start[k])

    def fused():
        icp.iterate(st, dE, sensor, K, None, **PAR)

    small = icp.new_state(te)
    tiny_e = dE[:, :3, :3].contiguous()
    tiny_t = sensor[:, :3, :3].contiguous()

    def floor():
        icp.iterate(small, tiny_e, tiny_t, K, None, **dict(PAR, min_count=0))

    res = {}

    def base():
        res["t"] = torch_iterate(start["pose"], dE, sensor, K, PAR)

    try:                                             # a torch build without a batched solver still leaves the rest
        with torch.cuda.stream(stream):
            base()
            stream.synchronize()
    except RuntimeError as e:
        res["error"] = str(e).splitlines()[0]

        def base():                                  # noqa: F811
            pass

    gf, gs = capture(fused, stream), capture(floor, stream)
    reps = max(2, int(math.ceil(a.window * 1e3 / timed(gf.replay, stream, 2))))
    tf, ts, tb = [], [], []
    for _ in range(a.rounds):
        tf.append(timed(gf.replay, stream, reps))
        ts.append(timed(gs.replay, stream, reps))
        tb.append(timed(base, stream, 1))
    with torch.cuda.stream(stream):
        reset()
        gf.replay()
        stream.synchronize()
    one = {k: v.cpu().numpy() for k, v in st.items()}
    t0 = time.perf_counter()
    ref = R.new_state(est[:1])
    R.iterate(ref, dE[:1].cpu().numpy(), sensor[:1].cpu().numpy(), Knp, **PAR)
    t_np = (time.perf_counter() - t0) * 1e3
    tf, ts, tb = stats(tf), stats(ts), stats(tb)
    lin_ms = tf["median"] - ts["median"]
    nbytes = a.b * H * W * 4 + covered * 4
    moved = one["status"] <= 1
    if "error" in res:
        agree = dict(torch_error=res["error"])
    else:
        tp, tc = res["t"][0].cpu().numpy(), res["t"][1].cpu().numpy()
        agree = dict(cnt_equal_torch=bool((one["cnt"] == tc).all()),
                     pose_max_abs_diff_vs_torch=float(np.abs(one["pose"][moved] - tp[moved]).max()))
    rec["iterate"] = dict(replays_per_window=reps, fused_ms=tf, floor_ms_3x3=ts, linearise_and_reduce_ms=lin_ms, torch_ms=tb,
                          numpy_ms_one_pose=t_np, numpy_ms_batch_extrapolated=t_np * a.b, bytes=nbytes,
                          linearise_bytes_per_s=nbytes / (lin_ms * 1e-3), linearise_share_of_hbm=nbytes / (lin_ms * 1e-3) / PEAK_HBM,
                          call_share_of_hbm=nbytes / (tf["median"] * 1e-3) / PEAK_HBM, torch_over_fused=tb["median"] / tf["median"],
                          faster_by_more_than_the_spread=bool(tb["min"] > tf["max"]), numpy_batch_over_fused=t_np * a.b / tf["median"],
                          status_counts=np.bincount(one["status"], minlength=5).tolist(),
                          **agree,
                          pose0_bits_equal_numpy=bool((one["pose"][0].view(np.uint64) == ref["pose"][0].view(np.uint64)).all()),
                          neq0_bits_equal_numpy=bool((one["neq"][0].view(np.uint64) == ref["neq"][0].view(np.uint64)).all()))
    print(json.dumps(rec["iterate"]), flush=True)

    # ---- the chain
    def add(P):
        d = P.cpu().numpy() - gt
        return float(np.median(np.abs(d[:, :, 3]).max(1)))

    chain = {}
    for iters in (1, 8):
        out = {}

        def go():
            out["r"] = icp.refine_depth(mesh, te, mid, sensor, K, iters=iters)

        with torch.cuda.stream(stream):
            go()
            stream.synchronize()
        chain[str(iters)] = dict(ms=stats([timed(go, stream, 1) for _ in range(a.rounds)]),
                                 status_counts=np.bincount(out["r"][1]["status"].cpu().numpy(), minlength=5).tolist(),
                                 median_translation_error=add(out["r"][0]))
    rec["chain"] = dict(start_median_translation_error=add(te), **chain)
    print(json.dumps(rec["chain"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
