#!/usr/bin/env python3
"""The BOP pose errors on the device against the way a user would write them today.

MSSD + MSPD: b poses (default 256) of one model of pn vertices (default 8,192) at ns = 1, 8 and 315
symmetries.  Per size, in one process and alternating round by round:

  fused: one ``sym_errors`` call (two launches), captured into a hipGraph and replayed between two
         device events, enough replays per window to fill --window seconds;
  torch: the same two errors written with torch in float64 on the same device -- the ground truth
         composed with every symmetry, both clouds transformed by batched matmul, the distances'
         ``amax`` over vertices and ``amin`` over symmetries -- in chunks of poses that keep the
         [poses, ns, pn, 3] intermediate at or under 256 MB;
  numpy: the same form on the host for one pose (once per size).

VSD: b poses at 480 x 640, each with its own sensor image.  The fused ``pv_bop_vsd`` (a memset and
two launches, captured) against the torch mask algebra on the same three maps in chunks of 32
poses; the two ``render_labels`` calls that make the maps are timed on their own.

Recorded: ms per call (median and range over the rounds, and the range over the median as the
spread), the operation and byte counts from the shapes, and the share of the bound that applies.
Operation counts are the algorithm's, a divide or a square root counted as one operation:
  MSSD  24 per (vertex, symmetry): 9 products and 9 sums of A p + c, 3 products and 2 sums, 1 maximum
  MSPD  34 per (vertex, symmetry): 18 of G p, 3 products, 3 sums and 2 divides of the projection,
        2 differences, 2 products, 1 sum, the test and the select, 1 maximum
  VSD   23 per pixel either map covers, 12 bytes per pixel
against the MI355X's 78.6 TFLOP/s fp64 vector rate counted as instructions (an FMA counts two FLOP, and
the definition allows none): 39.3e12 lane operations a second, and 8 TB/s of HBM.  The fp64 divide
and square root each expand to a dozen instructions, so the share of issue slots is higher than the
share quoted.  Needs the GPU; there is no fallback.

    python tools/bop_probe.py [--b 256] [--pn 8192] [--ns 1,8,315] [--rounds 5] [--out FILE]
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
from pvnet_amd import bop  # noqa: E402
from pvnet_amd.evaluation_utils import ModelTable  # noqa: E402
from pvnet_amd.synth import LINEMOD_K  # noqa: E402

OPS_MSSD, OPS_MSPD, OPS_VSD, BYTES_VSD = 24, 34, 23, 12
PEAK_F64_LANE_OPS = 78.6e12 / 2
PEAK_HBM = 8.0e12
CHUNK_BYTES = 256 << 20


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def make_poses(rng, b, z=(0.7, 1.1), off_deg=(0.5, 8.0), off_t=0.004):
    gt, est = np.zeros((b, 3, 4)), np.zeros((b, 3, 4))
    for i in range(b):
        R = rodrigues(rng.standard_normal(3), rng.uniform(0, np.pi))
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(*z)])
        gt[i] = np.concatenate([R, t[:, None]], 1)
        dR = rodrigues(rng.standard_normal(3), np.radians(rng.uniform(*off_deg)))
        est[i] = np.concatenate([dR @ R, (t + rng.standard_normal(3) * off_t)[:, None]], 1)
    return est, gt


def make_syms(ns):
    """ns = 315: BOP's discretisation of one continuous axis; otherwise ns turns about z."""
    if ns == 315:
        return bop.symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    return np.stack([np.concatenate([rodrigues([0, 0, 1], 2 * np.pi * k / ns), np.zeros((3, 1))], 1) for k in range(ns)])


def torch_sym(pts, Pe, Pg, S, K):
    """MSSD and MSPD as a user would write them: batched matmul, amax over vertices, amin over symmetries."""
    b, ns, pn = Pe.shape[0], S.shape[0], pts.shape[0]
    bc = max(1, CHUNK_BYTES // (ns * pn * 3 * 8))
    mssd = torch.empty(b, dtype=torch.float64, device=pts.device)
    mspd = torch.empty(b, dtype=torch.float64, device=pts.device)
    Kt = K.transpose(0, 1)
    for s in range(0, b, bc):
        pe, pg = Pe[s:s + bc], Pg[s:s + bc]
        RG = torch.matmul(pg[:, None, :, :3], S[None, :, :, :3])                       # [bc, ns, 3, 3]
        tG = torch.matmul(pg[:, None, :, :3], S[None, :, :, 3:]) + pg[:, None, :, 3:]  # [bc, ns, 3, 1]
        est = torch.matmul(pts, pe[:, :, :3].transpose(1, 2)) + pe[:, None, :, 3]       # [bc, pn, 3]
        gt = torch.matmul(pts, RG.transpose(2, 3)) + tG.transpose(2, 3)                 # [bc, ns, pn, 3]
        mssd[s:s + bc] = (est[:, None] - gt).norm(dim=-1).amax(-1).amin(-1)
        qe, qg = torch.matmul(est, Kt), torch.matmul(gt, Kt)
        ue, ug = qe[..., :2] / qe[..., 2:], qg[..., :2] / qg[..., 2:]
        mspd[s:s + bc] = (ue[:, None] - ug).norm(dim=-1).amax(-1).amin(-1)
    return mssd, mspd


def numpy_sym_one(pts, pe, pg, S, K):
    RG = pg[:, :3] @ S[:, :, :3]
    tG = S[:, :, 3] @ pg[:, :3].T + pg[:, 3]
    est = pts @ pe[:, :3].T + pe[:, 3]
    gt = pts @ RG.transpose(0, 2, 1) + tG[:, None]
    mssd = np.linalg.norm(est - gt, axis=-1).max(-1).min()
    qe, qg = est @ K.T, gt @ K.T
    mspd = np.linalg.norm(qe[:, :2] / qe[:, 2:] - qg[..., :2] / qg[..., 2:], axis=-1).max(-1).min()
    return mssd, mspd


def torch_vsd(dT, dE, dG, K, delta, taus, chunk=32):
    """The mask algebra of VSD on three depth maps, in float64, `chunk` poses at a time."""
    b, H, W = dE.shape
    dev = dE.device
    xs = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    ys = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    ax, ay = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
    r = torch.sqrt(ax * ax + ay * ay + 1.0)
    err = torch.empty_like(taus)
    for s in range(0, b, chunk):
        zt, ze, zg = dT[s:s + chunk], dE[s:s + chunk], dG[s:s + chunk]
        t_ok, e_ok, g_ok = (torch.isfinite(z) & (z > 0) for z in (zt, ze, zg))
        dt, de, dg = zt.double() * r, ze.double() * r, zg.double() * r
        vis_gt = g_ok & (~t_ok | (dg - dt <= delta))
        vis_est = e_ok & (~t_ok | (de - dt <= delta) | vis_gt)
        inter = vis_gt & vis_est
        un = (vis_gt | vis_est).sum((1, 2))
        ni = inter.sum((1, 2))
        diff = (dg - de).abs()
        tk = taus[s:s + chunk]
        ge = torch.stack([(inter & (diff >= tk[:, k, None, None])).sum((1, 2)) for k in range(tk.shape[1])], 1)
        e = (ge + (un - ni)[:, None]).double() / un[:, None].double()
        err[s:s + chunk] = torch.where(un[:, None] > 0, e, torch.ones_like(e))
    return err


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


def compare(fused, base, stream, rounds, window):
    """Capture `fused`, then time it and `base` alternately -> (fused stats, base stats, replays)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        fused()                                      # warm-up: workspace, code objects
        base()
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            fused()
    t1 = timed(g.replay, stream, 2)
    reps = max(2, int(math.ceil(window * 1e3 / t1)))
    tf, tb = [], []
    for _ in range(rounds):
        tf.append(timed(g.replay, stream, reps))
        tb.append(timed(base, stream, 1))
    torch.cuda.synchronize()
    return stats(tf), stats(tb), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--pn", type=int, default=8192)
    ap.add_argument("--ns", default="1,8,315")
    ap.add_argument("--hw", default="480,640")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of fused replays per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bop_probe.json"))
    a = ap.parse_args()
    nss = [int(s) for s in a.ns.split(",")]
    H, W = (int(v) for v in a.hw.split(","))
    rng = np.random.default_rng(0)
    pts = (rng.standard_normal((a.pn, 3)) * 0.03).astype(np.float32)
    est, gt = make_poses(rng, a.b)
    plan = {ns: dict(vertex_transforms=a.b * ns * a.pn, lane_ops=a.b * ns * a.pn * (OPS_MSSD + OPS_MSPD)) for ns in nss}
    print("plan:", json.dumps(plan), flush=True)

    if not torch.cuda.is_available():
        raise RuntimeError("bop_probe needs the GPU (no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    K = torch.from_numpy(LINEMOD_K).to(dev)
    rec = dict(device=torch.cuda.get_device_name(dev), b=a.b, pn=a.pn, rounds=a.rounds,
               ops_per_vertex_symmetry=dict(mssd=OPS_MSSD, mspd=OPS_MSPD), peak_f64_lane_ops_per_s=PEAK_F64_LANE_OPS,
               peak_hbm_bytes_per_s=PEAK_HBM, sym=[], vsd=None)
    table = ModelTable([(pts, 0.1, False)], dev)
    te, tg = torch.from_numpy(est).to(dev), torch.from_numpy(gt).to(dev)
    pts64 = table.points.double()
    for ns in nss:
        S = make_syms(ns)
        st = bop.SymmetryTable.from_arrays([S], dev)
        out = {"err": torch.empty((a.b, 2), dtype=torch.float64, device=dev),
               "best": torch.empty((a.b, 2), dtype=torch.int32, device=dev)}
        res = {}

        def fused():
            return bop.sym_errors(te, tg, table, st, K, None, out=out)

        def base():
            res["t"] = torch_sym(pts64, te, tg, st.syms, K)

        tf, tb, reps = compare(fused, base, stream, a.rounds, a.window)
        t0 = time.perf_counter()
        host = numpy_sym_one(pts.astype(np.float64), est[0], gt[0], S, LINEMOD_K)
        t_np = (time.perf_counter() - t0) * 1e3
        err = out["err"].cpu().numpy()
        ops = plan[ns]["lane_ops"]
        ms = tf["median"]
        r = dict(ns=ns, replays_per_window=reps, fused_ms=tf, torch_ms=tb, numpy_ms_one_pose=t_np,
                 numpy_ms_batch_extrapolated=t_np * a.b, vertex_transforms=plan[ns]["vertex_transforms"], lane_ops=ops,
                 share_of_fp64_vector_peak=ops / (ms * 1e-3) / PEAK_F64_LANE_OPS, bound="fp64 vector issue",
                 torch_over_fused=tb["median"] / ms, faster_by_more_than_the_spread=bool(tb["min"] > tf["max"]),
                 numpy_batch_over_fused=t_np * a.b / ms,
                 mssd_max_abs_diff_vs_torch=float((out["err"][:, 0] - res["t"][0]).abs().max()),
                 mspd_max_abs_diff_vs_torch=float((out["err"][:, 1] - res["t"][1]).abs().max()),
                 mssd_abs_diff_vs_numpy_pose0=float(abs(err[0, 0] - host[0])), mspd_abs_diff_vs_numpy_pose0=float(abs(err[0, 1] - host[1])))
        print(json.dumps(r), flush=True)
        rec["sym"].append(r)
        del st, out, res
        torch.cuda.empty_cache()

    # ---- VSD
    from pvnet_amd.render import MeshTable, render_labels
    from tests import render_ref as RR
    mesh = MeshTable([RR.bumpy_ellipsoid(level=4)], device=dev)          # 5,120 faces
    scale = W / 640.0
    Kv = torch.from_numpy(LINEMOD_K * np.array([[scale], [H / 480.0], [1.0]])).to(dev)
    ve, vg = make_poses(np.random.default_rng(1), a.b, z=(0.35, 0.6), off_deg=(0.5, 15.0), off_t=0.01)
    ve, vg = torch.from_numpy(ve).to(dev), torch.from_numpy(vg).to(dev)
    mid = torch.zeros((a.b, 1), dtype=torch.int32, device=dev)
    maps = {}

    def render(name, poses):
        def go():
            maps[name] = torch.cat([render_labels(mesh, poses[s:s + 64, None], mid[s:s + 64], None, Kv, H, W, want=("depth",))["depth"]
                                    for s in range(0, a.b, 64)])
        return go

    with torch.cuda.stream(stream):
        for name, poses in (("est", ve), ("gt", vg)):
            render(name, poses)()
        stream.synchronize()
    t_render = {name: stats([timed(render(name, poses), stream, 1) for _ in range(a.rounds)]) for name, poses in (("est", ve), ("gt", vg))}
    dE, dG = maps["est"], maps["gt"]
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=dev).manual_seed(2)
        sensor = torch.where(torch.isfinite(dG), dG + 0.002 * torch.randn(dG.shape, generator=gen, device=dev), torch.full_like(dG, 0.9))
        sensor[torch.rand(dG.shape, generator=gen, device=dev) < 0.1] = 0.0
        sensor[:, :, : W // 4] = 0.3
        taus = torch.tensor(bop.FRACTIONS, dtype=torch.float64, device=dev)[None, :].repeat(a.b, 1) * 0.12
        covered = int((torch.isfinite(dE) | torch.isfinite(dG)).sum())
        stream.synchronize()
    res = {}

    def fused_v():
        res["f"] = bop.vsd_maps(sensor, dE, dG, Kv, taus, 0.015)

    def base_v():
        res["t"] = torch_vsd(sensor, dE, dG, Kv, 0.015, taus)

    tf, tb, reps = compare(fused_v, base_v, stream, a.rounds, a.window)
    npix = a.b * H * W
    ms = tf["median"] * 1e-3
    t_hbm, t_ops = npix * BYTES_VSD / PEAK_HBM, covered * OPS_VSD / PEAK_F64_LANE_OPS
    rec["vsd"] = dict(H=H, W=W, ntau=taus.shape[1], faces=mesh.max_faces, replays_per_window=reps, fused_ms=tf, torch_ms=tb,
                      render_est_ms=t_render["est"], render_gt_ms=t_render["gt"], pixels=npix, covered_pixels=covered,
                      bytes=npix * BYTES_VSD, lane_ops=covered * OPS_VSD, least_ms_hbm=t_hbm * 1e3, least_ms_fp64=t_ops * 1e3,
                      bound="HBM" if t_hbm >= t_ops else "fp64 vector issue", share_of_bound=max(t_hbm, t_ops) / ms,
                      bytes_per_s=npix * BYTES_VSD / ms, torch_over_fused=tb["median"] / tf["median"],
                      faster_by_more_than_the_spread=bool(tb["min"] > tf["max"]),
                      err_max_abs_diff_vs_torch=float((res["f"]["err"] - res["t"]).abs().max()),
                      mean_err=float(res["f"]["err"].mean()))
    print(json.dumps(rec["vsd"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
