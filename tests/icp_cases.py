"""The scenes tests/test_icp_ref.py (CPU) and tests/test_gpu_icp.py (device) share.  The CPU file shows
on tests/icp_ref.py that every case reaches the state its name promises; the device file then holds
the device to the reference on the same cases, bit for bit.

A *call case* feeds ``pv_icp_iterate`` directly: its "rendered" maps are analytic surfaces, since the
entry never looks at the pose while it linearises.  A *scene* goes through the renderer."""
import numpy as np

from tests import icp_ref as R
from tests import render_ref as RR

K_SKEW = np.array([[310.0, 0.6, 31.4], [0.0, 305.0, 23.7], [0.0, 0.0, 1.0]])
K_PLAIN = np.array([[300.0, 0.0, 32.0], [0.0, 300.0, 24.0], [0.0, 0.0, 1.0]])
BASE = dict(dist_max=0.02, edge_max=0.01, lam=1e-6, min_count=6, max_rot=0.2, max_trans=0.05, eps_rot=1e-7, eps_trans=1e-7)
POSE0 = RR.pose(np.eye(3), [0.0, 0.0, 0.7])


def rays(H, W, K):
    """ax, ay f64 [H, W] of pvicp.h rule 1."""
    y, x = np.mgrid[:H, :W].astype(np.float64)
    ay = (y - K[1, 2]) / K[1, 1]
    ax = ((x - K[0, 2]) - K[0, 1] * ay) / K[0, 0]
    return ax, ay


def plane_depth(H, W, K, normal, d):
    """The depth map of the plane normal . X = d, and the unit normal."""
    n = np.asarray(normal, np.float64)
    n = n / np.sqrt(n @ n)
    ax, ay = rays(H, W, K)
    return (d / (n[0] * ax + n[1] * ay + n[2])).astype(np.float32), n


def sphere_depth(H, W, K, centre, radius):
    """The near intersection of each pixel's ray with a sphere (+inf where it misses), and the outward
    unit normals f64 [H, W, 3]."""
    ax, ay = rays(H, W, K)
    D = np.stack([ax, ay, np.ones_like(ax)], -1)
    c = np.asarray(centre, np.float64)
    a, bq = (D * D).sum(-1), D @ c
    disc = bq * bq - a * (c @ c - radius * radius)
    with np.errstate(invalid="ignore"):
        z = (bq - np.sqrt(disc)) / a
    hit = disc > 0
    n = (D * np.where(hit, z, 0.0)[..., None] - c) / radius
    return np.where(hit, z, np.inf).astype(np.float32), n


def bumpy(H, W, shift=0.0, tilt=0.0, disc=None, z0=0.7):
    """A smooth surface with normals in every direction (full-rank normal equations) -> f32 [H, W];
    outside the disc (cx, cy, r) it is background."""
    y, x = np.mgrid[:H, :W].astype(np.float64)
    u, v = (x - W / 2) / max(W, 4), (y - H / 2) / max(H, 4)
    z = z0 + shift + tilt * u + 0.02 * (u * u - 0.7 * v * v + 0.8 * u * v) + 0.004 * np.sin(5 * u + 1) * np.cos(4 * v) + 0.01 * v ** 3
    if disc is not None:
        z = np.where((x - disc[0]) ** 2 + (y - disc[1]) ** 2 < disc[2] ** 2, z, np.inf)
    return z.astype(np.float32)


def case(name, de, dt, K=K_SKEW, img_id=None, poses=None, calls=1, second=None, **kw):
    de, dt = np.asarray(de, np.float32), np.asarray(dt, np.float32)
    de = de[None] if de.ndim == 2 else de
    dt = dt[None] if dt.ndim == 2 else dt
    b = len(de)
    poses = np.stack([POSE0] * b) if poses is None else np.asarray(poses, np.float64)
    return dict(name=name, depth_est=de, depth_test=dt, K=np.asarray(K, np.float64), img_id=None if img_id is None
                else np.asarray(img_id, np.int32), poses=poses, calls=calls, second=second, params={**BASE, **kw})


def run_ref(c, detail=None):
    """The reference's state after the case's calls.  A second call sees `second` as its rendered maps
    when the case has one (a converged pose must not notice)."""
    st = R.new_state(c["poses"])
    for k in range(c["calls"]):
        de = c["second"] if (k > 0 and c["second"] is not None) else c["depth_est"]
        R.iterate(st, de, c["depth_test"], c["K"], c["img_id"], detail=detail if k == 0 else None, **c["params"])
    return st


def call_cases():
    """name -> case.  Kept small: at most 48 x 64 but for the block-boundary shapes, which are the
    smallest that cross the boundary."""
    rng = np.random.default_rng(7)
    out = []
    full = lambda H, W, **kw: bumpy(H, W, **kw)                                      # noqa: E731
    # frames: 3x3 has one interior pixel, 5x7 fifteen; the object touches all four borders in both
    out.append(case("frame_3x3", full(3, 3), full(3, 3, shift=0.002), min_count=1))
    out.append(case("frame_5x7", full(5, 7), full(5, 7, shift=0.002), min_count=1))
    out.append(case("frame_1x1", full(1, 1), full(1, 1), min_count=1))
    out.append(case("frame_2x9", full(2, 9), full(2, 9), min_count=0))
    # 25 x 41 = 1025: one pixel more than a block; 41 is no multiple of the lane run of 4
    out.append(case("block_plus_pixel", full(25, 41), full(25, 41, shift=0.003, tilt=0.004)))
    # 17 x 64 = 1024 + one row
    out.append(case("block_plus_row", full(17, 64), full(17, 64, shift=-0.002, tilt=-0.003)))
    # 3 blocks, an object in the middle, a W of 4 k + 1
    out.append(case("three_blocks", bumpy(48, 61, disc=(30, 22, 17)), full(48, 61, shift=0.002, tilt=0.002)))
    out.append(case("no_rendered_pixel", np.full((12, 16), np.inf), full(12, 16)))
    out.append(case("no_rendered_pixel_min0", np.full((12, 16), np.inf), full(12, 16), min_count=0))
    out.append(case("all_rejected_by_dist", full(12, 16), full(12, 16, shift=0.05)))
    out.append(case("all_rejected_by_edge", full(12, 16) + (np.arange(16) % 2 * 0.05).astype(np.float32), full(12, 16)))
    # a camera so long that du x dv underflows to exactly 0: every pixel is rejected by l2
    K_far = np.array([[1e300, 0.0, 8.0], [0.0, 1e300, 6.0], [0.0, 0.0, 1.0]])
    out.append(case("all_rejected_by_l2", np.full((12, 16), 0.7), np.full((12, 16), 0.7), K=K_far))
    # cnt == min_count and min_count - 1: the disc's used pixels are counted by the reference first
    de, dt = bumpy(20, 24, disc=(12, 10, 6.5)), full(20, 24, shift=0.001)
    n = int(R.pixel_terms(de[...], dt, K_SKEW, BASE["dist_max"], BASE["edge_max"])["used"].sum())
    out.append(case("cnt_equals_min_count", de, dt, min_count=n))
    out.append(case("cnt_below_min_count", de, dt, min_count=n + 1))
    # rank-deficient: a fronto-parallel plane under a camera without skew has three exactly zero columns
    flat = np.full((16, 20), 0.7, np.float32)
    out.append(case("plane_lambda_0", flat, flat + np.float32(0.002), K=K_PLAIN, lam=0.0))
    out.append(case("plane_lambda_pos", flat, flat + np.float32(0.002), K=K_PLAIN, lam=1e-3))
    tilted = plane_depth(16, 20, K_SKEW, (0.2, -0.3, 1.0), 0.7)[0]
    out.append(case("tilted_plane_lambda_0", tilted, tilted + np.float32(0.002), lam=0.0))
    out.append(case("tilted_plane_lambda_pos", tilted, tilted + np.float32(0.002), lam=1e-3))
    # the step limiter: the sensor is 8 mm behind and tilted; the free step is about 0.08 rad and 0.056
    out.append(case("limit_none", de := full(40, 56), dt := full(40, 56, shift=0.008, tilt=0.01), max_rot=1.0, max_trans=1.0))
    out.append(case("limit_rot", de, dt, max_rot=1e-2, max_trans=1.0))
    out.append(case("limit_trans", de, dt, max_rot=1.0, max_trans=1e-3))
    out.append(case("limit_both_rot_wins", de, dt, max_rot=1e-3, max_trans=1e-2))
    out.append(case("limit_both_trans_wins", de, dt, max_rot=4e-2, max_trans=1e-3))
    # converged on call 1 (sensor == render: e is exactly 0), untouched by call 2, which sees other maps
    same = full(24, 32)
    out.append(case("converged_then_untouched", np.stack([same, same]), np.stack([same, full(24, 32, shift=0.004)]),
                    calls=2, second=np.stack([full(24, 32, shift=0.01), full(24, 32, shift=0.001)])))
    out.append(case("two_calls_running", full(24, 32), full(24, 32, shift=0.004), calls=2))
    # bad input, per-pose K, img_id, and the sensor's missing values
    H, W, b = 25, 41, 8
    de = np.stack([bumpy(H, W, shift=0.001 * i, disc=(20 + i, 12, 9 + i % 3)) for i in range(b)])
    dt = np.stack([full(H, W, shift=0.002 + 0.001 * j, tilt=0.002 * j) for j in range(3)])
    hole = rng.random(dt.shape)
    dt[hole < 0.05] = 0.0
    dt[(hole >= 0.05) & (hole < 0.10)] = -0.7
    dt[(hole >= 0.10) & (hole < 0.15)] = np.inf
    dt[(hole >= 0.15) & (hole < 0.20)] = np.nan
    dt[(hole >= 0.20) & (hole < 0.22)] = -np.inf
    Ks = np.stack([K_SKEW + np.diag([i, 2.0 * i, 0.0]) for i in range(b)])
    poses = np.stack([RR.pose(RR.random_rotation(rng), [0.01 * i, -0.01, 0.7]) for i in range(b)])
    img_id = np.array([2, 0, 1, 3, 2, 1, -1, 2], np.int32)                      # pose 3 and pose 6: outside [0, 3)
    poses[1, 2, 1] = np.nan
    Ks[2, 0, 1] = np.nan                                                        # the skew
    Ks[4, 0, 0] = 0.0                                                           # fx
    Ks[5, 2, 2] = np.nan                                                        # K22 is not read: pose 5 is good
    out.append(case("mixed_batch", de, dt, K=Ks, img_id=img_id, poses=poses))
    Kf = Ks.copy()
    Kf[0, 1, 1] = 0.0                                                           # fy
    Kf[1, 1, 2] = np.inf                                                        # cy
    Pf = poses.copy()
    Pf[1] = poses[0]
    Pf[7, 0, 3] = -np.inf
    out.append(case("mixed_batch_2", de, dt, K=Kf, img_id=np.array([0, 1, 2, 2, 2, 2, 2, 2], np.int32), poses=Pf))
    # shared K with img_id NULL: pose i reads image i
    out.append(case("shared_K_no_img_id", de[:3], dt, K=K_SKEW, poses=poses[[0, 3, 7]]))
    out.append(case("per_pose_K_no_img_id", de[:3], dt, K=Ks[[0, 3, 7]], poses=poses[[0, 3, 7]]))
    # fewer images than poses with img_id NULL: the last pose has no image
    out.append(case("img_id_null_short", de[:3], dt[:2], K=K_SKEW, poses=poses[[0, 3, 7]]))
    return {c["name"]: c for c in out}


# ---------------------------------------------------------------- scenes through the renderer
def scene_models():
    return [RR.icosphere(2, 0.05), RR.box(0.05, 0.04, 0.03)]


def small_rotation(axis, angle):
    """Rodrigues' rotation, for the tests' perturbations (the code under test uses no sin or cos)."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt(a @ a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def perturb(P, axis, angle, dt):
    """Rotate the object by `angle` about `axis` through its own origin and move it by dt."""
    R_ = small_rotation(axis, angle) @ P[:, :3]
    return RR.pose(R_, P[:, 3] + np.asarray(dt, np.float64))


def add_metric(verts, Pa, Pb):
    v = np.asarray(verts, np.float64)
    da = v @ Pa[:, :3].T + Pa[:, 3]
    db = v @ Pb[:, :3].T + Pb[:, 3]
    return float(np.sqrt(((da - db) ** 2).sum(1)).mean())


def convergence_scene(which, H=48, W=64, occluder=False, missing=0.0, seed=3):
    """One object at 0.7 m seen so that three faces of the box show; the sensor map is the render at the
    true pose (noise-free), optionally with a nearer occluding plane over its left part and with a
    fraction of pixels missing.  The start is 5 mm and 2 degrees off.
    -> dict(models, model_id, K, gt, start, depth f32 [1, H, W])."""
    rng = np.random.default_rng(seed)
    models = scene_models()
    Rg = small_rotation((1.0, 0.3, 0.2), 0.9) @ small_rotation((0.0, 1.0, 0.1), 0.7)
    gt = RR.pose(Rg, [0.004, -0.003, 0.7])
    K = K_PLAIN
    depth = R.render_depth(models, [which], [gt], K, H, W)
    depth = np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)        # a sensor reports 0 for "nothing"
    if occluder:
        depth[:, :, : W // 2 - 6] = 0.55
    if missing > 0:
        depth[rng.random(depth.shape) < missing] = 0.0
    t = np.array([0.003, -0.002, 0.00346])                                      # |t| = 5 mm
    start = perturb(gt, (0.5, 1.0, -0.4), np.deg2rad(2.0), t)
    return dict(models=models, model_id=np.array([which], np.int32), K=K, gt=gt, start=start, depth=depth)
