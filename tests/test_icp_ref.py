"""tests/icp_ref.py, the numpy restatement of include/pvicp.h, against truth: analytic normals, a zero
step at the true pose, an orthogonal update, a solve that agrees with LAPACK, and convergence on
rendered scenes.  It also proves the cases of tests/icp_cases.py fair: every status value and every
rejection rule is reached, so the device tests that replay those cases exercise them too."""
import numpy as np
import pytest

from tests import icp_cases as C
from tests import icp_ref as R

U = 2.0 ** -53


@pytest.fixture(scope="module")
def replay():
    """name -> (case, final state, the first call's per-pose pixel_terms)."""
    out = {}
    for name, c in C.call_cases().items():
        detail = []
        out[name] = (c, C.run_ref(c, detail), detail)
    return out


def test_plane_normals_are_analytic():
    H, W, K = 24, 32, C.K_SKEW
    z, n = C.plane_depth(H, W, K, (0.3, -0.2, 1.0), 0.7)
    t = R.pixel_terms(z, z, K, 0.02, 0.05)
    assert t["used"][1:-1, 1:-1].all() and not t["used"][0].any() and not t["used"][:, 0].any()
    got = t["n"][1:-1, 1:-1]
    # chords of points on a plane lie in it, so the only error is the f32 rounding of the four depths:
    # each moves a chord's end by at most z 2^-24 along its ray, over a baseline of two pixels
    baseline = 2.0 * 0.6 / 310.0
    bound = 4.0 * 0.9 * 2.0 ** -24 / baseline
    assert np.abs(got - n).max() <= bound
    np.testing.assert_allclose((got * got).sum(-1), 1.0, rtol=0, atol=8 * U)
    assert np.all(t["e"] == 0.0)                                       # sensor == render: d is exactly 0


def test_sphere_normals_are_analytic():
    H, W, K = 48, 64, C.K_PLAIN
    z, n = C.sphere_depth(H, W, K, (0.002, -0.001, 0.7), 0.05)
    t = R.pixel_terms(z, z, K, 0.02, 0.004)
    used = t["used"]
    assert used.sum() > 600
    cosang = (t["n"][used] * n[used]).sum(-1)
    # a central difference on a sphere of radius r with a chord of h: the secant's direction is off by
    # O((h / r)^2); h is below two pixels' footprint on a surface steep enough to step edge_max = 4 mm
    h = np.hypot(2 * 0.7 / 300.0, 0.004)
    assert np.all(np.abs(cosang) >= 1.0 - (h / 0.05) ** 2)
    assert np.all(cosang < 0) or np.all(cosang > 0)                    # one orientation all over
    assert (t["why"] == R.REJECT.index("edge")).any()                  # the limb is cut by edge_max


def test_true_pose_gives_zero_gradient_and_zero_step():
    z = C.bumpy(24, 32)
    st = R.new_state([C.POSE0])
    R.iterate(st, z[None], z[None], C.K_SKEW, **C.BASE)
    assert st["cnt"][0] == 22 * 30
    assert np.all(st["neq"][0][21:] == 0.0) and np.all(st["neq"][0][[0, 6, 11, 15, 18, 20]] > 0.0)
    assert st["status"][0] == R.CONVERGED and st["iters"][0] == 1
    assert np.all(st["stats"][0] == 0.0)
    np.testing.assert_array_equal(st["pose"][0], C.POSE0)               # C is exactly the identity


def test_cayley_keeps_rotations_orthogonal():
    rng = np.random.default_rng(5)
    P = C.POSE0.copy()
    worst = 0.0
    for _ in range(64):
        w, v = rng.normal(size=3) * 0.1, rng.normal(size=3) * 0.01
        Cm = R.cayley(w, 0.7)
        assert np.abs(Cm.T @ Cm - np.eye(3)).max() < 8 * U
        assert abs(np.linalg.det(Cm) - 1.0) < 8 * U
        # the Cayley map of a is the rotation by 2 atan|a| about a
        a = 0.7 * w / 2
        ang = 2 * np.arctan(np.sqrt(a @ a))
        np.testing.assert_allclose(Cm, C.small_rotation(a, ang), rtol=0, atol=1e-15)
        P = R.apply_step(P, w, v, 0.7)
        worst = max(worst, np.abs(P[:, :3].T @ P[:, :3] - np.eye(3)).max())
    assert worst < 1e-12                                               # 64 steps of a few 2^-53 each
    np.testing.assert_array_equal(R.cayley(np.zeros(3)), np.eye(3))


def test_solve_agrees_with_lapack():
    rng = np.random.default_rng(11)
    for _ in range(32):
        J = rng.normal(size=(40, 6))
        A, g = J.T @ J, J.T @ rng.normal(size=40)
        assert np.linalg.cond(A) < 1e3
        neq = np.array([A[k, l] for k in range(6) for l in range(k, 6)] + list(g) + [1.0])
        ok, w, v, rn, tn, k = R.solve_step(neq, 0.0, np.inf, np.inf)
        want = -np.linalg.solve(A, g)
        assert ok and k == 1.0
        np.testing.assert_allclose(np.concatenate([w, v]), want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
        lam = 0.25
        ok, w, v, *_ = R.solve_step(neq, lam, np.inf, np.inf)
        want = -np.linalg.solve(A + lam * np.diag(np.diag(A)), g)
        np.testing.assert_allclose(np.concatenate([w, v]), want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    bad = np.zeros(28)
    assert R.solve_step(bad, 1.0, 1.0, 1.0)[0] is False
    neq = np.array([1.0 if k == l else 0.0 for k in range(6) for l in range(k, 6)] + [np.inf] * 6 + [1.0])
    assert R.solve_step(neq, 0.0, 1.0, 1.0)[0] is False                # a non-finite step


def test_ordered_sums_is_a_sum_and_has_the_header_order():
    rng = np.random.default_rng(13)
    T = rng.normal(size=(25, 41, 28))
    got = R.ordered_sums(T)
    np.testing.assert_allclose(got, T.reshape(-1, 28).sum(0), rtol=1e-12)
    # integers sum exactly in any order; powers of two spread over 60 binades do not: lane 0's run first
    T = np.zeros((1, 8, 28))
    T[0, :5, 0] = [2.0 ** 60, 1.0, -2.0 ** 60, 1.0, 1.0]
    # lane 0: ((2^60 + 1) - 2^60) + 1 = 1 (the first 1 is absorbed); lane 1: 1; the tree adds them
    assert R.ordered_sums(T)[0] == 2.0


def test_step_limit_rules(replay):
    free = replay["limit_none"][1]["stats"][0]
    rn, tn = free[1], free[2]
    P0 = C.POSE0
    for name, (mr, mt) in dict(limit_none=(1.0, 1.0), limit_rot=(1e-2, 1.0), limit_trans=(1.0, 1e-3),
                               limit_both_rot_wins=(1e-3, 1e-2), limit_both_trans_wins=(4e-2, 1e-3)).items():
        c, st, _ = replay[name]
        assert (c["params"]["max_rot"], c["params"]["max_trans"]) == (mr, mt)
        np.testing.assert_array_equal(st["stats"][0], free)            # the stats are the free step's
        k = min(1.0, mr / rn if rn > mr else 1.0, mt / tn if tn > mt else 1.0)
        moved = st["pose"][0][:, 3] - P0[:, 3]
        ang = np.arccos(np.clip((np.trace(st["pose"][0][:, :3]) - 1) / 2, -1, 1))
        # the rotation applied is 2 atan(k rn / 2), the translation C t + k v with |C t - t| <= 0.7 angle
        np.testing.assert_allclose(ang, 2 * np.arctan(k * rn / 2), rtol=1e-6)
        assert abs(np.sqrt(moved @ moved) - k * tn) <= 0.7 * ang + 1e-12
    assert rn > 4e-2 and tn > 1e-2                                     # every limit above was below the free step
    assert (1e-3 / rn) < (1e-2 / tn) and (1e-3 / tn) < (4e-2 / rn)     # "rot wins" and "trans wins" say what they do


def test_cases_reach_every_status_and_every_rejection(replay):
    statuses, reasons = set(), set()
    for name, (c, st, detail) in replay.items():
        statuses |= set(int(s) for s in st["status"])
        for d in detail:
            if d is not None:
                reasons |= set(int(w) for w in np.unique(d["why"]))
    assert statuses == {R.RUNNING, R.CONVERGED, R.FEW, R.NOT_PD, R.BAD_INPUT}
    assert reasons == set(range(len(R.REJECT)))
    s = lambda n: replay[n][1]                                         # noqa: E731
    assert s("frame_3x3")["cnt"][0] == 1 and s("frame_5x7")["cnt"][0] == 15
    assert s("frame_1x1")["status"][0] == R.FEW and s("frame_2x9")["status"][0] == R.NOT_PD
    for n, px in (("block_plus_pixel", 1025), ("block_plus_row", 1024 + 64)):
        c = replay[n][0]
        assert c["depth_est"][0].size == px and replay[n][2][0]["used"][-2, -2]   # the last interior pixel is used
    assert replay["block_plus_pixel"][0]["depth_est"].shape[2] % R.RUN != 0
    assert s("no_rendered_pixel")["status"][0] == R.FEW and s("no_rendered_pixel_min0")["status"][0] == R.NOT_PD
    for n, why in (("no_rendered_pixel", "ze"), ("all_rejected_by_dist", "dist"), ("all_rejected_by_edge", "edge"),
                   ("all_rejected_by_l2", "l2")):
        w = replay[n][2][0]["why"][1:-1, 1:-1]
        assert s(n)["cnt"][0] == 0 and np.all(w == R.REJECT.index(why)), n
    a, bq = s("cnt_equals_min_count"), s("cnt_below_min_count")
    assert a["cnt"][0] == replay["cnt_equals_min_count"][0]["params"]["min_count"] and a["status"][0] == R.RUNNING
    assert bq["cnt"][0] == replay["cnt_below_min_count"][0]["params"]["min_count"] - 1 and bq["status"][0] == R.FEW
    assert np.isfinite(bq["stats"][0][0]) and np.isnan(bq["stats"][0][1:]).all()
    np.testing.assert_array_equal(bq["pose"][0], C.POSE0)
    # the rank-deficient plane: three exactly zero columns, so no damping relative to the diagonal helps
    for n in ("plane_lambda_0", "plane_lambda_pos"):
        assert s(n)["status"][0] == R.NOT_PD and s(n)["iters"][0] == 0
        assert np.all(s(n)["neq"][0][[11, 15, 18]] == 0.0)
        np.testing.assert_array_equal(s(n)["pose"][0], C.POSE0)
    assert s("tilted_plane_lambda_pos")["status"][0] == R.RUNNING
    A = R.unpack(s("tilted_plane_lambda_pos")["neq"][0])[0]
    assert np.linalg.matrix_rank(A, tol=1e-9 * np.abs(A).max()) == 3
    # converged on call 1, untouched by call 2 although call 2's maps differ; its neighbour went on
    c, st, _ = replay["converged_then_untouched"]
    assert st["status"].tolist() == [R.CONVERGED, R.RUNNING] and st["iters"].tolist() == [1, 2]
    one = R.iterate(R.new_state(c["poses"]), c["depth_est"], c["depth_test"], c["K"], c["img_id"], **c["params"])
    for k in ("pose", "stats", "neq", "cnt"):
        np.testing.assert_array_equal(st[k][0], one[k][0])
        assert not np.array_equal(st[k][1], one[k][1]) or k == "cnt"
    # bad input: which pose, and why
    c, st, _ = replay["mixed_batch"]
    assert st["status"].tolist() == [0, 4, 4, 4, 4, 0, 4, 0]
    assert np.isnan(c["poses"][1]).any() and np.isnan(c["K"][2, 0, 1]) and c["img_id"][3] == 3 and c["K"][4, 0, 0] == 0 and \
        c["img_id"][6] == -1 and np.isnan(c["K"][5, 2, 2])
    bad = st["status"] == R.BAD_INPUT
    assert np.isnan(st["stats"][bad]).all() and np.isnan(st["neq"][bad]).all() and (st["cnt"][bad] == 0).all()
    np.testing.assert_array_equal(st["pose"][bad], c["poses"][bad])
    assert (st["iters"][bad] == 0).all() and (st["iters"][~bad] == 1).all()
    c, st, _ = replay["mixed_batch_2"]
    assert st["status"].tolist() == [4, 4, 4, 0, 4, 0, 0, 4] and c["K"][0, 1, 1] == 0 and np.isinf(c["K"][1, 1, 2]) and \
        np.isinf(c["poses"][7]).any()
    assert replay["img_id_null_short"][1]["status"].tolist() == [0, 0, 4]
    # the sensor's missing values: 0, negative, +inf, -inf and NaN are all in the maps and all rejected by "zt"
    dt = replay["mixed_batch"][0]["depth_test"]
    assert (dt == 0).any() and (dt < 0).any() and np.isposinf(dt).any() and np.isneginf(dt).any() and np.isnan(dt).any()
    d0 = replay["mixed_batch"][2][0]
    zt_rej = d0["why"] == R.REJECT.index("zt")
    assert zt_rej.sum() >= 20 and not (np.isfinite(dt[2][zt_rej]) & (dt[2][zt_rej] > 0)).any()
    # shared and per-pose K differ in the result unless the matrices are equal
    assert not np.array_equal(s("shared_K_no_img_id")["neq"][2], s("per_pose_K_no_img_id")["neq"][2])
    np.testing.assert_array_equal(s("shared_K_no_img_id")["neq"][0], s("per_pose_K_no_img_id")["neq"][0])


@pytest.mark.parametrize("which", [0, 1], ids=["icosphere", "box"])
@pytest.mark.parametrize("kind", ["clean", "occluder", "missing"])
def test_convergence_on_rendered_scenes(which, kind):
    s = C.convergence_scene(which, occluder=kind == "occluder", missing=0.3 if kind == "missing" else 0.0)
    verts = s["models"][which][0]
    start = C.add_metric(verts, s["start"], s["gt"])
    assert 0.004 < start < 0.007                                       # 5 mm and 2 degrees on a 5 cm object
    detail = []
    st = R.new_state([s["start"]])
    H, W = s["depth"].shape[1:]
    for it in range(10):
        de = R.render_depth(s["models"], s["model_id"], st["pose"], s["K"], H, W)
        R.iterate(st, de, s["depth"], s["K"], detail=detail if it == 0 else None)
    ratio = C.add_metric(verts, st["pose"][0], s["gt"]) / start
    print(f"{'icosphere' if which == 0 else 'box'} {kind}: ADD {start * 1e3:.3f} mm -> ratio {ratio:.2e}, "
          f"status {st['status'][0]}, iters {st['iters'][0]}, cnt {st['cnt'][0]}")
    assert ratio < 0.1
    assert st["status"][0] in (R.RUNNING, R.CONVERGED) and st["iters"][0] >= 3
    why = detail[0]["why"]
    if kind == "occluder":
        assert (why == R.REJECT.index("dist")).sum() > 50              # the occluder's pixels, rejected by dist_max
    if kind == "missing":
        assert (why == R.REJECT.index("zt")).sum() > 200
        assert (s["depth"] == 0).mean() > 0.3
