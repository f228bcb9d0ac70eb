"""Scenes for pv_epnp's edge states (include/pvpose.h), TEST INFRASTRUCTURE ONLY: shared by
tests/test_epnp_cases.py (the scenes are what they say), tests/test_epnp_core_host.py (the host
form on them) and tests/test_gpu_epnp_edges.py (the device).  Everything comes from SEED.

Families (``FAMILIES``; DESIGN 10c lists what each is for):

* ``rep/<model>/<placement>``: models with repeated PCA eigenvalues.  Models: a regular octahedron
  (6 points, all three eigenvalues equal), cube corners (8), cube / square plate / square rod as
  corners + centre (9), icosahedron (12).  Placements: ``axis`` (axis-aligned, dyadic coordinates),
  ``exact`` (the (3/5, 4/5) rotation about x after the one about z, and a dyadic shift: every
  coordinate, deviation, product and sum of step 1 is exact in fp64, so the covariance has the same
  bits in any summation order and on any machine), ``generic`` (a random rotation and shift per
  image).  The regular icosahedron's coordinates are irrational; ``axis`` and ``exact`` use the
  vertices (0, +-8, +-13) and their cyclic shifts (13 / 8 for the golden ratio), which keep the
  symmetry that makes the covariance a multiple of I, with integers.
* ``thin/<model>/<r>``: ``random_model(21)`` and ``cuboid_model`` squeezed along the smallest PCA
  axis to the eigenvalue ratio r (``THIN_OK`` above the band pvpose.h step 9 describes,
  ``THIN_FLAT`` below it; nothing in between).
* ``depth/<t_z>``, ``offaxis`` (also as f32 keypoints: ``offaxis32``), ``theta/<k>``.
* ``branch/rank``: scenes searched for step 7's rank gate with another candidate left to win (see
  ``RANK_SCENES``); the other decisions of steps 5 and 7 fire in the families above.

``family(name)`` -> dict(p3: n arrays [pn, 3] (pn may differ between the images), K [n, 3, 3],
Rt [n, 3, 4], p2: n arrays [pn, 2] (f64 or f32), noise [n]); ``batches()`` -> one mixed batch per
(pn, keypoint type) with ``rows[name]`` giving each family's rows.  The arrays are shared and
read-only.  The gates and the assertions both test files make are at the end (``check_family``).
"""
import functools

import numpy as np

from oracle.pnp import rodrigues_vec_to_mat
from tests import epnp_ref as E
from tests.test_pnp_oracle import K_LM

SEED = 20240611
N_FAMILY, N_RMS = 24, 60          # images per family and noise level; per rms-gated set
THIN_OK, THIN_FLAT = (1e-4, 1e-6, 1e-8), (1e-11, 1e-13)
DEPTHS = (0.15, 3.0, 10.0)
THETAS = (0.0, 1e-12, 1e-7, np.pi - 1e-6, np.pi - 1e-9, np.pi)
OFFAXIS_T = ((0.6, -0.45, 0.8), (0.9, -0.65, 0.72))      # keypoints about 500 and 800 px from the principal point
REP_NOISES = (0.0, 1.0, 3.0)
PLACEMENTS = ("axis", "exact", "generic")

# ---------------------------------------------------------------- models with repeated eigenvalues
_BOX = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]


def _box_int(h, centre):
    pts = [(sx * h[0], sy * h[1], sz * h[2]) for sx, sy, sz in _BOX]
    return np.array(pts + ([(0, 0, 0)] if centre else []), np.int64)


def _cyclic_int(p, q):
    """(0, +-p, +-q) and its cyclic shifts: 12 points whose covariance is 4 (p^2 + q^2) I for any p, q."""
    base = [(0, sp * p, sq * q) for sp in (-1, 1) for sq in (-1, 1)]
    return np.array([tuple(np.roll(b, k)) for k in range(3) for b in base], np.int64)


# name -> (integer coordinates, log2 of the unit, (number of equal largest, of equal smallest) eigenvalues)
REP_MODELS = {
    "octa6": (np.array([(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3)], np.int64), -10, 3),
    "cube8": (_box_int((2, 2, 2), False), -10, 3),
    "cube9": (_box_int((2, 2, 2), True), -10, 3),
    "plate9": (_box_int((3, 3, 1), True), -10, 2),       # the two largest are equal
    "rod9": (_box_int((3, 1, 1), True), -10, -2),        # the two smallest are equal
    "icosa12": (_cyclic_int(8, 13), -13, 3),
}
R_EXACT_25 = np.array([[5, 0, 0], [0, 3, -4], [0, 4, 3]], np.int64) @ np.array([[3, -4, 0], [4, 3, 0], [0, 0, 5]], np.int64)
SHIFT_INT = np.array([40, -24, 56], np.int64)           # in units of 2^-10


def rep_model_int(model, placement):
    """-> (integer coordinates [pn, 3], unit) of the ``axis`` and ``exact`` placements: the model is
    25 m in ``axis`` and (R_EXACT_25 m + shift) in ``exact``, each times the unit."""
    m, lg, _ = REP_MODELS[model]
    if placement == "axis":
        return 25 * m, 2.0 ** lg
    assert placement == "exact"
    return m @ R_EXACT_25.T + SHIFT_INT * 2 ** (-10 - lg), 2.0 ** lg


def _regular(model):
    """The model in float coordinates for the generic placement (the icosahedron is the regular one)."""
    if model == "icosa12":
        g = (1.0 + np.sqrt(5.0)) / 2.0
        base = [(0.0, sp, sq * g) for sp in (-1, 1) for sq in (-1, 1)]
        return 0.045 * np.array([tuple(np.roll(b, k)) for k in range(3) for b in base])
    m, lg, _ = REP_MODELS[model]
    return 25.0 * m * 2.0 ** lg


def random_rotation(rng):
    ax = rng.standard_normal(3)
    return rodrigues_vec_to_mat(ax / np.linalg.norm(ax) * rng.uniform(0.0, np.pi))


# ---------------------------------------------------------------- thin models
def squeeze(p3, r):
    """p3 scaled along its smallest PCA axis so that smallest / largest PCA eigenvalue becomes r."""
    c = p3.mean(0)
    d = p3 - c
    w, U = np.linalg.eigh(d.T @ d)
    y = d @ U
    y[:, 0] *= np.sqrt(r * w[2] / w[0])
    return c + y @ U.T


def eigen_ratio(p3):
    """Smallest / largest PCA eigenvalue, from the singular values of the centred points (the
    covariance's eigenvalues lose the small one to rounding below about 1e-13)."""
    s = np.linalg.svd(p3 - p3.mean(0), compute_uv=False)
    return float((s[-1] / s[0]) ** 2)


# ---------------------------------------------------------------- families
def _camera(rng):
    K = K_LM * np.array([[1 + 0.1 * rng.uniform(-1, 1)], [1 + 0.1 * rng.uniform(-1, 1)], [1.0]])
    K[0, 2] += rng.uniform(-20, 20)
    K[1, 2] += rng.uniform(-20, 20)
    return K


def _pose(R, t):
    return np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1)


def _separated_model(rng, i):
    """pn 6 / 9 / 21 in turn: random points, the cuboid, random points."""
    return (E.random_model(rng, 6), E.cuboid_model(), E.random_model(rng, 21))[i % 3]


def _names():
    names = [f"rep/{m}/{p}" for m in REP_MODELS for p in PLACEMENTS]
    names += [f"thin/{m}/{r:g}" for m in ("random21", "cuboid9") for r in THIN_OK + THIN_FLAT]
    names += [f"depth/{d:g}" for d in DEPTHS] + ["offaxis", "offaxis32"] + [f"theta/{k}" for k in range(len(THETAS))]
    return names


FAMILIES = tuple(_names())
BRANCH_FAMILIES = ("branch/rank",)
ALL_FAMILIES = FAMILIES + BRANCH_FAMILIES


def _finish(rng, models, poses, noises, f32=False):
    """Cameras, projections and noise for per-image models and poses, frozen."""
    n = len(models)
    K = np.stack([_camera(rng) for _ in range(n)])
    Rt = np.stack(poses)
    noise = np.asarray(noises, np.float64)
    p3 = tuple(np.array(m, np.float64) for m in models)
    p2 = tuple(E.project(Rt[i], p3[i], K[i]) + noise[i] * rng.standard_normal((p3[i].shape[0], 2)) for i in range(n))
    if f32:
        p2 = tuple(q.astype(np.float32) for q in p2)
    out = dict(p3=p3, K=K, Rt=Rt, p2=p2, noise=noise)
    for a in (K, Rt, noise) + p3 + p2:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "branch/rank":
        return _rank_family()
    rng = np.random.default_rng([SEED, FAMILIES.index(name)])
    kind, *arg = name.split("/")
    models, poses, noises = [], [], []
    if kind == "rep":
        model, placement = arg
        for noise in REP_NOISES:
            for _ in range(N_RMS if noise > 0.0 else N_FAMILY):
                if placement == "generic":
                    p3 = _regular(model) @ random_rotation(rng).T + rng.uniform(-0.05, 0.05, 3)
                else:
                    q, unit = rep_model_int(model, placement)
                    p3 = q * unit
                models.append(p3)
                poses.append(E.random_pose(rng, 3.0))
                noises.append(noise)
        return _finish(rng, models, poses, noises)
    if kind == "thin":
        r = float(arg[1])
        for noise in (0.0, 1.0):
            for _ in range(N_FAMILY):
                models.append(squeeze(E.random_model(rng, 21) if arg[0] == "random21" else E.cuboid_model(), r))
                poses.append(E.random_pose(rng, 3.0))
                noises.append(noise)
        return _finish(rng, models, poses, noises)
    for noise in (0.0, 1.0):
        for i in range(N_FAMILY):
            models.append(_separated_model(rng, i))
            pose = E.random_pose(rng, 3.0)
            if kind == "depth":
                tz = float(arg[0])
                pose = _pose(pose[:, :3], [rng.uniform(-0.1, 0.1) * tz, rng.uniform(-0.1, 0.1) * tz, tz])
            elif kind.startswith("offaxis"):
                pose = _pose(pose[:, :3], np.array(OFFAXIS_T[i % 2]) + rng.uniform(-0.03, 0.03, 3))
            else:
                ax = rng.standard_normal(3)
                pose = _pose(rodrigues_vec_to_mat(ax / np.linalg.norm(ax) * THETAS[int(arg[0])]), pose[:, 3])
            poses.append(pose)
            noises.append(noise)
    return _finish(rng, models, poses, noises, f32=kind == "offaxis32")


def image(name, i):
    f = family(name)
    return f["p3"][i], f["p2"][i], f["K"][i], f["Rt"][i], float(f["noise"][i])


def is_repeated(name):
    return name.startswith("rep/")


def thin_ratio(name):
    return float(name.split("/")[2]) if name.startswith("thin/") else None


# ---------------------------------------------------------------- branch scenes
BRANCHES = ("x0_neg", "x2_zero", "x1_neg", "negated", "det_flip", "rank_reject")
MARGIN = 1e-6          # a decision counts when its deciding quantity is this far (relative) from its threshold
_MARGIN_OF = dict(x0_neg="x0_margin", x2_zero="x2_margin", x1_neg="x1_margin", negated="z0_margin",
                  det_flip="det_margin", rank_reject="rank_margin")


def fired(trace, margin=MARGIN):
    """The branches of one image's trace (epnp_ref.epnp) that fired in some start or candidate with
    the deciding quantity at least `margin` from its threshold."""
    out = set()
    for rec in trace["starts"] + trace["cands"]:
        for b in BRANCHES:
            if rec.get(b) and rec[_MARGIN_OF[b]] >= margin:
                out.add(b)
    return out


# The step-7 rank gate with another candidate left to win.  On exact data a model in or below the
# thin band loses all three candidates (they all are the true, flat cloud); under 1 px of noise none
# is flat.  In between, at 0.003 to 0.3 px on a model of ratio 1e-11 or 3e-12, about one image in 400 has
# one or two candidates flat and a finite winner.  RANK_SCENES are the indices k, out of the first
# 20,000 of rank_scene's stream, where the reference does that with the smallest singular value at
# least 1e-3 (relative) from the gate; tests/test_epnp_cases.py holds them to it.
RANK_SCENES = (1686, 2898, 3151, 4260, 4443, 5044, 5762, 6790, 7002, 9302, 10061, 10078, 12180, 12258, 12989, 13356, 15245,
               15695, 16742, 19079, 19471)


def rank_scene(k):
    """Image k of the stream RANK_SCENES was searched in -> (p3, p2, K, Rt, noise in px)."""
    rng = np.random.default_rng([SEED, 1000, k])
    p3 = squeeze(E.random_model(rng, 21) if k % 2 else E.cuboid_model(), (1e-11, 3e-12)[(k // 2) % 2])
    Rt, K = E.random_pose(rng, 3.0), _camera(rng)
    noise = 10.0 ** rng.uniform(-2.5, -0.5)
    return p3, E.project(Rt, p3, K) + noise * rng.standard_normal((p3.shape[0], 2)), K, Rt, noise


def _rank_family():
    sc = [rank_scene(k) for k in RANK_SCENES]
    out = dict(p3=tuple(s[0] for s in sc), K=np.stack([s[2] for s in sc]), Rt=np.stack([s[3] for s in sc]),
               p2=tuple(s[1] for s in sc), noise=np.array([s[4] for s in sc]))
    for a in (out["K"], out["Rt"], out["noise"]) + out["p3"] + out["p2"]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def traces(name):
    """(reference result, trace) of every image of a family."""
    f = family(name)
    out = []
    for i in range(len(f["p3"])):
        t = {}
        out.append((E.epnp(f["p3"][i], f["p2"][i].astype(np.float64), f["K"][i], trace=t), t))
    return out


# ---------------------------------------------------------------- batches
@functools.lru_cache(maxsize=None)
def batches():
    """One batch per (pn, keypoint type): {(pn, "f64" | "f32"): dict(p3, K, Rt, p2, noise, rows)},
    the families interleaved image by image (so that neighbours are of other families), with
    rows[name] the rows of each family in its own order."""
    groups = {}
    for name in ALL_FAMILIES:
        f = family(name)
        for i in range(len(f["p3"])):
            key = (f["p3"][i].shape[0], "f32" if f["p2"][i].dtype == np.float32 else "f64")
            groups.setdefault(key, {}).setdefault(name, []).append(i)
    out = {}
    for key, fam in sorted(groups.items()):
        order = sorted(((j, name, i) for name, idx in fam.items() for j, i in enumerate(idx)),
                       key=lambda t: (t[0], ALL_FAMILIES.index(t[1])))
        bt = {k: np.stack([family(name)[k][i] for _, name, i in order]) for k in ("p3", "K", "Rt", "p2", "noise")}
        rows = {}
        for row, (_, name, i) in enumerate(order):
            rows.setdefault(name, []).append((i, row))
        bt["rows"] = {name: (np.array([i for i, _ in v]), np.array([r for _, r in v])) for name, v in rows.items()}
        for k in ("p3", "K", "Rt", "p2", "noise"):
            bt[k].setflags(write=False)
        out[key] = bt
    return out




# ---------------------------------------------------------------- gates
TOL = 1e-7             # device or host form against the reference, device against host form (test_gpu_epnp.py)
TOL_EXACT = 1e-9       # exact f64 projections against the true pose
TOL_EXACT_F32 = 1e-4   # keypoints rounded to f32 (test_gpu_epnp.py)
RMS_FACTOR = 1.25      # repeated eigenvalues under noise: rms error to truth against the reference's
D_FACTOR = 100.0
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def uses_d_rule(name):
    """Families whose conditioning puts the reference's own resolution above TOL: 10 m of depth, the
    models at or below the thin band under noise, and the rank-gate scenes (which are such models)."""
    r = thin_ratio(name)
    return name == "depth/10" or name.startswith("branch/") or (r is not None and r <= max(THIN_FLAT))


def diff(a, b):
    """max |a - b| where +inf equals +inf and NaN equals NaN, and a finite value is never equal to
    either (np.abs(a - b) alone turns inf - inf into NaN)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all="ignore"):
        d = np.where(same, 0.0, np.abs(a - b))
    return float(np.where(np.isnan(d), np.inf, d).max())


def pose_diff(a, b):
    """Rt, cand_err and rt6 (the rotation vector is ill-conditioned near pi: compared as a matrix)
    of two results."""
    return max(diff(a["Rt"], b["Rt"]), diff(a["cand_err"], b["cand_err"]),
               diff(rodrigues_vec_to_mat(a["rt6"][:3]), rodrigues_vec_to_mat(b["rt6"][:3])),
               diff(a["rt6"][3:], b["rt6"][3:]))


@functools.lru_cache(maxsize=None)
def resolution(name):
    """d [n]: per image, the disagreement of the two CPU restatements test_epnp_ref.py pairs (the
    reference through LAPACK's eigh and through a plain Jacobi solver): the reference's own
    resolution at that image's conditioning.  Only computed for the families of uses_d_rule."""
    from tests.test_epnp_ref import jacobi_eigh
    f = family(name)
    return np.array([pose_diff(r, E.epnp(f["p3"][i], f["p2"][i].astype(np.float64), f["K"][i], eigh=jacobi_eigh))
                     for i, (r, _) in enumerate(traces(name))])


def gates(name):
    """The per-image bound on |got - reference|: TOL, or max(TOL, 100 d) in the families of uses_d_rule."""
    n = len(family(name)["p3"])
    return np.maximum(TOL, D_FACTOR * resolution(name)) if uses_d_rule(name) else np.full(n, TOL)


def check_family(name, got, compared=None):
    """Everything tests/test_epnp_core_host.py and tests/test_gpu_epnp_edges.py assert about one
    family's results `got` (a list of dicts Rt, rt6, cand_err, n_used, status, one per image) against
    the truth and the reference.  `compared` (a Counter) counts the images whose n_used was compared,
    by winner.  Returns the measured figures."""
    f, ref = family(name), traces(name)
    n = len(f["p3"])
    assert len(got) == n
    r_thin = thin_ratio(name)
    gate = None if is_repeated(name) else gates(name)
    out = dict(truth=0.0) if is_repeated(name) else dict(truth=0.0, ref=0.0, ref_over_gate=0.0)
    err = {}
    for i in range(n):
        g, (r, _) = got[i], ref[i]
        noise, f32 = float(f["noise"][i]), f["p2"][i].dtype == np.float32
        assert g["status"] == r["status"], (name, i)
        if r_thin is not None and r_thin <= max(THIN_FLAT) and noise == 0.0:
            assert r["status"] == E.DEGENERATE, (name, i)
        elif r_thin is None or r_thin >= min(THIN_OK):
            assert r["status"] == E.OK, (name, i)
        if g["status"] == E.DEGENERATE:
            np.testing.assert_array_equal(g["Rt"], IDENT)
            np.testing.assert_array_equal(g["rt6"], np.zeros(6))
            np.testing.assert_array_equal(r["Rt"], IDENT)
            continue
        assert 1 <= g["n_used"] <= 3
        if noise == 0.0:
            e = diff(g["Rt"], f["Rt"][i])
            out["truth"] = max(out["truth"], e)
            assert e < (TOL_EXACT_F32 if f32 else TOL_EXACT), (name, i, e)
        if is_repeated(name):
            if noise > 0.0:
                err.setdefault(noise, []).append((diff(g["Rt"], f["Rt"][i]), diff(r["Rt"], f["Rt"][i])))
        else:
            e = pose_diff(g, r)
            out["ref"], out["ref_over_gate"] = max(out["ref"], e), max(out["ref_over_gate"], e / gate[i])
            assert e < gate[i], (name, i, e, gate[i])
            s = np.sort(r["cand_err"])
            if s[1] - s[0] > max(1e-9 * s[1], gate[i]):        # the rule of tests/test_gpu_epnp.py
                assert g["n_used"] == r["n_used"], (name, i, r["cand_err"], g["cand_err"])
                if compared is not None:
                    compared[r["n_used"]] += 1
        if name.startswith("theta/"):
            rv = float(np.linalg.norm(g["rt6"][:3]))
            assert np.isfinite(g["rt6"]).all() and rv <= np.pi + 1e-9, (name, i, rv)
            if THETAS[int(name.split("/")[1])] == 0.0 and noise == 0.0:
                assert rv < 1e-7, (name, i, rv)
    for noise, e in sorted(err.items()):
        e = np.array(e)
        assert e.shape[0] == N_RMS
        got_rms, ref_rms = np.sqrt((e ** 2).mean(0))
        out[f"rms_ratio_{noise:g}px"] = float(got_rms / ref_rms)
        assert got_rms <= RMS_FACTOR * ref_rms, (name, noise, got_rms, ref_rms)
    if gate is not None and uses_d_rule(name):
        out["d"] = float(resolution(name).max())
    return out


def check_against_host(name, got, hosted):
    """The device's results against the host form's, image by image: within TOL, the same status and
    the same winner.  Returns the worst difference."""
    worst = 0.0
    for i, (g, h) in enumerate(zip(got, hosted)):
        assert g["status"] == h["status"] and g["n_used"] == h["n_used"], (name, i, g["cand_err"], h["cand_err"])
        worst = max(worst, pose_diff(g, h))
        assert worst < TOL, (name, i, worst)
    return worst
