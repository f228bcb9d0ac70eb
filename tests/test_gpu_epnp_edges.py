"""pv_epnp on the device over the edge families of tests/epnp_cases.py (tests/test_epnp_cases.py
proves on the CPU that they are what they say): models with repeated PCA eigenvalues, thin models on
both sides of the band pvpose.h step 9 describes, depth, off-axis and f32 keypoints, rotations at 0
and pi, and the scenes where step 7's rank gate rejects a candidate and another wins.

Three references.  The truth, on exact projections.  tests/epnp_ref.py, image by image, wherever the
PCA eigenvalues are separated (C.check_family, the assertions of tests/test_epnp_core_host.py).  And
the host form of the kernel's own header (tests/epnp_host.cpp), image by image in every family: with
repeated eigenvalues the control axes are the 3x3 Jacobi solver's, the reference's are LAPACK's, and
under noise the two poses differ by up to 0.3, so the host form is the only per-image check there
is; the reference enters those families through the rms gate.

Each batch (one per pn and keypoint type, the families mixed) is two launches, made once."""
import collections

import numpy as np
import pytest
import torch

from oracle import pnp as O
from tests import epnp_cases as C
from tests import epnp_ref as E
from tests.test_epnp_core_host import build_host_form
from tests.test_gpu_epnp import bits, device_rt6, run_device
from tests.test_pnp_oracle import K_LM

pytestmark = pytest.mark.gpu

REP = [n for n in C.ALL_FAMILIES if C.is_repeated(n)]
LM_PER_FAMILY = 5


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_form(tmp_path_factory.mktemp("epnp_host_edges"))


def _as_batch(bt, rows=slice(None)):
    return dict(p3=np.array(bt["p3"][rows]), K=np.array(bt["K"][rows]), p2=np.array(bt["p2"][rows]), per_image=True)   # copies: the shared arrays are read-only


def _launch(bt, device):
    """pnp_batch(diag=...) and pv_epnp with rt6 -> one dict per image; the two Rt are the same bits."""
    Rt, dg = run_device(bt, bt["p2"], device)
    Rt2, rt6 = device_rt6(bt, bt["p2"], device)
    np.testing.assert_array_equal(bits(Rt), bits(Rt2))
    return [dict(Rt=Rt[i], rt6=rt6[i], cand_err=dg["cand_err"][i], n_used=int(dg["n_used"][i]), status=int(dg["status"][i]))
            for i in range(Rt.shape[0])]


@pytest.fixture(scope="module")
def results(device):
    """{family: the device's result of every image, in the family's order}, from the mixed batches."""
    out = {}
    for bt in C.batches().values():
        got = _launch(_as_batch(bt), device)
        for name, (idx, row) in bt["rows"].items():
            for i, r in zip(idx, row):
                out.setdefault(name, {})[int(i)] = got[r]
    return {name: [v[i] for i in range(len(v))] for name, v in out.items()}


@pytest.fixture(scope="module")
def hosted(host):
    def of(name, cache={}):
        if name not in cache:
            f = C.family(name)
            cache[name] = [host(f["p3"][i], f["p2"][i], f["K"][i]) for i in range(len(f["p3"]))]
        return cache[name]
    return of


@pytest.mark.parametrize("name", C.ALL_FAMILIES)
def test_device_on_the_edge_families(name, results):
    """The assertions of tests/test_epnp_core_host.py::test_host_form_on_the_edge_families, on the
    device (f32 keypoints: the reference gets the same f32 values)."""
    assert len(results[name]) == len(C.family(name)["p3"])
    m = C.check_family(name, results[name])
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" if "ratio" not in k else f"{k} {v:.3f}" for k, v in m.items()))


@pytest.mark.parametrize("name", C.ALL_FAMILIES)
def test_device_matches_the_host_form(name, results, hosted):
    """Every image of every family, the repeated-eigenvalue ones included: Rt, rt6 as a matrix and
    cand_err within TOL of the host form, the same status and the same winner.  The two run the same
    operations without contraction; no placement is exempt."""
    worst = C.check_against_host(name, results[name], hosted(name))
    print(f"{name}: worst device vs host form {worst:.2e}")


def test_n_used_comparisons_are_not_empty(results):
    count = collections.Counter()
    inf_and_winner = 0
    for name in C.ALL_FAMILIES:
        if C.is_repeated(name):
            continue
        gate = C.gates(name)
        for i, (r, _) in enumerate(C.traces(name)):
            s = np.sort(r["cand_err"])
            if r["status"] == E.OK and s[1] - s[0] > max(1e-9 * s[1], gate[i]):
                assert results[name][i]["n_used"] == r["n_used"]
                count[r["n_used"]] += 1
                if np.isinf(r["cand_err"]).any():
                    np.testing.assert_array_equal(np.isinf(results[name][i]["cand_err"]), np.isinf(r["cand_err"]))
                    inf_and_winner += 1
    print(f"n_used compared: N=1 {count[1]}, N=2 {count[2]}, N=3 {count[3]}; with a candidate at +inf {inf_and_winner}")
    assert min(count[1], count[2], count[3]) >= 3 and inf_and_winner >= 3


def test_a_family_alone_has_the_bits_of_its_rows_in_the_mix(results, device):
    """Neighbours: the images of one family, launched alone, against their rows of the mixed batch."""
    for key, name in (((9, "f64"), "rep/rod9/exact"), ((21, "f64"), "thin/random21/1e-11"), ((21, "f32"), "offaxis32")):
        bt = C.batches()[key]
        idx, row = bt["rows"][name]
        alone = _launch(_as_batch(bt, row), device)
        for i, a in zip(idx, alone):
            m = results[name][int(i)]
            for k in ("Rt", "rt6", "cand_err"):
                np.testing.assert_array_equal(bits(np.asarray(a[k])), bits(np.asarray(m[k])))
            assert a["status"] == m["status"] and a["n_used"] == m["n_used"]


def test_epnp_lm_on_repeated_eigenvalues(device, hosted):
    """EPnP -> Levenberg-Marquardt on the device against the host form's rt6 -> oracle.pnp.ceres_lm,
    on the first 1 px images of every repeated-eigenvalue family.  The oracle starts from the host
    form and not from the reference: the reference's start (another basis of the eigenspace) ends up
    to 3e-4 away, which is the LM's stop threshold and no property of the device.  The stability
    filter and the tolerance are test_gpu_epnp.py::test_epnp_lm_matches_the_cpu_chain's."""
    p3, p2, K, want, stable = [], [], [], [], []
    for name in REP:
        f = C.family(name)
        for i in np.flatnonzero(f["noise"] == 1.0)[:LM_PER_FAMILY]:
            h = hosted(name)[i]
            assert h["status"] == E.OK
            w = np.tile(np.array([1.0, 0.0, 1.0]), (f["p3"][i].shape[0], 1))
            x = O.ceres_lm(h["rt6"], f["p2"][i], f["p3"][i], w, f["K"][i])
            x2 = O.ceres_lm(h["rt6"] + 1e-9 * np.array([1, -1, 1, -1, 1, -1.0]), f["p2"][i], f["p3"][i], w, f["K"][i])
            stable.append(bool(np.abs(x - x2).max() < 1e-8))
            want.append(np.concatenate([O.rodrigues_vec_to_mat(x[:3]), x[3:, None]], 1))
            p3.append(f["p3"][i])
            p2.append(f["p2"][i])
            K.append(f["K"][i])
    assert sum(stable) >= len(stable) - len(stable) // 10, stable
    worst, at = 0.0, 0
    for pn in sorted({p.shape[0] for p in p3}):
        sel = [j for j, p in enumerate(p3) if p.shape[0] == pn]
        bt = dict(p3=np.stack([p3[j] for j in sel]), K=np.stack([K[j] for j in sel]), p2=np.stack([p2[j] for j in sel]),
                  per_image=True)
        Rt, dg = run_device(bt, bt["p2"], device, "epnp_lm")
        assert (dg["status"] == E.OK).all() and (dg["iterations"] >= 0).all() and np.isfinite(dg["cost"]).all()
        for k, j in enumerate(sel):
            if stable[j]:
                at += 1
                worst = max(worst, np.abs(Rt[k] - want[j]).max())
    print(f"epnp_lm vs host form -> ceres_lm: worst {worst:.2e} over {at} stable images of {len(stable)}")
    assert worst < C.TOL


def _box_mesh(lo, hi):
    v = np.array([[(hi if c & 4 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 1 else lo)[2]] for c in range(8)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


@pytest.mark.parametrize("method", ["epnp", "epnp_lm"])
def test_closed_loop_on_a_cube_and_a_square_box(method, device):
    """The keypoints the product builds for a cube and a box with a square section (models.corners_3d
    and the box centre: repeated PCA eigenvalues), projections of random poses, Evaluator.evaluate:
    a hit in all three recorders for every pose, the pose within 1e-6 of the truth."""
    from pvnet_amd import models
    from pvnet_amd.evaluation_utils import Evaluator, ModelTable
    from pvnet_amd.render import MeshTable
    mesh = MeshTable([_box_mesh((-0.046875, -0.046875, -0.046875), (0.046875, 0.046875, 0.046875)),
                      _box_mesh((-0.03125, -0.03125, -0.078125), (0.03125, 0.03125, 0.078125))], device=device)
    ext = models.extent(mesh)
    kp = torch.cat([models.corners_3d(mesh), ((ext["bbox_min"] + ext["bbox_max"]) * 0.5)[:, None]], 1)
    kp_h = kp.cpu().numpy()
    assert kp_h.shape == (2, 9, 3)
    for m, mult in ((0, 3), (1, -2)):
        d = kp_h[m] - kp_h[m].mean(0)
        w = np.linalg.eigvalsh(d.T @ d)[::-1]
        assert (w[0] - w[2] if mult == 3 else w[1] - w[2]) <= 1e-12 * w[0]
    rng = np.random.default_rng(17)
    b = 24
    mid = rng.integers(0, 2, b)
    Rt = np.stack([E.random_pose(rng, 3.0) for _ in range(b)])
    p2 = np.stack([E.project(Rt[i], kp_h[mid[i]], K_LM) for i in range(b)])
    ev = Evaluator(ModelTable.from_meshes(mesh), kp)
    pose = ev.evaluate(torch.from_numpy(p2).to(device), torch.from_numpy(Rt).to(device), mid, K_LM, method=method)
    assert float((pose - torch.from_numpy(Rt).to(device)).abs().max()) < 1e-6
    assert ev.average_precision() == (1.0, 1.0, 1.0)
