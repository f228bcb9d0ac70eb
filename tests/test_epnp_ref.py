"""The numpy EPnP (tests/epnp_ref.py) pinned on the CPU, independently of the device:
exact data recovers the pose, two eigen solvers of different families give the same pose once
the control-axis sign is pinned (and do not when it is not), degenerate inputs and the
selection rule behave as include/pvpose.h states."""
import numpy as np
import pytest

from tests import epnp_ref as E
from tests.test_pnp_oracle import K_LM, K_SELF

PNS = (6, 7, 9, 21, 64)


def jacobi_eigh(A, sweeps=60):
    """A plain cyclic Jacobi eigen solver (Golub & Van Loan 8.5), of another family than LAPACK's
    tridiagonal QR -> (eigenvalues ascending, eigenvectors in columns)."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    V = np.eye(n)
    for _ in range(sweeps):
        off = np.sqrt((np.triu(A, 1) ** 2).sum())
        if off <= 1e-300 or off <= 1e-22 * np.sqrt((np.diag(A) ** 2).sum()):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if A[p, q] == 0.0:
                    continue
                th = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                t = (1.0 if th >= 0 else -1.0) / (abs(th) + np.sqrt(th * th + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                J = np.eye(n)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                A = J.T @ A @ J
                A[p, q] = A[q, p] = 0.0
                V = V @ J
    w = np.diag(A).copy()
    o = np.argsort(w, kind="stable")
    return w[o], V[:, o]


def models():
    """(name, points): the cuboid (9 points) and random points in an anisotropic box for every pn."""
    rng = np.random.default_rng(2024)
    out = [("cuboid9", E.cuboid_model())]
    for pn in PNS:
        out.append((f"random{pn}", E.random_model(rng, pn)))
    return out


MODELS = models()


def cases(noises, poses=3):
    """(model name, p3, K, true Rt, p2) over every model, both cameras and `poses` rotations up to 3 rad."""
    rng = np.random.default_rng(7)
    for name, p3 in MODELS:
        for K in (K_LM, K_SELF):
            for _ in range(poses):
                Rt = E.random_pose(rng, 3.0)
                p2 = E.project(Rt, p3, K)
                for noise in noises:
                    yield name, p3, K, Rt, p2 + noise * rng.standard_normal(p2.shape), noise


def test_models_have_distinct_pca_eigenvalues():
    assert sorted({m.shape[0] for _, m in MODELS}) == sorted(PNS)
    for name, p3 in MODELS:
        d = p3 - p3.mean(0)
        w = np.linalg.eigvalsh(d.T @ d)[::-1]
        assert w[0] - w[1] > 0.1 * w[0] and w[1] - w[2] > 0.1 * w[1], (name, w)
        assert w[2] > 1e-3 * w[0], (name, w)


def test_jacobi_eigh_is_an_eigen_solver():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((12, 12))
    A = B @ B.T
    w, V = jacobi_eigh(A)
    assert np.abs(w - np.linalg.eigvalsh(A)).max() < 1e-12 * w[-1]
    assert np.abs(A @ V - V * w).max() < 1e-12 * w[-1] and np.abs(V.T @ V - np.eye(12)).max() < 1e-13


def test_exact_projections_recover_the_pose():
    worst = worst32 = 0.0
    for name, p3, K, Rt, p2, _ in cases((0.0,), poses=4):
        r = E.epnp(p3, p2, K)
        assert r["status"] == E.OK, name
        worst = max(worst, np.abs(r["Rt"] - Rt).max())
        r32 = E.epnp(p3, p2.astype(np.float32).astype(np.float64), K)
        worst32 = max(worst32, np.abs(r32["Rt"] - Rt).max())
    print(f"exact f64 points: worst |Rt - truth| {worst:.2e}; f32-rounded points: {worst32:.2e}")
    assert worst < 1e-9
    assert worst32 < 1e-4


def test_rt6_is_the_rodrigues_vector_of_Rt():
    from oracle.pnp import rodrigues_vec_to_mat
    for name, p3, K, Rt, p2, _ in cases((1.0,), poses=1):
        r = E.epnp(p3, p2, K)
        assert np.abs(rodrigues_vec_to_mat(r["rt6"][:3]) - r["Rt"][:, :3]).max() < 1e-12
        np.testing.assert_array_equal(r["rt6"][3:], r["Rt"][:, 3])


def test_solver_independence_needs_the_sign_convention():
    """LAPACK and Jacobi agree to 1e-8 with the control-axis sign pinned; without it some case differs."""
    worst = worst_unpinned = 0.0
    for name, p3, K, Rt, p2, noise in cases((1.0, 3.0)):
        a = E.epnp(p3, p2, K)
        b = E.epnp(p3, p2, K, eigh=jacobi_eigh)
        assert a["status"] == b["status"] == E.OK
        worst = max(worst, np.abs(a["Rt"] - b["Rt"]).max())
        a0 = E.epnp(p3, p2, K, sign=0)
        b0 = E.epnp(p3, p2, K, eigh=jacobi_eigh, sign=0)
        worst_unpinned = max(worst_unpinned, np.abs(a0["Rt"] - b0["Rt"]).max())
    print(f"LAPACK vs Jacobi: pinned sign {worst:.2e}, unpinned {worst_unpinned:.2e}")
    assert worst < 1e-8
    assert worst_unpinned > 1e-5


def test_flipped_convention_is_another_pose_under_noise():
    """The sign is not cosmetic: the flipped convention moves the noisy pose, and not the exact one."""
    moved = 0.0
    for name, p3, K, Rt, p2, noise in cases((0.0, 3.0), poses=1):
        d = np.abs(E.epnp(p3, p2, K)["Rt"] - E.epnp(p3, p2, K, sign=-1)["Rt"]).max()
        if noise == 0.0:
            assert d < 1e-9
        else:
            moved = max(moved, d)
    assert moved > 1e-5


def test_degenerate_inputs_give_identity():
    rng = np.random.default_rng(5)
    p3 = E.cuboid_model()
    Rt = E.random_pose(rng)
    p2 = E.project(Rt, p3, K_LM)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    planar = p3.copy()
    planar[:, 2] = 0.01
    nan = p2.copy()
    nan[4, 1] = np.nan
    inf = p2.copy()
    inf[0, 0] = np.inf
    for what, (m, q) in dict(planar=(planar, p2), nan=(p3, nan), inf=(p3, inf), zeros=(p3, np.zeros_like(p2)),
                             coincident=(p3, np.full_like(p2, 17.5))).items():
        r = E.epnp(m, q, K_LM)
        assert r["status"] == E.DEGENERATE, what
        np.testing.assert_array_equal(r["Rt"], ident)
        np.testing.assert_array_equal(r["rt6"], np.zeros(6))
    assert E.epnp(p3, p2, K_LM)["status"] == E.OK


@pytest.mark.parametrize("errs,n", [
    ((1.0, 2.0, 3.0), 1), ((2.0, 1.0, 3.0), 2), ((3.0, 2.0, 1.0), 3), ((2.0, 3.0, 1.0), 3),
    ((1.0, 1.0, 1.0), 1),            # an exact tie keeps the lower N
    ((2.0, 1.0, 1.0), 2), ((1.0, 2.0, 1.0), 1), ((2.0, 2.0, 1.0), 3),
    ((3.0, 1.0, 2.0), 2),            # N = 3 is compared with the current best, not with N = 1
    ((np.nan, 1.0, 2.0), 1), ((1.0, np.nan, 0.5), 3), ((np.inf, np.inf, np.inf), 1), ((np.inf, 5.0, np.inf), 2),
])
def test_selection_rule(errs, n):
    assert E.select(np.array(errs)) == n
