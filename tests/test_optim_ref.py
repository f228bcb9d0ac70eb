"""tests/optim_ref.py, the numpy restatement of include/pvoptim.h, against independent yardsticks (CPU only):
torch.optim.Adam / AdamW / SGD in f64, torch._amp_update_scale_ and torch.nn.utils.clip_grad_norm_."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

SHAPES = [(3,), (17,), (4, 5), (R.CHUNK + 9,), (1,)]
STEPS = 20
# Measured with these inputs (20 steps, 5 tensors, lr 1e-2, weight decay 0 and 0.01), as
# max |a - b| / max |b| over all parameters after each step, the largest over steps, algorithms and decays:
#   the restatement run in f64 against f64 torch        F64_SEEN
#   the f32 restatement against the f64 restatement     F32_SEEN
# The f32 gate is twice the second figure.
F64_SEEN = 4.38e-16
F32_SEEN = 2.97e-7
F64_GATE = 1e-12
F32_GATE = 2 * F32_SEEN


def _inputs():
    rng = np.random.default_rng(7)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    grads = [[(rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32) for s in SHAPES] for _ in range(STEPS)]
    return p0, grads


def _torch_run(alg, wd, p0, grads, lr=1e-2, momentum=0.9):
    ps = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    if alg == R.ADAM:
        opt = torch.optim.Adam(ps, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    elif alg == R.ADAMW:
        opt = torch.optim.AdamW(ps, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    else:
        opt = torch.optim.SGD(ps, lr=lr, momentum=momentum, weight_decay=wd)
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        out.append([p.detach().numpy().copy() for p in ps])
    return out


def _ref_run(alg, wd, p0, grads, dtype, lr=1e-2, momentum=0.9):
    F = dtype
    ts = [dict(master=p.astype(F).reshape(-1), model=None, grad=np.zeros(p.size, F), m=np.zeros(p.size, F), v=np.zeros(p.size, F))
          for p in p0]
    d = R.desc(alg, weight_decay=wd, momentum=momentum, growth_interval=0, zero_grads=1)
    S = R.state(lr=lr, scale=1.0)
    if F is np.float64:
        S["lr"] = np.float64(lr)
    out = []
    for gs in grads:
        for t, g in zip(ts, gs):
            t["grad"][...] = g.reshape(-1)
        rec = R.step(d, ts, S, dtype)
        assert rec["k"] == 1 and not rec["skipped"] and all(not t["grad"].any() for t in ts)
        out.append([t["master"].astype(np.float64).reshape(s) for t, s in zip(ts, SHAPES)])
    assert S["step"] == len(grads)
    return out


def _dev(a, b):
    return max(max(float(np.abs(x - y).max()) for x, y in zip(sa, sb)) / max(float(np.abs(y).max()) for y in sb)
               for sa, sb in zip(a, b))


@pytest.fixture(scope="module")
def deviations():
    p0, grads = _inputs()
    seen = {}
    for alg in (R.ADAM, R.ADAMW, R.SGD):
        for wd in (0.0, 0.01):
            want = _torch_run(alg, wd, p0, grads)
            r64 = _ref_run(alg, wd, p0, grads, np.float64)
            r32 = _ref_run(alg, wd, p0, grads, np.float32)
            seen[alg, wd] = (_dev(r64, want), _dev(r32, r64))
            print(f"alg {alg} wd {wd}: f64 restatement vs torch {seen[alg, wd][0]:.3e}, f32 vs f64 restatement {seen[alg, wd][1]:.3e}")
    return seen


def test_f64_restatement_is_torch(deviations):
    """The restatement run in f64 against torch.optim in f64: rounding of f64 only: 4.38e-16 measured on
    these inputs, the gate is the issue's "about 1e-12"."""
    worst = max(v[0] for v in deviations.values())
    print("f64 restatement vs torch, worst:", worst)
    assert worst <= F64_GATE


def test_f32_restatement_differs_by_rounding_only(deviations):
    """The f32 restatement against the f64 one: 2.97e-7 measured on these inputs (about 2.5 ulp of f32
    after 20 steps), gated at twice that, 5.94e-7."""
    worst = max(v[1] for v in deviations.values())
    print("f32 vs f64 restatement, worst:", worst)
    assert 0 < worst <= F32_GATE


def test_scale_update_is_torchs():
    d = R.desc(growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    S = R.state(scale=65536.0)
    scale = torch.tensor(65536.0)
    tracker = torch.tensor(0, dtype=torch.int32)
    seq = [0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    for i, found in enumerate(seq):
        R.decide(d, S, bool(found), 0.0)
        torch._amp_update_scale_(scale, tracker, torch.tensor(float(found)), 2.0, 0.5, 3)
        assert (float(S["scale"]), S["growth_tracker"], S["found_inf"]) == (float(scale), int(tracker), found), i
    assert float(scale) == 65536.0 * 2.0 ** (-4 + 3) and S["step"] == seq.count(0)
    # a growth that would overflow is not taken; the tracker still restarts
    S = R.state(scale=3e38)
    S["growth_tracker"] = 2
    scale, tracker = torch.tensor(3e38), torch.tensor(2, dtype=torch.int32)
    R.decide(d, S, False, 0.0)
    torch._amp_update_scale_(scale, tracker, torch.tensor(0.0), 2.0, 0.5, 3)
    assert float(S["scale"]) == float(scale) == float(np.float32(3e38)) and S["growth_tracker"] == int(tracker) == 0
    # growth_interval 0: static
    S = R.state(scale=128.0)
    for found in (True, False, False):
        R.decide(R.desc(growth_interval=0), S, found, 0.0)
        assert float(S["scale"]) == 128.0 and S["growth_tracker"] == 0 and S["skipped"] == int(found)


@pytest.mark.parametrize("max_norm", [0.5, 1e3])
def test_clip_is_clip_grad_norm(max_norm):
    rng = np.random.default_rng(3)
    gs = [rng.standard_normal(s) for s in SHAPES]
    ps = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in SHAPES]
    for p, g in zip(ps, gs):
        p.grad = torch.tensor(g)
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    ts = [dict(master=np.zeros(g.size), grad=g.reshape(-1).copy()) for g in gs]
    found, ssq = R.global_stats(ts)
    S = R.state(scale=1.0)
    rec = R.decide(R.desc(max_norm=max_norm, growth_interval=0), S, found, ssq, np.float64)
    assert not found and abs(float(np.sqrt(ssq)) - total) <= 1e-12 * total
    assert abs(float(S["grad_norm"]) - total) <= 1e-6 * total
    assert (rec["k"] < 1) == (total > max_norm)
    for p, g in zip(ps, gs):
        np.testing.assert_allclose(g * rec["k"], p.grad.numpy(), rtol=1e-12, atol=0)
    # a scaled loss's gradients: the same clipped, unscaled gradients
    S = R.state(scale=1024.0)
    found, ssq = R.global_stats([dict(master=t["master"], grad=t["grad"] * 1024.0) for t in ts])
    rec2 = R.decide(R.desc(max_norm=max_norm, growth_interval=0), S, found, ssq, np.float64)
    assert abs(rec2["k"] * 1024.0 - rec["k"]) <= 1e-12 * rec["k"]


def test_plan_and_sum_order():
    C = R.CHUNK
    assert R.plan([0, 1, C - 1, C, C + 1, 0, 3 * C + 5]) == \
        [(1, 0), (2, 0), (3, 0), (4, 0), (4, C), (6, 0), (6, C), (6, 2 * C), (6, 3 * C)]
    assert R.plan([]) == [] and R.plan([0, 0]) == []
    rng = np.random.default_rng(0)
    g = rng.standard_normal(C - 3).astype(np.float32)
    g[5], g[C - 4] = np.nan, -np.inf
    cnt, ssq = R.chunk_stats(g)
    ok = np.isfinite(g)
    assert cnt == 2 and abs(ssq - float((g[ok].astype(np.float64) ** 2).sum())) <= 1e-12 * ssq
    # subnormal squares are kept, zeros of either sign add nothing
    cnt, ssq = R.chunk_stats(np.array([1e-20, -0.0, 0.0, 1e-30], np.float32))
    assert cnt == 0 and ssq == float(np.float64(np.float32(1e-20)) ** 2 + np.float64(np.float32(1e-30)) ** 2) > 0
    # a skipped step changes nothing but the gradients, the scale, the tracker and the outputs
    t = dict(master=np.ones(9, np.float32), model=np.ones(9, np.float16), grad=np.full(9, np.inf, np.float32),
             m=np.ones(9, np.float32), v=np.ones(9, np.float32))
    S = R.state(scale=4.0)
    R.step(R.desc(growth_interval=5), [t], S)
    assert (S["step"], S["b1pow"], S["b2pow"], float(S["scale"]), S["growth_tracker"], S["found_inf"], S["skipped"]) == \
        (0, 1.0, 1.0, 2.0, 0, 1, 1) and float(S["grad_norm"]) == 0.0
    assert (t["master"] == 1).all() and (t["m"] == 1).all() and (t["v"] == 1).all() and (t["model"] == 1).all() and not t["grad"].any()
