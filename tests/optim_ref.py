"""The optimiser step in numpy -- the checker of libpvoptim.so (include/pvoptim.h), TEST INFRASTRUCTURE ONLY.

The header's three kernels restated with the same per-operation rounding and the same sum order:
    plan(ns)                          the chunk list of pv_optim_plan
    step(desc, tensors, state)        one pv_optim_step, in place on numpy arrays and a dict
`desc` is a dict of the pv_optim_desc fields, `state` a dict of the pv_optim_state fields, a tensor a
dict(master=f32, model=f16 or None, grad=f32 or f16, m=f32, v=f32 or None).  With dtype=np.float64 the
element arithmetic and every hyper-parameter are f64 instead (the yardstick of tests/test_optim_ref.py);
the device is only ever compared with the default, f32."""
import numpy as np

CHUNK, THREADS, GROUP = 8192, 256, 8
ADAM, ADAMW, SGD = 0, 1, 2


def desc(algorithm=ADAM, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, momentum=0.0, max_norm=0.0,
         growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, zero_grads=1):
    return dict(algorithm=algorithm, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, momentum=momentum,
                max_norm=max_norm, growth_factor=growth_factor, backoff_factor=backoff_factor,
                growth_interval=growth_interval, zero_grads=zero_grads)


def state(lr=1e-3, scale=1.0):
    return dict(b1pow=1.0, b2pow=1.0, step=0, lr=np.float32(lr), scale=np.float32(scale), growth_tracker=0,
                grad_norm=np.float32(0), found_inf=0, skipped=0)


def plan(ns):
    return [(i, first) for i, n in enumerate(ns) for first in range(0, int(n), CHUNK)]


def _tree(lanes):
    red = lanes.copy()
    s = THREADS // 2
    while s >= 1:
        red[:s] += red[s:2 * s]
        s //= 2
    return red[0]


def chunk_stats(g):
    """(non-finite count, f64 sum of squares of the finite elements) of one chunk's gradients: element e
    is lane (e // 8) % 256's, a lane adds in increasing order, the lanes combine in the halving tree."""
    g = np.asarray(g)
    g = (g if g.dtype == np.float64 else g.astype(np.float32)).astype(np.float64)
    ok = np.isfinite(g)
    sq = np.zeros(CHUNK)
    sq[:g.size] = np.where(ok, g, 0.0) ** 2
    sq = sq.reshape(CHUNK // (THREADS * GROUP), THREADS, GROUP)
    acc = np.zeros(THREADS)
    for q in range(sq.shape[0]):
        for e in range(GROUP):
            acc = acc + sq[q, :, e]
    return int((~ok).sum()), _tree(acc)


def global_stats(tensors):
    parts = [chunk_stats(t["grad"][first:first + CHUNK]) for i, first in plan([t["master"].size for t in tensors])
             for t in (tensors[i],)]
    acc = np.zeros(THREADS)
    for q, (_, s) in enumerate(parts):
        acc[q % THREADS] += s
    return any(c for c, _ in parts), _tree(acc)


def decide(d, S, found, total, dtype=np.float32):
    """k_optim_decide: updates S in place and returns the decision record."""
    F = dtype
    f32 = np.float32
    hp = (lambda x: np.float64(x)) if F is np.float64 else (lambda x: np.float64(f32(x)))
    with np.errstate(all="ignore"):
        inv = 1.0 / np.float64(S["scale"])
        norm = np.sqrt(np.float64(total)) * inv
        c = min(1.0, hp(d["max_norm"]) / (norm + 1e-6)) if d["max_norm"] > 0 else 1.0
        k = F(inv * c)
        if not found:
            S["step"] += 1
            S["b1pow"] = np.float64(S["b1pow"]) * hp(d["beta1"])
            S["b2pow"] = np.float64(S["b2pow"]) * hp(d["beta2"])
        bc1, bc2 = F(1.0 - S["b1pow"]), F(1.0 - S["b2pow"])
        lr = F(S["lr"])
        rec = dict(k=k, step_size=F(lr / bc1), sq2=F(np.sqrt(bc2)), lr=lr, lr_wd=F(lr * F(d["weight_decay"])), skipped=bool(found))
        if d["growth_interval"] > 0:
            if found:
                S["scale"] = f32(f32(S["scale"]) * f32(d["backoff_factor"]))
                S["growth_tracker"] = 0
            else:
                t = S["growth_tracker"] + 1
                if t == d["growth_interval"]:
                    grown = f32(f32(S["scale"]) * f32(d["growth_factor"]))
                    if np.isfinite(grown):
                        S["scale"] = grown
                    t = 0
                S["growth_tracker"] = t
        S["grad_norm"] = f32(norm)
        S["found_inf"] = S["skipped"] = int(bool(found))
    return rec


def apply(d, rec, t, dtype=np.float32):
    """k_optim_apply on one tensor, in place."""
    F = dtype
    if rec["skipped"]:
        if d["zero_grads"]:
            t["grad"][...] = 0
        return
    alg = d["algorithm"]
    wd, b1, b2, eps, mom = (F(d[k]) for k in ("weight_decay", "beta1", "beta2", "eps", "momentum"))
    omb1, omb2 = F(F(1.0) - b1), F(F(1.0) - b2)
    with np.errstate(all="ignore"):
        g = t["grad"].astype(F) * rec["k"]
        p, m = t["master"].astype(F), t["m"].astype(F)
        if alg == SGD:
            if wd != 0:
                g = g + wd * p
            m = mom * m + g
            p = p - rec["lr"] * m
        else:
            v = t["v"].astype(F)
            if wd != 0:
                if alg == ADAM:
                    g = g + wd * p
                else:
                    p = p - rec["lr_wd"] * p
            m = b1 * m + omb1 * g
            v = b2 * v + (omb2 * g) * g
            p = p - rec["step_size"] * (m / (np.sqrt(v) / rec["sq2"] + eps))
            assert v.dtype == F
            t["v"][...] = v
        assert p.dtype == F and m.dtype == F and g.dtype == F
        t["master"][...] = p
        t["m"][...] = m
        if t.get("model") is not None:
            t["model"][...] = t["master"].astype(np.float32).astype(np.float16)
    if d["zero_grads"]:
        t["grad"][...] = 0


def step(d, tensors, S, dtype=np.float32):
    """One pv_optim_step.  A table without elements changes nothing, the state included."""
    if not any(t["master"].size for t in tensors):
        return None
    found, total = global_stats(tensors)
    rec = decide(d, S, found, total, dtype)
    for t in tensors:
        apply(d, rec, t, dtype)
    return rec
