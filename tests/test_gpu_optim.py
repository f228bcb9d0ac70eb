"""libpvoptim.so on the device (include/pvoptim.h, pvnet_amd/optim.py) against its numpy restatement
tests/optim_ref.py: masters, moments, the f16 model, the gradients and every field of the state, bit for bit."""
import copy
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

C = R.CHUNK
SIZES = [0, 1, 7, 8, 9, C - 1, C, C + 1, 3 * C + 5]
ALGS = {"adam": R.ADAM, "adamw": R.ADAMW, "sgd": R.SGD}
ARRAYS = ("master", "model", "grad", "m", "v")
BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16}


@pytest.fixture(scope="module")
def P(device):
    import __graft_entry__ as g
    g.build()
    from pvnet_amd import _optim_lib
    _optim_lib.load()
    return _optim_lib


def bits(a):
    return np.ascontiguousarray(a).view(BITS[a.dtype])


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


# ---- inputs ------------------------------------------------------------------------------------------------------
def gradients(rng, n, kind):
    """Magnitudes from 1e-20 to 1e4 (the square of the small ones is subnormal in f32), both signs, exact zeros
    of both signs; an f16 gradient also holds the f16 subnormal and the largest f16 of both signs."""
    g = (10.0 ** rng.uniform(-20, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.1] = 0.0
    g[rng.random(n) < 0.1] = -0.0
    if kind == "f16":
        g = np.clip(g, -6e4, 6e4).astype(np.float16)
        if n > 9:
            g[[2, 3, 4, n - 1]] = np.array([5.96e-8, 65504.0, -65504.0, -5.96e-8], np.float16)
    return g


def make_tensors(sizes, kind, seed, sgd=False):
    """One tensor per size; every third is an f32 parameter (no model copy)."""
    rng = np.random.default_rng([seed, len(sizes)])
    out = []
    for i, n in enumerate(sizes):
        master = rng.standard_normal(n).astype(np.float32)
        out.append(dict(master=master, model=master.astype(np.float16) if i % 3 else None, grad=gradients(rng, n, kind),
                        m=np.zeros(n, np.float32), v=np.full(n, np.nan, np.float32) if sgd else np.zeros(n, np.float32)))
    return out


def table_sizes():
    """About 40 tensors: every size of SIZES four or five times, in an order that mixes them."""
    rng = np.random.default_rng(11)
    sizes = SIZES * 4 + [0, 1, 9, C + 1]
    return [int(s) for s in rng.permutation(sizes)]


# ---- the device side ------------------------------------------------------------------------------------------------
class Case:
    """The tensors of a table carved from one flat device buffer per array.  layout 'aligned': every tensor starts
    at a multiple of 8 elements (the vector form); 'odd': at an odd element offset (the scalar form); 'mixed': the
    two alternate.  The padding between tensors holds NaN and must stay as it is."""

    def __init__(self, P, device, tensors, alg, layout, state, g=None, ws_fill=0x00):
        from pvnet_amd import optim as O
        self.P, self.device, self.n, self.alg = P, device, len(tensors), alg
        self.ns = [t["master"].size for t in tensors]
        self.has_model = [t["model"] is not None for t in tensors]
        self.offs, at = [], 8
        for i, n in enumerate(self.ns):
            odd = layout == "odd" or (layout == "mixed" and i % 2 == 1)
            self.offs.append(at + (2 * (i % 4) + 1 if odd else 0))
            at = (self.offs[-1] + n + 8 + 7) // 8 * 8
        self.total = at
        self.flat0, self.dev = {}, {}
        for name in ARRAYS:
            dtype = tensors[0][name].dtype if name == "grad" else np.dtype(np.float16 if name == "model" else np.float32)
            flat = np.full(self.total, np.nan, dtype)
            for t, off, n in zip(tensors, self.offs, self.ns):
                if t[name] is not None:
                    flat[off:off + n] = t[name]
            self.flat0[name] = flat
            tdt = torch.float16 if dtype == np.float16 else torch.float32
            buf = g.out((self.total,), tdt, name=name) if g else torch.empty(self.total, dtype=tdt, device=device)
            buf.copy_(torch.from_numpy(flat))
            assert buf.data_ptr() % 16 == 0
            self.dev[name] = buf
        entries = []
        for i, (off, n) in enumerate(zip(self.offs, self.ns)):
            v = {name: self.dev[name][off:off + n] for name in ARRAYS}
            entries.append((v["master"], v["model"] if self.has_model[i] else None, v["grad"], v["m"],
                            None if (alg == R.SGD and i % 2) else v["v"]))       # SGD: v present or NULL, never touched
        self.table, self.chunks, self.n_chunks = O.make_table(entries, alg, device)
        assert self.n_chunks == len(R.plan(self.ns))
        need = P.load().pv_optim_workspace_size(self.n_chunks)
        self.ws = g.workspace(need, fill=ws_fill) if g else torch.full((need,), ws_fill, dtype=torch.uint8, device=device)
        assert self.ws.data_ptr() % 256 == 0 and self.ws.numel() == need
        self.state = O.upload((P.OptState * 1)(P.OptState(state["b1pow"], state["b2pow"], state["step"], float(state["lr"]),
                                                          float(state["scale"]), state["growth_tracker"], 0.0, 0, 0)), device)

    def set_grads(self, tensors):
        flat = self.flat0["grad"].copy()
        for t, off, n in zip(tensors, self.offs, self.ns):
            flat[off:off + n] = t["grad"]
        self.dev["grad"].copy_(torch.from_numpy(flat))

    def step(self, d):
        desc = self.P.OptDesc(**d, pad_=0)
        code = self.P.load().pv_optim_step(ctypes.byref(desc), self.table.data_ptr(), self.n, self.chunks.data_ptr(),
                                           self.n_chunks, self.state.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                           torch.cuda.current_stream().cuda_stream)
        assert code == 0, code

    def read_state(self):
        return self.P.OptState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def compare(self, tensors, S, what=""):
        """Every array of every tensor, the padding around them and the state against the restatement's."""
        for name in ARRAYS:
            got = self.dev[name].cpu().numpy()
            want = self.flat0[name].copy()
            for i, (t, off, n) in enumerate(zip(tensors, self.offs, self.ns)):
                if t[name] is not None:
                    want[off:off + n] = t[name]
            same(got, want, f"{what} {name}")
        st = self.read_state()
        for f in ("b1pow", "b2pow", "step", "growth_tracker", "found_inf", "skipped"):
            assert getattr(st, f) == S[f], (what, f, getattr(st, f), S[f])
        for f in ("lr", "scale", "grad_norm"):
            same(np.array([getattr(st, f)], np.float32), np.array([S[f]], np.float32), f"{what} state.{f}")


def desc_for(alg, **kw):
    d = dict(weight_decay=0.01, momentum=0.9, max_norm=0.0 if alg == R.SGD else 100.0, growth_interval=3)
    d.update(kw)
    return R.desc(alg, **d)


@functools.lru_cache(maxsize=None)
def reference_run(alg_name, kind):
    """Five steps of the big table in the restatement: [(tensors before the step, tensors after, state after)]."""
    alg = ALGS[alg_name]
    ts = make_tensors(table_sizes(), kind, seed=5, sgd=alg == R.SGD)
    S = R.state(lr=1e-3, scale=1024.0)
    d = desc_for(alg)
    out = []
    for s in range(5):
        rng = np.random.default_rng([99, s])
        for t in ts:
            t["grad"] = gradients(rng, t["master"].size, kind)
        before = copy.deepcopy(ts)
        R.step(d, ts, S)
        out.append((before, copy.deepcopy(ts), dict(S)))
    return out


@pytest.mark.parametrize("layout", ["mixed", "aligned", "odd"])
@pytest.mark.parametrize("kind", ["f16", "f32"])
@pytest.mark.parametrize("alg_name", list(ALGS))
def test_five_steps_bit_equal(P, device, alg_name, kind, layout):
    """~40 tensors of every size around a chunk and a group, each layout against the one restatement run: the
    vector and the scalar form give the same bits."""
    alg = ALGS[alg_name]
    ref = reference_run(alg_name, kind)
    assert len(ref[0][0]) >= 40 and not any(S["skipped"] for _, _, S in ref) and ref[-1][2]["step"] == 5
    assert any(S["growth_tracker"] == 0 for _, _, S in ref) and float(ref[-1][2]["scale"]) == 2048.0
    case = Case(P, device, ref[0][0], alg, layout, R.state(lr=1e-3, scale=1024.0))
    d = desc_for(alg)
    for s, (before, after, S) in enumerate(ref):
        case.set_grads(before)
        case.step(d)
        case.compare(after, S, f"{alg_name} {kind} {layout} step {s}")


def small(kind="f32", sgd=False):
    return make_tensors([7, C + 1, 0, 9], kind, seed=21, sgd=sgd)


def run_both(P, device, ts, d, S, steps=1, layout="mixed", edit=None, **kw):
    """`steps` steps on the device and in the restatement from the same inputs, compared after each; `edit(ts, s)`
    rewrites the gradients before step s.  Returns the case, the restatement's tensors and state."""
    ts, S = copy.deepcopy(ts), dict(S)
    case = Case(P, device, ts, d["algorithm"], layout, S, **kw)
    for s in range(steps):
        if edit:
            edit(ts, s)
        case.set_grads(ts)
        R.step(d, ts, S)
        case.step(d)
        case.compare(ts, S, f"step {s}")
    return case, ts, S


@pytest.mark.parametrize("where", ["last of last", "first of first"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("kind", ["f16", "f32"])
def test_non_finite_gradient_skips_the_step(P, device, kind, bad, where):
    ts = small(kind)
    t, e = (ts[-1], -1) if where == "last of last" else (ts[0], 0)
    t["grad"][e] = bad
    S0 = R.state(lr=1e-3, scale=64.0)
    S0["growth_tracker"] = 1
    for zero in (1, 0):
        d = desc_for(R.ADAM, zero_grads=zero)
        start = copy.deepcopy(ts)
        _, after, S = run_both(P, device, ts, d, S0)
        assert (S["skipped"], S["found_inf"], S["step"], S["b1pow"], S["b2pow"], S["growth_tracker"]) == (1, 1, 0, 1.0, 1.0, 0)
        assert float(S["scale"]) == 32.0 and np.isfinite(S["grad_norm"])
        for a, b in zip(after, start):
            for name in ("master", "model", "m", "v"):
                if a[name] is not None:
                    same(a[name], b[name])
            if zero:
                assert not bits(a["grad"]).any()
            else:
                same(a["grad"], b["grad"])


@pytest.mark.parametrize("max_norm,clipped", [(5.0001, False), (4.9999, True), (0.0, False), (-1.0, False), (float("inf"), False)])
def test_clip_threshold(P, device, max_norm, clipped):
    ts = make_tensors([2, C], "f32", seed=1)
    ts[0]["grad"][:] = [3.0 * 256.0, 0.0]
    ts[1]["grad"][:] = 0.0
    ts[1]["grad"][C - 1] = -4.0 * 256.0
    S0 = R.state(lr=1e-2, scale=256.0)
    d = desc_for(R.ADAMW, max_norm=max_norm)
    found, ssq = R.global_stats(ts)
    rec = R.decide(d, dict(S0), found, ssq)
    assert (rec["k"] < np.float32(1 / 256.0)) == clipped and (clipped or rec["k"] == np.float32(1 / 256.0))
    _, _, S = run_both(P, device, ts, d, S0)
    assert float(S["grad_norm"]) == 5.0 and S["skipped"] == 0


def test_scale_growth_static_and_overflow(P, device):
    ts = small("f16")

    def regrad(ts_, s):
        rng = np.random.default_rng([4, s])
        for t in ts_:
            t["grad"] = gradients(rng, t["master"].size, "f16")
        if s == 3:
            ts_[1]["grad"][C] = np.inf
    # growth_interval 2: the scale doubles on every second unskipped step and halves on the overflow
    _, _, S = run_both(P, device, ts, desc_for(R.SGD, growth_interval=2), R.state(lr=1e-3, scale=8.0), steps=5, edit=regrad)
    assert (float(S["scale"]), S["growth_tracker"], S["step"]) == (8.0, 1, 4)
    # growth_interval 0: static, the overflowed step is still skipped
    _, _, S = run_both(P, device, ts, desc_for(R.ADAM, growth_interval=0), R.state(lr=1e-3, scale=8.0), steps=5, edit=regrad)
    assert (float(S["scale"]), S["growth_tracker"], S["step"]) == (8.0, 0, 4)
    # a growth that would overflow the scale is not taken
    _, _, S = run_both(P, device, ts, desc_for(R.ADAM, growth_interval=1), R.state(lr=1e-3, scale=3e38), steps=2, edit=regrad)
    assert (float(S["scale"]), S["growth_tracker"], S["step"]) == (float(np.float32(3e38)), 0, 2)


@pytest.mark.parametrize("alg_name", list(ALGS))
def test_zero_grads_off_keeps_the_gradients(P, device, alg_name):
    ts = small("f16", sgd=alg_name == "sgd")
    grads = [t["grad"].copy() for t in ts]
    _, after, S = run_both(P, device, ts, desc_for(ALGS[alg_name], zero_grads=0, weight_decay=0.0), R.state(lr=1e-3, scale=2.0), steps=2)
    assert S["step"] == 2 and all(bits(a["grad"]).tolist() == bits(g).tolist() for a, g in zip(after, grads))


def test_one_tensor_of_one_element(P, device):
    for kind in ("f16", "f32"):
        for layout in ("aligned", "odd"):
            ts = make_tensors([1], kind, seed=8)
            if kind == "f16":
                ts[0]["model"] = ts[0]["master"].astype(np.float16)
            ts[0]["grad"][0] = 3.0
            _, after, S = run_both(P, device, ts, desc_for(R.ADAM), R.state(lr=0.5, scale=1.0), steps=3, layout=layout)
            assert S["step"] == 3 and S["grad_norm"] == np.float32(0)      # zeroed by step 1; 3 at step 1 (compared)


def test_two_runs_give_the_same_bits(P, device):
    ref = reference_run("adam", "f16")
    outs = []
    for _ in range(2):
        case = Case(P, device, ref[0][0], R.ADAM, "mixed", R.state(lr=1e-3, scale=1024.0))
        for before, _, _ in ref[:2]:
            case.set_grads(before)
            case.step(desc_for(R.ADAM))
        outs.append([case.dev[name].cpu().numpy() for name in ARRAYS] + [case.state.cpu().numpy()])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0xA5])
def test_workspace_need_not_be_cleared(P, device, fill):
    ref = reference_run("adamw", "f32")
    case = Case(P, device, ref[0][0], R.ADAMW, "mixed", R.state(lr=1e-3, scale=1024.0), ws_fill=fill)
    case.step(desc_for(R.ADAMW))
    case.compare(ref[0][1], ref[0][2], f"workspace {fill:#x}")


@pytest.mark.parametrize("alg_name,kind", [("adam", "f16"), ("adamw", "f32"), ("sgd", "f16")])
def test_memory_contract(P, device, alg_name, kind):
    """Every array and the exactly sized workspace between patterned guards; the NaN padding between the tensors
    and the NaN-filled v of an SGD table stay bit for bit (compare() checks both)."""
    ref = reference_run(alg_name, kind)
    g = Guarded(device)
    case = Case(P, device, ref[0][0], ALGS[alg_name], "mixed", R.state(lr=1e-3, scale=1024.0), g=g, ws_fill=0xA5)
    if alg_name == "sgd":
        assert all(np.isnan(t["v"]).all() for t in ref[0][0])
    for before, after, S in ref[:2]:
        case.set_grads(before)
        case.step(desc_for(ALGS[alg_name]))
        case.compare(after, S, f"guarded {alg_name}")
    g.check()


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def ref_of(opt):
    """The restatement's tensors and state of an Optimizer, read from the device."""
    ts = [dict(master=w.detach().cpu().numpy().reshape(-1).copy(),
               model=p.detach().cpu().numpy().reshape(-1).copy() if p.dtype == torch.float16 else None,
               grad=g.cpu().numpy().reshape(-1).copy(), m=m.cpu().numpy().reshape(-1).copy(),
               v=v.cpu().numpy().reshape(-1).copy() if v is not None else None)
          for w, p, g, m, v in zip(opt.masters, opt.params, opt.grads, opt.m, opt.v)]
    st = opt.stats()
    S = R.state(lr=float(opt._views["lr"]), scale=float(st["scale"]))
    S.update(step=int(st["step"]), b1pow=float(opt._views["b1pow"]), b2pow=float(opt._views["b2pow"]),
             growth_tracker=int(opt._views["growth_tracker"]))
    return ts, S


def desc_of(opt):
    return {f: getattr(opt.desc, f) for f, _ in opt.desc._fields_ if f != "pad_"}


def compare_opt(opt, ts, S, what):
    got, gS = ref_of(opt)
    for a, b in zip(got, ts):
        for name in ARRAYS:
            if b[name] is not None:
                same(a[name], b[name], f"{what} {name}")
    st = opt.stats()
    for f in ("b1pow", "b2pow", "step", "growth_tracker"):
        assert gS[f] == S[f], (what, f)
    assert (int(st["found_inf"]), int(st["skipped"])) == (S["found_inf"], S["skipped"]), what
    for f in ("lr", "scale"):
        same(np.array([gS[f]], np.float32), np.array([S[f]], np.float32), f"{what} {f}")
    same(st["grad_norm"].cpu().numpy().reshape(1), np.array([S["grad_norm"]], np.float32), f"{what} grad_norm")


def test_captured_step_replays(P, device):
    from pvnet_amd import Optimizer
    torch.manual_seed(0)
    params = [("w16", torch.nn.Parameter(torch.randn(C + 5, device=device).half())),
              ("b32", torch.nn.Parameter(torch.randn(3, 3, device=device))),
              ("g16", torch.nn.Parameter(torch.randn(8, device=device).half()))]
    opt = Optimizer(params, "adamw", lr=1e-2, weight_decay=0.01, max_norm=50.0, init_scale=16.0, growth_interval=2)
    assert all(p.grad is g for (_, p), g in zip(params, opt.grads))
    d = desc_of(opt)

    def write_grads(s, plant=None):
        rng = np.random.default_rng([31, s])
        for i, g in enumerate(opt.grads):
            a = gradients(rng, g.numel(), "f16" if g.dtype == torch.float16 else "f32")
            if plant is not None and i == 0:
                a[C + 4] = plant
            g.copy_(torch.from_numpy(a).reshape(g.shape))

    # an eager step first, on a side stream as captures want it
    write_grads(0)
    ts, S = ref_of(opt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    R.step(d, ts, S)
    compare_opt(opt, ts, S, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    compare_opt(opt, ts, S, "after the capture")          # a capture runs nothing
    for s in range(1, 5):
        write_grads(s, plant=np.inf if s == 3 else None)
        if s == 2:
            opt.set_lr(3e-3)
            S["lr"] = np.float32(3e-3)
        for t, g in zip(ts, opt.grads):
            t["grad"] = g.cpu().numpy().reshape(-1).copy()
        graph.replay()
        R.step(d, ts, S)
        compare_opt(opt, ts, S, f"replay {s}")
        assert S["skipped"] == (1 if s == 3 else 0)
    assert S["step"] == 4
    # a gradient that is no longer the table's: rebuilt outside a capture, an error inside one
    fresh = [torch.zeros_like(g) for g in opt.grads]
    params[1][1].grad = fresh[1]
    opt.step()
    assert opt.grads[1] is fresh[1]
    params[0][1].grad = None
    opt.step()
    assert params[0][1].grad is opt.grads[0]
    torch.cuda.synchronize()
    other = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="g16"), warnings.catch_warnings():
        warnings.simplefilter("ignore")              # torch remarks that the graph is empty: nothing was launched
        with torch.cuda.graph(other):
            params[2][1].grad = fresh[2]
            opt.step()
    # state_dict round trip
    sd = opt.state_dict()
    write_grads(9)
    opt.step()
    opt.load_state_dict(sd)
    for a, b in zip(opt.masters, sd["master"]):
        assert torch.equal(a, b)
    assert torch.equal(opt.state, sd["state"])


def test_closed_loop_training(P, device):
    """A two-layer f16 conv net trained 30 steps through pvnet_loss, scale_loss and Optimizer from a scale that
    overflows: the recorded gradients replayed through the restatement give the final parameters bit for bit."""
    from pvnet_amd import Optimizer, pvnet_loss
    torch.manual_seed(1)
    ncls, vn, H, W, b = 2, 1, 32, 32, 2
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(),
                              torch.nn.Conv2d(8, ncls + 1 + 2 * ncls * vn, 3, padding=1)).to(device).half()
    y, x = np.mgrid[:H, :W]
    label = np.zeros((b, H, W), np.uint8)
    label[0, 4:16, 4:20] = 1
    label[0, 18:30, 10:28] = 2
    label[1, 8:24, 2:14] = 2
    label[1, 6:20, 18:30] = 1
    image = np.stack([label * 0.5, np.broadcast_to(x / W, (b, H, W)), np.broadcast_to(y / H, (b, H, W))], 1)
    target = np.zeros((b, H, W, ncls * vn, 2), np.float32)
    target[..., 0] = ((x - 16.0) / 16.0)[None, :, :, None]
    target[..., 1] = ((y - 16.0) / 16.0)[None, :, :, None]
    image_d = torch.from_numpy(image.astype(np.float16)).to(device)
    label_d, target_d = torch.from_numpy(label).to(device), torch.from_numpy(target).to(device)
    opt = Optimizer(net.named_parameters(), "adam", lr=2e-2, max_norm=100.0, init_scale=2.0 ** 30, growth_interval=4)
    d = desc_of(opt)
    ts, S = ref_of(opt)
    losses, skipped = [], 0
    for s in range(30):
        out = net(image_d)
        loss_seg, loss_vertex, _ = pvnet_loss(out[:, :ncls + 1], out[:, ncls + 1:], label_d, target_d, class_num=ncls)
        loss = loss_seg.mean() + loss_vertex.mean()
        opt.scale_loss(loss).backward()
        losses.append(float(loss.detach()))
        for t, g in zip(ts, opt.grads):
            t["grad"] = g.cpu().numpy().reshape(-1).copy()
        opt.step()
        R.step(d, ts, S)
        skipped += int(opt.stats()["skipped"])
        assert int(opt.stats()["skipped"]) == S["skipped"], s
    compare_opt(opt, ts, S, "after 30 steps")
    print("closed loop: losses", losses[0], losses[-1], "skipped", skipped, "scale", float(S["scale"]))
    assert skipped >= 1 and S["step"] == 30 - skipped and S["step"] >= 5
    assert losses[-1] < losses[0]
