"""pvnet_amd.net_utils on the device against the numpy float64 restatement (tests/loss_ref.py) on the
same, already rounded inputs: values and gradients within the f32 round-off bounds, exact counts,
every layout and stride, the edge labels and thresholds, zero-weight elements that are never used,
autograd, determinism under graph capture, the reference-named wrappers, and the closed loop
render_ground_truth -> loss -> one gradient step -> the ground truth.

The bounds (u = 2^-24) are the issue's, from the f32 round-off and not from a run:
    |loss_seg - ref|    <= 32 u (1 + max|logit|)
    |loss_vertex - ref| <= 16 u ref + 1e-12
    |grad_seg - ref|    <= 16 u |g| / (H W)              (+ half an f16 ulp of the value for f16)
    |grad_vertex - ref| <= 16 u |g| / (2 vn fg + 1e-3)   (+ half an f16 ulp of the value for f16)
Every check prints its measured maximum as a fraction of its bound (pytest -s shows them; DESIGN 10f
records a run)."""
import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests import render_ref as RR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NP = {torch.float32: np.float32, torch.float16: np.float16, torch.uint8: np.uint8, torch.int32: np.int32,
      torch.int64: np.int64}
F32, F16 = torch.float32, torch.float16


@pytest.fixture(scope="module")
def N(device):
    import __graft_entry__ as g
    g.build()
    from pvnet_amd import net_utils
    return net_utils


# ---- inputs ----------------------------------------------------------------------------------------------------
def blob_labels(rng, b, H, W, ncls):
    """Labels 0..ncls in axis-aligned blobs over a background, about 40 % foreground."""
    lab = np.zeros((b, H, W), np.int64)
    for i in range(b):
        for c in range(ncls):
            for _ in range(2):
                y0, x0 = rng.integers(0, H), rng.integers(0, W)
                lab[i, y0:y0 + max(1, H // 3), x0:x0 + max(1, W // 3)] = c + 1
    return lab


def make(seed, b, H, W, ncls, vn, sdt=F32, vdt=F32, tdt=F32, logit_scale=3.0):
    """numpy inputs already rounded to the kinds the device gets: seg [b, ncls+1, H, W], vertex and
    target logical [b, H, W, C, 2], label i64."""
    rng = np.random.default_rng(seed)
    seg = rng.normal(0, logit_scale, (b, ncls + 1, H, W)).astype(NP[sdt])
    vertex = rng.normal(0, 1.0, (b, H, W, ncls * vn, 2)).astype(NP[vdt])
    target = rng.normal(0, 0.7, (b, H, W, ncls * vn, 2))
    target = (target / np.maximum(np.linalg.norm(target, axis=-1, keepdims=True), 1e-3)).astype(NP[tdt])
    return seg, vertex, target, blob_labels(rng, b, H, W, ncls)


def place(a, device, crop=False, channels_last=False):
    """A device tensor holding `a`: contiguous, channels-last (4-D), or a cropped view of a larger tensor
    filled with NaN (floats) or 200 (integers), which no kernel may touch."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if crop:
        pad = [(0, 0)] + [(1, 2)] * (t.dim() - 1)
        big = torch.full([s + lo + hi for s, (lo, hi) in zip(t.shape, pad)], float("nan") if t.is_floating_point() else 200,
                         dtype=t.dtype)
        sl = tuple(slice(lo, lo + s) for s, (lo, hi) in zip(t.shape, pad))
        big[sl] = t
        return big.to(device)[sl]
    t = t.to(device)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def field(a5, layout, device, crop=False):
    return place(a5 if layout == "bhwk2" else R.network(a5), device, crop)


def half_ulp16(v):
    """Half an f16 ulp of |v| (the subnormal spacing below 2^-14)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


def report(what, err, bound):
    frac = float(np.max(err / bound)) if np.size(err) else 0.0
    print(f"  {what}: max error / bound = {frac:.3f}")
    assert frac <= 1.0, f"{what}: error {float(np.max(err)):.3e} is {frac:.2f} x its bound"
    return frac


def run(N, seg, ver, lab, tgt, ncls, sigma, g_seg, g_ver):
    """One forward and one backward with the given per-image upstream gradients -> numpy results."""
    seg, ver = seg.detach().requires_grad_(), ver.detach().requires_grad_()
    ls, lv, st = N.pvnet_loss(seg, ver, lab, tgt, ncls, sigma)
    assert ls.dtype == lv.dtype == torch.float32 and ls.shape == lv.shape == (lab.shape[0],)
    dev = lab.device
    ((ls * torch.as_tensor(g_seg, device=dev)).sum() + (lv * torch.as_tensor(g_ver, device=dev)).sum()).backward()
    assert seg.grad.dtype == seg.dtype and ver.grad.dtype == ver.dtype
    assert seg.grad.shape == seg.shape and ver.grad.shape == ver.shape
    out = dict(loss_seg=ls, loss_vertex=lv, grad_seg=seg.grad, grad_vertex=ver.grad, **st)
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def upstream(label, ncls, vn):
    """Per-image upstream gradients that keep f16 gradients normal: about H W for the segmentation and
    the vector field's own denominator, non-uniform over the batch (exact in f32)."""
    b, H, W = label.shape
    fg = ((label >= 1) & (label <= ncls)).reshape(b, -1).sum(1)
    k = 1.0 - 0.25 * (np.arange(b) % 3)
    return (H * W * k).astype(np.float32), (np.maximum(2 * vn * fg, 1) * k[::-1]).astype(np.float32)


def compare(got, seg, vertex, target, label, ncls, vn, sigma, g_seg, g_ver, tag):
    """Everything `run` returned against the restatement on the same inputs, with the issue's bounds."""
    b, H, W = label.shape
    print(f"{tag}:")
    ref = R.forward(seg, vertex, target, label, ncls, vn, sigma)
    gs, gv = R.backward(seg, vertex, target, label, ncls, vn, sigma, g_seg, g_ver)
    assert (got["fg"] == ref["fg"]).all()
    for j, k in enumerate(("tp", "fp", "fn")):
        assert (got[k] == ref["counts"][:, :, j]).all(), k
    tp, fp, fn = (ref["counts"][..., j].astype(np.float32) for j in range(3))
    np.testing.assert_allclose(got["precision"], (tp + 1) / (tp + fp + 1), rtol=4 * U, atol=0)
    np.testing.assert_allclose(got["recall"], (tp + 1) / (tp + fn + 1), rtol=4 * U, atol=0)
    fr = {}
    fr["loss_seg"] = report("loss_seg", np.abs(got["loss_seg"] - ref["loss_seg"]),
                            32 * U * (1 + np.abs(seg.astype(np.float64)).max()))
    fr["loss_vertex"] = report("loss_vertex", np.abs(got["loss_vertex"] - ref["loss_vertex"]), 16 * U * ref["loss_vertex"] + 1e-12)
    bound = 16 * U * np.abs(g_seg.astype(np.float64))[:, None, None, None] / (H * W) + np.zeros_like(gs)
    if got["grad_seg"].dtype == np.float16:
        bound = bound + half_ulp16(gs)
    fr["grad_seg"] = report("grad_seg", np.abs(got["grad_seg"].astype(np.float64) - gs), np.maximum(bound, 1e-300))
    g5 = R.logical(got["grad_vertex"], ncls).astype(np.float64)
    bound = 16 * U * (np.abs(g_ver.astype(np.float64)) / (2.0 * vn * ref["fg"] + 1e-3))[:, None, None, None, None] + np.zeros_like(gv)
    if got["grad_vertex"].dtype == np.float16:
        bound = bound + half_ulp16(gv)
    fr["grad_vertex"] = report("grad_vertex", np.abs(g5 - gv), np.maximum(bound, 1e-300))
    # a zero weight is an exact zero, an ignored pixel too
    w = np.broadcast_to(((label[..., None] - 1) == (np.arange(ncls * vn) // vn))[..., None], gv.shape)
    assert (g5[~w] == 0).all()
    assert (got["grad_seg"][np.broadcast_to(((label < 0) | (label > ncls))[:, None], gs.shape)] == 0).all()
    return fr


# ---- 1. shapes, kinds and layouts ------------------------------------------------------------------------------
# (seg kind, vertex kind, target kind, label kind, vertex layout, target layout): every kind of every
# input, and the four layout pairs
COMBOS = [(F32, F32, F32, torch.uint8, "network", "network"),
          (F16, F16, F16, torch.int32, "network", "bhwk2"),
          (F32, F16, F32, torch.int64, "bhwk2", "network"),
          (F16, F32, F16, torch.uint8, "bhwk2", "bhwk2")]
SHAPES = [(1, 5, 7), (3, 33, 67), (2, 64, 80)]


@pytest.mark.parametrize("vn", [1, 9])
@pytest.mark.parametrize("ncls", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_values_counts_and_gradients(device, N, shape, ncls, vn):
    b, H, W = shape
    for n, (sdt, vdt, tdt, ldt, vlay, tlay) in enumerate(COMBOS):
        sigma = (1.0, 2.0)[n % 2]
        seg, vertex, target, label = make(100 + n, b, H, W, ncls, vn, sdt, vdt, tdt)
        g_seg, g_ver = upstream(label, ncls, vn)
        got = run(N, place(seg, device), field(vertex, vlay, device), place(label.astype(NP[ldt]), device),
                  field(target, tlay, device), ncls, sigma, g_seg, g_ver)
        compare(got, seg, vertex, target, label, ncls, vn, sigma, g_seg, g_ver,
                f"{shape} ncls={ncls} vn={vn} seg={sdt} vertex={vdt}/{vlay} target={tdt}/{tlay} label={ldt} sigma={sigma}")


# ---- 2. strides ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
def test_channels_last_and_cropped_views(device, N, dt):
    b, H, W, ncls, vn = 3, 33, 67, 3, 9
    seg, vertex, target, label = make(7, b, H, W, ncls, vn, dt, dt, dt)
    g_seg, g_ver = upstream(label, ncls, vn)
    dense = run(N, place(seg, device), field(vertex, "network", device), place(label, device),
                field(target, "network", device), ncls, 1.0, g_seg, g_ver)
    compare(dense, seg, vertex, target, label, ncls, vn, 1.0, g_seg, g_ver, f"dense {dt}")
    variants = {
        "channels-last seg": dict(seg=place(seg, device, channels_last=True)),
        "cropped seg": dict(seg=place(seg, device, crop=True)),
        "cropped label u8": dict(lab=place(label.astype(np.uint8), device, crop=True)),
        "cropped label i64": dict(lab=place(label, device, crop=True)),
        "cropped network vertex": dict(ver=field(vertex, "network", device, crop=True)),
        "cropped bhwk2 vertex": dict(ver=field(vertex, "bhwk2", device, crop=True)),
        "cropped network target": dict(tgt=field(target, "network", device, crop=True)),
        "cropped bhwk2 target": dict(tgt=field(target, "bhwk2", device, crop=True)),
        "all cropped": dict(seg=place(seg, device, crop=True), lab=place(label.astype(np.int32), device, crop=True),
                            ver=field(vertex, "network", device, crop=True), tgt=field(target, "bhwk2", device, crop=True)),
    }
    for name, kw in variants.items():
        t = dict(seg=place(seg, device), ver=field(vertex, "network", device), lab=place(label, device),
                 tgt=field(target, "network", device))
        t.update(kw)
        assert name.startswith("channels") or not all(x.is_contiguous() for x in kw.values()), name
        got = run(N, t["seg"], t["ver"], t["lab"], t["tgt"], ncls, 1.0, g_seg, g_ver)
        # the same lanes add the same terms in the same order whatever the strides: the same bits
        for k in dense:
            a = got[k] if k != "grad_vertex" else R.logical(got[k], ncls)
            np.testing.assert_array_equal(a, dense[k] if k != "grad_vertex" else R.logical(dense[k], ncls), err_msg=f"{name}: {k}")


# ---- 3. edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldt", [torch.uint8, torch.int32, torch.int64], ids=["u8", "i32", "i64"])
@pytest.mark.parametrize("ncls", [1, 3])
def test_edge_labels_and_empty_and_full_images(device, N, ncls, ldt):
    b, H, W, vn = 3, 33, 67, 9
    seg, vertex, target, label = make(21, b, H, W, ncls, vn)
    label[0] = 0                                                       # no foreground
    label[1] = 1 + (np.arange(W)[None, :] // 7) % ncls                 # all foreground
    edge = [0, ncls, ncls + 1, 255] + ([] if ldt == torch.uint8 else [-1, -2 ** 31])
    label[2, :, :] = np.array(edge)[(np.arange(H)[:, None] * 5 + np.arange(W)[None, :]) % len(edge)]
    dev_label = label.astype(NP[ldt])
    assert (dev_label.astype(np.int64) == label).all()
    g_seg, g_ver = upstream(label, ncls, vn)
    got = run(N, place(seg, device), field(vertex, "network", device), place(dev_label, device),
              field(target, "bhwk2", device), ncls, 1.0, g_seg, g_ver)
    compare(got, seg, vertex, target, label, ncls, vn, 1.0, g_seg, g_ver, f"edge labels ncls={ncls} {ldt}")
    assert got["fg"][0] == 0 and got["loss_vertex"][0] == 0.0 and (got["grad_vertex"][0] == 0).all()
    assert got["fg"][1] == H * W and got["loss_vertex"][1] > 0 and (got["tp"][0] == 0).all() and (got["fn"][0] == 0).all()


@pytest.mark.parametrize("sigma", [1.0, 2.0])
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
def test_smooth_l1_threshold(device, N, dt, sigma):
    """|d| exactly at 1 / sigma^2 and one step of the kind's last place to either side, both signs; the
    target there is 0, so d is the prediction itself."""
    b, H, W, ncls, vn = 1, 5, 67, 1, 9
    seg, vertex, target, label = make(31, b, H, W, ncls, vn, F32, dt, dt)
    t = NP[dt](1.0 / sigma ** 2)
    lo, hi = np.nextafter(t, NP[dt](0)), np.nextafter(t, NP[dt](2))
    steps = np.array([t, -t, lo, hi, -lo, -hi], NP[dt])
    label[0, 1] = 1
    target[0, 1] = 0
    vertex[0, 1] = steps[(np.arange(W)[:, None, None] + np.arange(vn)[None, :, None] + np.arange(2)[None, None, :]) % 6]
    g_seg, g_ver = upstream(label, ncls, vn)
    got = run(N, place(seg, device), field(vertex, "network", device), place(label, device),
              field(target, "network", device), ncls, sigma, g_seg, g_ver)
    compare(got, seg, vertex, target, label, ncls, vn, sigma, g_seg, g_ver, f"threshold {dt} sigma={sigma}")
    # at and beyond the threshold the slope is the sign, below it sigma^2 d: exact factors of the scale
    g5 = R.logical(got["grad_vertex"], ncls)[0, 1].astype(np.float64)
    scale = np.float32(g_ver[0]) / np.float32(2.0 * vn * got["fg"][0] + 1e-3)
    d = vertex[0, 1].astype(np.float64)
    lin = np.abs(d) >= 1.0 / sigma ** 2
    assert lin.any() and (~lin).any()
    if dt == F32:
        assert (g5[lin] == np.float32(scale) * np.sign(d[lin])).all()


def test_large_logits_and_ties(device, N):
    b, H, W, ncls, vn = 2, 33, 67, 3, 1
    seg, vertex, target, label = make(41, b, H, W, ncls, vn)
    rng = np.random.default_rng(5)
    seg[0] = rng.choice(np.array([-80.0, 80.0], np.float32), seg[0].shape)      # ties among the +80 too
    tie = rng.integers(0, 4, (H, W))
    seg[1] = 0
    seg[1, 1][tie == 1] = 2.5
    seg[1, 2][tie == 1] = 2.5                                          # 1 and 2 tie above 0 and 3 -> 1
    seg[1, 2][tie == 2] = 1.25
    seg[1, 3][tie == 2] = 1.25                                         # 2 and 3 tie -> 2;  tie == 0 / 3: all equal -> 0
    g_seg, g_ver = upstream(label, ncls, vn)
    got = run(N, place(seg, device), field(vertex, "network", device), place(label, device),
              field(target, "network", device), ncls, 1.0, g_seg, g_ver)
    assert np.isfinite(got["loss_seg"]).all() and np.isfinite(got["grad_seg"]).all()
    compare(got, seg, vertex, target, label, ncls, vn, 1.0, g_seg, g_ver, "logits of +-80, exact ties")
    pred = np.where(tie == 1, 1, np.where(tie == 2, 2, 0))
    for c in range(ncls):
        assert got["tp"][1, c] + got["fp"][1, c] == (pred == c + 1).sum()


# ---- 4. zero-weight elements are not used -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["network", "bhwk2"])
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
def test_zero_weight_elements_neither_loaded_nor_spread(device, N, dt, layout):
    b, H, W, ncls, vn = 3, 33, 67, 3, 9
    seg, vertex, target, label = make(51, b, H, W, ncls, vn, F32, dt, dt)
    label[0, :2, :5] = (ncls + 1, 255, 77, 0, 200)                     # ignored labels among them
    label[2] = 0
    w = np.broadcast_to(((label[..., None] - 1) == (np.arange(ncls * vn) // vn))[..., None], vertex.shape)
    g_seg, g_ver = upstream(label, ncls, vn)
    res = []
    for poison in (False, True):
        v, t = vertex.copy(), target.copy()
        v[~w], t[~w] = (np.nan, np.inf) if poison else (0, 0)
        if poison:
            t[~w & (np.arange(W)[None, None, :, None, None] % 2 == 1)] = np.nan
            v[~w & (np.arange(H)[None, :, None, None, None] % 2 == 1)] = -np.inf
        res.append(run(N, place(seg, device), field(v, layout, device), place(label, device), field(t, layout, device),
                       ncls, 2.0, g_seg, g_ver))
    for k in ("loss_seg", "loss_vertex", "grad_seg", "grad_vertex", "fg", "tp", "fp", "fn"):
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)
    assert np.isfinite(res[1]["loss_vertex"]).all() and (res[1]["loss_vertex"][:2] > 0).all()
    assert (R.logical(res[1]["grad_vertex"], ncls)[~w] == 0).all()
    compare(res[1], seg, vertex, target, label, ncls, vn, 2.0, g_seg, g_ver, f"poisoned {dt} {layout}")


# ---- 5. autograd ----------------------------------------------------------------------------------------------------
def test_autograd_through_the_means(device, N):
    b, H, W, ncls, vn = 3, 33, 67, 3, 9
    seg, vertex, target, label = make(61, b, H, W, ncls, vn)
    label[1] = 0
    ts, tv = place(seg, device).requires_grad_(), field(vertex, "network", device).requires_grad_()
    lab, tgt = place(label.astype(np.uint8), device), field(target, "bhwk2", device)
    ls, lv, st = N.pvnet_loss(ts, tv, lab, tgt, ncls, 1.0)
    assert ls.requires_grad and lv.requires_grad and not any(v.requires_grad for v in st.values())
    (ls.mean() + 0.5 * lv.mean()).backward()
    g_seg, g_ver = np.full(b, np.float32(1) / np.float32(b)), np.full(b, np.float32(0.5) / np.float32(b))
    gs, gv = R.backward(seg, vertex, target, label, ncls, vn, 1.0, g_seg, g_ver)
    fg = ((label >= 1) & (label <= ncls)).reshape(b, -1).sum(1)
    print("autograd through the means:")
    report("grad_seg", np.abs(ts.grad.cpu().numpy() - gs), 16 * U * g_seg[0] / (H * W) + np.zeros_like(gs))
    report("grad_vertex", np.abs(R.logical(tv.grad.cpu().numpy(), ncls) - gv),
           (16 * U * g_ver / (2.0 * vn * fg + 1e-3))[:, None, None, None, None] + np.zeros_like(gv))
    # a second call with non-uniform upstream gradients, zero included; only one prediction wants a gradient
    g_seg, g_ver = np.array([0.0, 2.0, -1.5], np.float32), np.array([3.0, 1.0, 0.0], np.float32)
    got = run(N, place(seg, device), field(vertex, "network", device), lab, tgt, ncls, 1.0, g_seg, g_ver)
    compare(got, seg, vertex, target, label, ncls, vn, 1.0, g_seg, g_ver, "non-uniform upstream gradients")
    assert (got["grad_seg"][0] == 0).all() and (got["grad_vertex"][2] == 0).all()
    tv2 = field(vertex, "network", device).requires_grad_()
    ls, lv, _ = N.pvnet_loss(place(seg, device), tv2, lab, tgt, ncls, 1.0)
    assert not ls.requires_grad and lv.requires_grad
    (lv * torch.as_tensor(g_ver, device=device)).sum().backward()
    np.testing.assert_array_equal(tv2.grad.cpu().numpy(), got["grad_vertex"])


# ---- 6. determinism and graphs --------------------------------------------------------------------------------------
def test_two_runs_and_two_replays_give_the_same_bits(device, N):
    b, H, W, ncls, vn = 2, 480, 640, 1, 9
    rng = np.random.default_rng(71)
    seg = torch.from_numpy(rng.normal(0, 3, (b, 2, H, W)).astype(np.float16)).to(device)
    ver = torch.from_numpy(rng.normal(0, 1, (b, 2 * vn, H, W)).astype(np.float16)).to(device)
    tgt = torch.from_numpy(rng.normal(0, 0.7, (b, 2 * vn, H, W)).astype(np.float16)).to(device)
    yy, xx = np.mgrid[:H, :W]
    label = np.stack([((yy - 200 - 40 * i) ** 2 + (xx - 300) ** 2 < 110 ** 2) for i in range(b)]).astype(np.uint8)
    lab = torch.from_numpy(label).to(device)
    g = torch.tensor([float(H * W), 0.5 * H * W], device=device)

    def step(seg_in, ver_in):
        ls, lv, st = N.pvnet_loss(seg_in, ver_in, lab, tgt, ncls, 1.0)
        gs, gv = torch.autograd.grad([(ls * g).sum() + (lv * g).sum()], [seg_in, ver_in])
        return [ls, lv, gs, gv, st["fg"], st["tp"], st["fp"], st["fn"]]

    seg_in, ver_in = seg.clone().requires_grad_(), ver.clone().requires_grad_()
    first = [t.detach().cpu().numpy() for t in step(seg_in, ver_in)]
    second = [t.detach().cpu().numpy() for t in step(seg_in, ver_in)]
    for x, y in zip(first, second):
        np.testing.assert_array_equal(x, y)
    assert first[4].tolist() == label.reshape(b, -1).sum(1).tolist() and np.abs(first[3]).max() > 0
    # many blocks: the order of the partials is the shapes' alone, so a third of the value is not noise
    ref = R.forward(seg.cpu().numpy(), ver.cpu().numpy(), tgt.cpu().numpy(), label, ncls, vn, 1.0)
    print("2 x 480 x 640:")
    report("loss_seg", np.abs(first[0] - ref["loss_seg"]), 32 * U * (1 + float(seg.abs().max())))
    report("loss_vertex", np.abs(first[1] - ref["loss_vertex"]), 16 * U * ref["loss_vertex"] + 1e-12)
    # captured on a side stream (the workspace comes from the graph's pool) and replayed twice
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gph, stream=side):
            outs = step(seg_in, ver_in)
    for _ in range(2):
        for t in outs:
            t.detach().fill_(77)
        gph.replay()
        torch.cuda.synchronize()
        for x, t in zip(first, outs):
            np.testing.assert_array_equal(x, t.detach().cpu().numpy())


# ---- 7. the reference-named wrappers ----------------------------------------------------------------------------------
def test_reference_named_wrappers_equal_the_pieces(device, N):
    b, H, W, vn = 3, 33, 67, 9
    seg, vertex, target, label = make(81, b, H, W, 1, vn)
    ts, tv = place(seg, device), field(vertex, "network", device)
    lab, tgt = place(label.astype(np.uint8), device), field(target, "network", device)
    got = run(N, ts, tv, lab, tgt, 1, 2.0, np.zeros(b, np.float32), np.ones(b, np.float32))
    weights = (lab[:, None] != 0).float() * 3.0                        # non-zero means foreground
    tv2 = tv.clone().requires_grad_()
    per_image = N.smooth_l1_loss(tv2, tgt, weights, sigma=2.0, normalize=True, reduce=False)
    np.testing.assert_array_equal(per_image.detach().cpu().numpy(), got["loss_vertex"])
    per_image.sum().backward()
    np.testing.assert_array_equal(tv2.grad.cpu().numpy(), got["grad_vertex"])
    mean = N.smooth_l1_loss(tv, tgt, weights, sigma=2.0)
    assert mean.shape == () and float(mean) == float(per_image.detach().mean())
    precision, recall = N.compute_precision_recall(ts, lab)
    np.testing.assert_array_equal(precision.cpu().numpy(), got["precision"][:, 0])
    np.testing.assert_array_equal(recall.cpu().numpy(), got["recall"][:, 0])
    pm, rm = N.compute_precision_recall(ts, lab.long(), reduce=True)
    assert float(pm) == float(precision.mean()) and float(rm) == float(recall.mean())
    with pytest.raises(NotImplementedError):
        N.smooth_l1_loss(tv, tgt, weights, normalize=False)


# ---- 8. the loop closes ---------------------------------------------------------------------------------------------
def test_one_gradient_step_reaches_the_ground_truth(device, N):
    from pvnet_amd import render as Rn
    H, W, ncls, vn = 96, 128, 2, 9
    models = [RR.bumpy_ellipsoid(2), RR.box(0.05, 0.04, 0.03)]
    p3 = np.stack([RR.spread_keypoints(m[0], 8) for m in models])
    rng = np.random.default_rng(9)
    t = [[(-0.06, -0.02, 0.45), (0.07, 0.03, 0.5)], [(0.0, 0.0, 0.5), (0.03, 0.01, 0.42)]]
    poses = np.array([[RR.pose(RR.random_rotation(rng), t[i][c]) for c in range(2)] for i in range(2)])
    K = np.array([[150.0, 0.0, 63.5], [0.0, 150.0, 47.5], [0.0, 0.0, 1.0]])
    table = Rn.MeshTable(models, device=device)
    label, target, _ = Rn.render_ground_truth(table, p3, torch.from_numpy(poses).to(device),
                                              torch.tensor([0, 1], dtype=torch.int32, device=device),
                                              torch.from_numpy(K).to(device), H, W, layout="network")
    b = label.shape[0]
    fg = torch.stack([((label >= 1) & (label <= ncls))[i].sum() for i in range(b)])
    assert (fg > 100).all() and tuple(target.shape) == (b, 2 * ncls * vn, H, W)
    seg = torch.zeros((b, ncls + 1, H, W), device=device, requires_grad=True)
    ver = torch.zeros((b, 2 * ncls * vn, H, W), device=device, requires_grad=True)
    ls0, lv0, st0 = N.pvnet_loss(seg, ver, label, target, ncls)
    assert (st0["fg"] == fg).all() and (st0["tp"] == 0).all() and (st0["fn"].sum(1) == fg).all()
    (ls0.sum() + lv0.sum()).backward()
    lr_ver = (2.0 * vn * fg.double() + 1e-3).float()[:, None, None, None]
    with torch.no_grad():
        ver1 = ver - lr_ver * ver.grad
        seg1 = seg - float(H * W) * seg.grad
    # the field equals the target on every foreground element: in the quadratic region the step is
    # exactly -d, and at |d| = 1 the linear branch gives the same step
    cls = torch.arange(ncls * vn, device=device) // vn
    w = ((label.long()[..., None] - 1) == cls)                         # [b, H, W, C]
    w = w.permute(0, 3, 1, 2).repeat_interleave(2, 1)                  # the network's channels
    err = (ver1 - target).abs()[w]
    print(f"the loop closes:\n  field - target on the foreground: max {float(err.max()) / U:.2f} u (bound 4 u)")
    assert float(err.max()) <= 4 * U and (ver1[~w] == 0).all()
    ls1, lv1, st1 = N.pvnet_loss(seg1, ver1, label, target, ncls)
    inr = label <= ncls
    assert (seg1.argmax(1)[inr] == label.long()[inr]).all()
    per_class = torch.stack([(label == c + 1).flatten(1).sum(1) for c in range(ncls)], 1)
    assert (st1["tp"] == per_class).all() and (st1["tp"].sum(1) == fg).all()
    assert (st1["fp"] == 0).all() and (st1["fn"] == 0).all()
    assert (ls1 < ls0).all() and (lv1 < lv0).all()
