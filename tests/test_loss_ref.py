"""tests/loss_ref.py (the numpy float64 restatement of include/pvloss.h) against torch on the CPU in
float64: F.cross_entropy with ignore_index and its view-mean, the reference's smooth-L1 written with
torch ops, autograd for both gradients; and a central-difference check of the restated gradient.
This pins the yardstick of the device tests without the reference tree."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_ref as R

RTOL = 1e-12


def make_case(seed, b, H, W, ncls, vn, out_of_range=False, empty_image=False, edge_sigma=None):
    rng = np.random.default_rng(seed)
    seg = rng.normal(0, 3, (b, ncls + 1, H, W))
    vertex = rng.normal(0, 1.2, (b, H, W, ncls * vn, 2))
    target = rng.normal(0, 0.7, (b, H, W, ncls * vn, 2))
    label = rng.integers(0, ncls + 1, (b, H, W)).astype(np.int64)
    if out_of_range:
        label[0, 0, :3] = (ncls + 1, 255, -1)
        label[-1, -1, -1] = -7
    if empty_image:
        label[b - 1] = 0
    if edge_sigma is not None:
        # |d| exactly at 1 / sigma^2 and one step of the last place to either side, both signs, on
        # foreground pixels (the target there is 0: the difference is the value itself)
        t = 1.0 / (edge_sigma * edge_sigma)
        label[0, 0, :] = 1
        target[0, 0, :, :vn] = 0.0
        steps = np.array([t, -t, np.nextafter(t, 0), np.nextafter(t, 2), -np.nextafter(t, 0), -np.nextafter(t, 2)])
        for x in range(W):
            vertex[0, 0, x, :vn, :] = steps[(x + np.arange(vn)[:, None] + np.arange(2)[None]) % len(steps)]
    return seg, vertex, target, label


def torch_objective(seg, vertex, target, label, ncls, vn, sigma):
    """-> (loss_seg [b], loss_vertex [b]) of float64 CPU tensors, the way the reference composes them."""
    b, _, H, W = seg.shape
    lab = label.long()
    inr = (lab >= 0) & (lab <= ncls)
    ce = F.cross_entropy(seg, torch.where(inr, lab, torch.full_like(lab, -100)), reduction="none", ignore_index=-100)
    loss_seg = ce.view(b, -1).mean(1)
    cls = torch.arange(ncls * vn) // vn
    w = ((lab[..., None] - 1) == cls)[..., None]                       # [b, H, W, C, 1]
    sigma2 = sigma ** 2
    diff = torch.where(w, vertex - target, torch.zeros((), dtype=vertex.dtype))
    ad = diff.abs()
    quad = (ad < 1.0 / sigma2).detach().to(vertex.dtype)
    in_loss = diff ** 2 * (sigma2 / 2.0) * quad + (ad - 0.5 / sigma2) * (1.0 - quad)
    in_loss = torch.where(w, in_loss, torch.zeros((), dtype=vertex.dtype))
    fg = ((lab >= 1) & (lab <= ncls)).view(b, -1).sum(1).to(vertex.dtype)
    loss_vertex = in_loss.view(b, -1).sum(1) / (2 * vn * fg + 1e-3)
    return loss_seg, loss_vertex


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    tol = RTOL * np.maximum(np.abs(b), np.abs(a))
    assert (err <= tol).all(), f"{what}: max error {err.max():.3e} beyond {RTOL} relative"


CASES = [
    dict(b=2, H=5, W=7, ncls=1, vn=1),
    dict(b=2, H=6, W=9, ncls=1, vn=9, out_of_range=True),
    dict(b=3, H=5, W=8, ncls=3, vn=2, out_of_range=True, empty_image=True),
    dict(b=2, H=4, W=12, ncls=3, vn=9, empty_image=True),
    dict(b=1, H=3, W=12, ncls=1, vn=3, edge_sigma=1.0),
    dict(b=2, H=3, W=12, ncls=3, vn=2, edge_sigma=2.0, out_of_range=True),
]


@pytest.mark.parametrize("sigma", [1.0, 2.0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_restatement_matches_torch_f64(case, sigma):
    kw = dict(case)
    if kw.get("edge_sigma") is not None and kw["edge_sigma"] != sigma:
        kw["edge_sigma"] = sigma
    ncls, vn = kw["ncls"], kw["vn"]
    seg, vertex, target, label = make_case(11, **kw)
    b = seg.shape[0]
    ref = R.forward(seg, vertex, target, label, ncls, vn, sigma)
    ts = torch.tensor(seg, requires_grad=True)
    tv = torch.tensor(vertex, requires_grad=True)
    ls, lv = torch_objective(ts, tv, torch.tensor(target), torch.tensor(label), ncls, vn, sigma)
    close(ref["loss_seg"], ls.detach().numpy(), "loss_seg")
    close(ref["loss_vertex"], lv.detach().numpy(), "loss_vertex")
    fg = ((label >= 1) & (label <= ncls)).reshape(b, -1).sum(1)
    assert (ref["fg"] == fg).all()
    if kw.get("empty_image"):
        assert ref["fg"][-1] == 0 and ref["loss_vertex"][-1] == 0.0
    # the counts against the reference's compute_precision_recall products, per class
    pred = torch.argmax(ts.detach(), 1).numpy()
    for c in range(ncls):
        p, t = (pred == c + 1).astype(np.float64), (label == c + 1).astype(np.float64)
        want = [(p * t).reshape(b, -1).sum(1), (p * (1 - t)).reshape(b, -1).sum(1), ((1 - p) * t).reshape(b, -1).sum(1)]
        assert (ref["counts"][:, c] == np.stack(want, 1)).all()
    # gradients with non-uniform upstream gradients, zero included
    g_seg = np.linspace(0.0, 2.0, b) if b > 1 else np.array([0.75])
    g_vertex = np.linspace(1.5, 0.0, b) if b > 1 else np.array([1.25])
    (ls * torch.tensor(g_seg)).sum().backward()
    (lv * torch.tensor(g_vertex)).sum().backward()
    gs, gv = R.backward(seg, vertex, target, label, ncls, vn, sigma, g_seg, g_vertex)
    close(gs, ts.grad.numpy(), "grad_seg")
    close(gv, tv.grad.numpy(), "grad_vertex")
    # a zero weight is an exact zero
    w = ((label[..., None] - 1) == (np.arange(ncls * vn) // vn))[..., None]
    assert (gv[~np.broadcast_to(w, gv.shape)] == 0).all()
    assert (gs[np.broadcast_to(((label < 0) | (label > ncls))[:, None], gs.shape)] == 0).all()


def test_either_layout_and_absent_terms():
    seg, vertex, target, label = make_case(5, 2, 4, 6, 3, 2, out_of_range=True)
    full = R.forward(seg, vertex, target, label, 3, 2, 2.0)
    net = R.forward(seg, R.network(vertex), R.network(target), label, 3, 2, 2.0)
    assert (full["loss_vertex"] == net["loss_vertex"]).all() and (R.logical(R.network(vertex), 3) == vertex).all()
    only_seg = R.forward(seg, None, None, label, 3, 2)
    only_vtx = R.forward(None, vertex, target, label, 3, 2, 2.0)
    assert only_seg["loss_vertex"] is None and only_vtx["loss_seg"] is None and only_vtx["counts"] is None
    assert (only_seg["loss_seg"] == full["loss_seg"]).all() and (only_vtx["loss_vertex"] == full["loss_vertex"]).all()
    assert (only_seg["fg"] == full["fg"]).all() and (only_seg["counts"] == full["counts"]).all()


def test_zero_weight_elements_do_not_spread():
    seg, vertex, target, label = make_case(6, 2, 4, 6, 3, 2, out_of_range=True, empty_image=True)
    w = np.broadcast_to(((label[..., None] - 1) == (np.arange(6) // 2))[..., None], vertex.shape)
    v2, t2 = vertex.copy(), target.copy()
    v2[~w] = np.nan
    t2[~w] = np.inf
    a, bb = R.forward(None, vertex, target, label, 3, 2), R.forward(None, v2, t2, label, 3, 2)
    assert (a["loss_vertex"] == bb["loss_vertex"]).all()
    ga, gb = R.backward(None, vertex, target, label, 3, 2)[1], R.backward(None, v2, t2, label, 3, 2)[1]
    assert (ga == gb).all() and (gb[~w] == 0).all()


def test_restated_gradient_by_central_differences():
    ncls, vn, sigma = 2, 2, 2.0
    seg, vertex, target, label = make_case(3, 1, 3, 4, ncls, vn)
    label[0, 0, 0] = 9                                                 # one ignored pixel
    g_seg, g_vertex = np.array([1.7]), np.array([0.6])

    def objective(s, v):
        o = R.forward(s, v, target, label, ncls, vn, sigma)
        return float((o["loss_seg"] * g_seg).sum() + (o["loss_vertex"] * g_vertex).sum())

    gs, gv = R.backward(seg, vertex, target, label, ncls, vn, sigma, g_seg, g_vertex)
    h = 1e-6
    for arr, grad, which in ((seg, gs, 0), (vertex, gv, 1)):
        num = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            up = objective(seg, vertex)
            arr[idx] = keep - h
            dn = objective(seg, vertex)
            arr[idx] = keep
            num[idx] = (up - dn) / (2 * h)
        # the objective is smooth away from |d| = 1 / sigma^2, which no random element sits within h of
        d = np.abs(vertex - target)
        assert (np.abs(d - 1.0 / sigma ** 2) > 10 * h).all()
        assert np.abs(num - grad).max() <= 1e-8, ("seg", "vertex")[which]
