"""The memory contract of the C entries, held through ctypes on guarded buffers
(tests/guarded.py).  Every case:

  W  all outputs and the workspace sit between 64 KiB patterned guards, the workspace is exactly
     pv_*_workspace_size(...) bytes and that number is what the call is told: no guard byte changes;
  D  the workspace prefilled with 0x00, 0xFF and 0xA5 gives the same bits;
  R  every input surrounded by 0x00 and by 0xFF (a NaN as f16 / f32 / f64, -1 as an integer, label 255)
     gives the same bits;
  I  no input and no surround changes;
  P  the 0x00 run equals the reference of the library's own GPU test, at that test's tolerance,

after two plain runs gave the same bits (pv_ransac_motion_voting alone may differ, within the bound
tests/test_gpu_tail_stages.py derives for it).  An output's bytes start as 0xCD, so elements a call
documents as not written compare equal too.  Shapes are the smallest that reach the edge named beside
them; the block structure they rely on is asserted from the headers' constants.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import augment_ref as AR
from tests import loss_ref as LR
from tests import model_ref as MR
from tests import render_ref as RR
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_FILL = 0xCD
TORCH = {np.dtype(k): v for k, v in {np.uint8: torch.uint8, np.int32: torch.int32, np.int64: torch.int64,
                                     np.float16: torch.float16, np.float32: torch.float32,
                                     np.float64: torch.float64}.items()}
LABEL_NP = {"u8": np.uint8, "i32": np.int32, "i64": np.int64}
LABEL_KIND = {"i64": 0, "u8": 1, "i32": 2}                      # PV_LABEL_* / PV_LOSS_LABEL_* / PV_AUG_LABEL_*


@pytest.fixture(scope="module", autouse=True)
def built(device):
    import __graft_entry__ as g
    g.build()


def defines(header):
    """The integer #defines of a public header, as the test_*_abi.py files parse them."""
    src = open(os.path.join(REPO, "include", header)).read()
    return {k: int(v) for k, v in re.findall(r"#define (PV_[A-Z0-9_]+) \(?(-?\d+)u?\)?[ \t]*(?:/\*|\n)", src)}


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the driver
class Spec:
    """One call of one entry.

    inputs   name -> numpy array (placed with Guarded.inp)
    outputs  name -> (shape, numpy dtype[, byte offset[, numpy array]]): the array is the output's contents
             before the call (an in/out array such as the OR vote's bytes), else every byte is 0xCD
    ws       bytes of workspace, None for an entry that takes none
    call     (ptr: name -> device address, ws address or None, ws bytes, stream) -> the entry's return code
    check    the library's check(code, what)
    exact    False: two runs may differ in the last bits (close(a, b, what) then holds them)"""

    def __init__(self, name, inputs, outputs, call, check, ws=None, exact=True, close=None):
        self.name, self.inputs, self.outputs, self.call, self.check, self.ws = name, inputs, outputs, call, check, ws
        self.exact, self.close = exact, close


def execute(device, spec, surround=0x00, ws_fill=0x00):
    """One guarded run -> name -> numpy array of every output."""
    g = Guarded(device)
    ptr, outs = {}, {}
    for k, a in spec.inputs.items():
        ptr[k] = g.inp(a, surround=surround, name=f"input {k}").data_ptr()
    for k, o in spec.outputs.items():
        t = g.out(o[0], TORCH[np.dtype(o[1])], fill=OUT_FILL, offset=o[2] if len(o) > 2 else 0, name=f"output {k}")
        if len(o) > 3:
            t.copy_(torch.from_numpy(np.ascontiguousarray(o[3])))
        outs[k] = t
        ptr[k] = t.data_ptr()
    ws = None if spec.ws is None else g.workspace(spec.ws, fill=ws_fill, name="workspace")
    with torch.cuda.device(device):
        code = spec.call(ptr, None if ws is None else ws.data_ptr(), spec.ws or 0, torch.cuda.current_stream(device).cuda_stream)
    spec.check(code, spec.name)
    g.check()                                                   # W and I
    return {k: t.cpu().numpy() for k, t in outs.items()}


def same(a, b, what):
    for k in a:
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).reshape(-1).view(np.uint8),
                                      np.ascontiguousarray(b[k]).reshape(-1).view(np.uint8), err_msg=f"{what}: {k}")


def contract(device, spec, parity=None):
    """Calibration, W, D, R, I and P for one call -> the baseline run's outputs."""
    hold = same if spec.exact else spec.close
    base = execute(device, spec)
    hold(base, execute(device, spec), f"{spec.name}: two plain runs")
    if spec.ws is not None:
        assert spec.ws > 0
        for fill in (0xFF, 0xA5):
            hold(base, execute(device, spec, ws_fill=fill), f"{spec.name}: workspace prefilled with {fill:#04x}")
    hold(base, execute(device, spec, surround=0xFF), f"{spec.name}: inputs surrounded by 0xFF")
    if parity is not None:
        parity(base)
    return base


def untouched(a):
    """Is every byte of an output still the fill it started with?"""
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == OUT_FILL).all())


# ---------------------------------------------------------------- render: pv_render_labels
def render_scene(shape):
    """(models, frames, K): frames is a list per image of (model_id, label, Rt)."""
    from tests.test_gpu_render import K_SKEW, seeded_poses
    models = [RR.box(), RR.icosphere(1, 0.05)]
    I = np.eye(3)
    if shape == (1, 1, 1):                                      # a box face over the only sample, a sphere behind it
        K = np.array([[64.0, 0, 0.0], [0, 64.0, 0.0], [0, 0, 1]])
        return models, [[(0, 7, RR.pose(I, [0.01, 0.005, 0.5])), (1, 3, RR.pose(I, [0.0, 0.0, 0.9]))]], K
    if shape == (1, 5, 7):
        K = np.array([[9.0, 0.3, 3.1], [0, 9.5, 2.2], [0, 0, 1]])
        rot = seeded_poses(5, 1)[0][:, :3]
        return models, [[(1, 255, RR.pose(I, [-0.02, 0.0, 0.3])), (0, 1, RR.pose(rot, [0.03, 0.01, 0.26]))]], K
    rot = [p[:, :3] for p in seeded_poses(21, 3)]
    frames = [[(1, 1, RR.pose(I, [-0.01, 0.0, 0.40])), (0, 2, RR.pose(rot[0], [0.02, 0.01, 0.33]))],
              [],                                               # a frame with no instance: the background alone
              [(1, 9, RR.pose(I, [-0.03, 0.0, 0.40])), (7, 4, RR.pose(I, [0.0, 0.0, 0.4])),      # model 7: skipped whole
               (0, 200, RR.pose(rot[2], [0.0, 0.01, 0.36]))]]
    return models, frames, K_SKEW


@functools.lru_cache(maxsize=None)
def render_reference(shape):
    models, frames, K = render_scene(shape)
    b, H, W = shape
    return [RR.render(models, f, K, H, W) for f in frames]


@pytest.mark.parametrize("kind", ["u8", "i32", "i64"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (3, 37, 53)], ids=lambda s: "x".join(map(str, s)))
def test_render_labels(device, shape, kind):
    from pvnet_amd import _render_lib as P
    from tests.test_gpu_render import ulp_apart
    L = P.load()
    b, H, W = shape
    models, frames, K = render_scene(shape)
    # an odd pixel count: k_clear's two keys per lane end on a lane that holds one
    assert (b * H * W) % 2 == 1
    flat = [i for f in frames for i in f]
    n = len(flat)
    off = np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)
    ragged = len({len(f) for f in frames}) > 1
    verts = np.concatenate([m[0] for m in models]).astype(np.float32)
    faces = np.concatenate([m[1] for m in models]).astype(np.int32)
    voff = np.cumsum([0] + [len(m[0]) for m in models]).astype(np.int32)
    foff = np.cumsum([0] + [len(m[1]) for m in models]).astype(np.int32)
    max_v, max_f = max(len(m[0]) for m in models), max(len(m[1]) for m in models)
    inputs = dict(verts=verts, vert_off=voff, faces=faces, face_off=foff,
                  model_id=np.array([i[0] for i in flat], np.int32), label=np.array([i[1] for i in flat], np.int32),
                  pose=np.array([i[2] for i in flat], np.float64), K=np.asarray(K, np.float64))
    if ragged:
        inputs["inst_off"] = off
    # the instances' labels are the input `label`: the label map goes by label_out
    outputs = dict(label_out=((b, H, W), LABEL_NP[kind]), inst=((b, H, W), np.int32), depth=((b, H, W), np.float32),
                   snap_xy=((n, max_v, 2), np.int32), snap_z=((n, max_v), np.float64), won=((n,), np.int32))
    need = int(L.pv_render_workspace_size(b, H, W, n * max_v, n))

    def call(p, ws, nbytes, stream):
        m = P.RenderMeshes(p["verts"], p["vert_off"], p["faces"], p["face_off"], len(models), len(verts), len(faces),
                           max_v, max_f, 0)
        bt = P.RenderBatch(b, H, W, 0 if ragged else n // b, n, LABEL_KIND[kind], p.get("inst_off"), p["model_id"],
                           p["label"], p["pose"], p["K"], 0, 1e-3)
        ot = P.RenderOut(p["label_out"], p["inst"], p["depth"], p["snap_xy"], p["snap_z"], p["won"])
        return L.pv_render_labels(ctypes.byref(m), ctypes.byref(bt), ctypes.byref(ot), ws, nbytes, stream)

    def parity(got):
        refs = render_reference(shape)
        assert min(r["snap_margin"] for r in refs if np.isfinite(r["snap_margin"])) >= 1e-6   # conditions on the scene:
        assert all(r["depth_margin"] >= 1e-6 for r in refs)                                   # no snap and no depth tie
        for i, r in enumerate(refs):
            np.testing.assert_array_equal(got["label_out"][i], r["label"], err_msg=f"label, frame {i}")
            np.testing.assert_array_equal(got["inst"][i], r["inst"], err_msg=f"inst, frame {i}")
            assert ulp_apart(got["depth"][i], r["depth"]).max() <= 1, f"depth, frame {i}"
            np.testing.assert_array_equal(got["won"][off[i]:off[i + 1]], r["won"], err_msg=f"won, frame {i}")
            for j, s in enumerate(r["snap"]):
                row = off[i] + j
                if s is None:                                   # a skipped instance writes nothing
                    assert untouched(got["snap_xy"][row]) and untouched(got["snap_z"][row])
                    continue
                nv = len(s["Z"])
                np.testing.assert_array_equal(got["snap_xy"][row, :nv], s["sxy"])
                np.testing.assert_allclose(got["snap_z"][row, :nv], s["Z"], rtol=1e-15, atol=0)
                assert untouched(got["snap_xy"][row, nv:]) and untouched(got["snap_z"][row, nv:])
        assert sum(int(r["won"].sum()) for r in refs) > 0

    contract(device, Spec(f"pv_render_labels {shape} {kind}", inputs, outputs, call, P.check, ws=need), parity)


# ---------------------------------------------------------------- render: pv_vertex_field
FIELD_SHAPES = [(37, 53, 1, 1), (37, 53, 1, 9), (37, 53, 3, 9), (37, 53, 3, 1), (48, 64, 2, 9), (48, 64, 3, 9)]


@functools.lru_cache(maxsize=None)
def field_case(shape):
    """tests/test_gpu_render.py's field_cases entry for the shape: labels, keypoints, the f32 reference."""
    from tests.test_gpu_render import blob_labels
    H, W, ncls, vn = shape
    lab = blob_labels(2, H, W, ncls + 1, 50 + ncls * 10 + vn)
    rng = np.random.default_rng(ncls * 100 + vn)
    kp = rng.uniform([-10.0, -10.0], [W + 10.0, H + 10.0], size=(2, ncls, vn, 2))
    for i in range(2):
        for c in range(ncls):
            ys, xs = np.nonzero(lab[i] == c + 1)
            kp[i, c, 0] = (xs[len(xs) // 2], ys[len(ys) // 2])
    return lab, kp, np.stack([RR.vertex_field(lab[i], kp[i]) for i in range(2)])


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("layout", ["bhwk2", "network"])
@pytest.mark.parametrize("shape", FIELD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vertex_field(device, shape, layout, half):
    from pvnet_amd import _render_lib as P
    L = P.load()
    H, W, ncls, vn = shape
    C = ncls * vn
    lab, kp, ref = field_case(shape)
    kind = ("u8", "i32", "i64")[FIELD_SHAPES.index(shape) % 3]
    dt = np.float16 if half else np.float32
    if layout == "bhwk2":
        oshape, strides = (2, H, W, C, 2), (H * W * C * 2, W * C * 2, C * 2, 2, 1)
    else:
        oshape, strides = (2, 2 * C, H, W), (2 * C * H * W, W, 1, 2 * H * W, H * W)

    def call(p, ws, nbytes, stream):
        d = P.FieldDesc()
        d.label, d.keypoints, d.vertex = p["label"], p["keypoints"], p["vertex"]
        d.label_strides[:] = (H * W, W, 1)
        d.vertex_strides[:] = strides
        d.label_kind, d.kp_kind, d.vertex_kind = LABEL_KIND[kind], P.PV_KP_F64, P.PV_FIELD_F16 if half else P.PV_FIELD_F32
        d.b, d.H, d.W, d.ncls, d.vn = 2, H, W, ncls, vn
        return L.pv_vertex_field(ctypes.byref(d), stream)

    def parity(got):
        v = got["vertex"]
        if layout == "network":
            v = v.transpose(0, 2, 3, 1).reshape(2, H, W, C, 2)
        if half:
            want = ref.astype(np.float16)
            ulp = np.spacing(np.abs(want)).astype(np.float64)
            assert (np.abs(v.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        else:
            assert np.abs(v.astype(np.float64) - ref).max() <= 2.0 ** -23
        assert (v[ref == 0] == 0).all() and (ref == 0).mean() > 0.3

    spec = Spec(f"pv_vertex_field {shape} {layout}", dict(label=lab.astype(LABEL_NP[kind]), keypoints=kp),
                dict(vertex=(oshape, dt)), call, P.check)
    contract(device, spec, parity)


# ---------------------------------------------------------------- loss
LOSS_SHAPES = [(1, 1, 1, 1, 1), (1, 5, 7, 1, 1), (2, 37, 53, 3, 9)]


@functools.lru_cache(maxsize=None)
def loss_case(shape, half):
    """Inputs as tests/test_gpu_loss.py makes them, its upstream gradients and the f64 restatement."""
    from tests.test_gpu_loss import make, upstream
    b, H, W, ncls, vn = shape
    dt = torch.float16 if half else torch.float32
    seg, vertex, target, label = make(300 + H, b, H, W, ncls, vn, dt, dt, dt)
    if H * W > 1:
        label[0, -1, -1] = 1                                    # the frame's last pixel is weighted
        label[0, 0, 0] = ncls + 1                               # and one pixel is ignored
    g_seg, g_ver = upstream(label, ncls, vn)
    return seg, vertex, target, label, g_seg, g_ver, LR.forward(seg, vertex, target, label, ncls, vn, 1.0)["fg"]


def loss_desc(P, p, shape, half, kind, target_network):
    b, H, W, ncls, vn = shape
    C = ncls * vn
    net = (2 * C * H * W, W, 1, 2 * H * W, H * W)               # the logical [b][H][W][C][2] view of [b][2 C][H][W]
    dense = (H * W * C * 2, W * C * 2, C * 2, 2, 1)
    d = P.LossDesc()
    d.seg, d.vertex, d.target, d.label = p["seg"], p["vertex"], p["target"], p["label"]
    d.seg_strides[:] = ((ncls + 1) * H * W, H * W, W, 1)
    d.vertex_strides[:] = net
    d.target_strides[:] = net if target_network else dense
    d.label_strides[:] = (H * W, W, 1)
    d.seg_kind = d.vertex_kind = d.target_kind = P.PV_LOSS_F16 if half else P.PV_LOSS_F32
    d.label_kind = LABEL_KIND[kind]
    d.b, d.H, d.W, d.ncls, d.vn, d.sigma = b, H, W, ncls, vn, 1.0
    return d, net


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_forward_and_backward(device, shape, half):
    """The forward's partials are nblk * b per kind; (37, 53): 37 * ceil(53 / 8) = 259 lanes, two blocks an
    image, the second with three lanes.  The backward's gradients are dense guarded outputs."""
    from pvnet_amd import _loss_lib as P
    from tests.test_gpu_loss import compare
    L = P.load()
    h = defines("pvloss.h")
    b, H, W, ncls, vn = shape
    lanes = H * cdiv(W, h["PV_LOSS_PIXELS"])
    if (H, W) == (37, 53):
        assert (lanes, cdiv(lanes, h["PV_LOSS_THREADS"]), lanes % h["PV_LOSS_THREADS"]) == (259, 2, 3)
    else:
        assert lanes < h["PV_LOSS_THREADS"]
    seg, vertex, target, label, g_seg, g_ver, fg = loss_case(shape, half)
    kind = "i32" if half else "u8"
    target_network = not half                                   # f16: the target in the other layout
    dt = np.float16 if half else np.float32
    inputs = dict(seg=seg, vertex=LR.network(vertex), target=LR.network(target) if target_network else target,
                  label=label.astype(LABEL_NP[kind]))
    need = int(L.pv_loss_workspace_size(b, H, W, ncls))

    def forward(p, ws, nbytes, stream):
        d, _ = loss_desc(P, p, shape, half, kind, target_network)
        o = P.LossOut(p["loss_seg"], p["loss_vertex"], p["fg"], p["counts"])
        return L.pv_loss_forward(ctypes.byref(d), ctypes.byref(o), ws, nbytes, stream)

    def backward(p, ws, nbytes, stream):
        d, net = loss_desc(P, p, shape, half, kind, target_network)
        g = P.LossGrad()
        g.g_seg, g.g_vertex, g.fg, g.grad_seg, g.grad_vertex = p["g_seg"], p["g_vertex"], p["fg"], p["grad_seg"], p["grad_vertex"]
        g.grad_seg_strides[:] = ((ncls + 1) * H * W, H * W, W, 1)
        g.grad_vertex_strides[:] = net
        return L.pv_loss_backward(ctypes.byref(d), ctypes.byref(g), stream)

    fwd = contract(device, Spec(f"pv_loss_forward {shape}", inputs,
                                dict(loss_seg=((b,), np.float32), loss_vertex=((b,), np.float32), fg=((b,), np.int64),
                                     counts=((b, ncls, 3), np.int64)), forward, P.check, ws=need))
    bwd = contract(device, Spec(f"pv_loss_backward {shape}", dict(inputs, g_seg=g_seg, g_vertex=g_ver, fg=fg),
                                dict(grad_seg=(seg.shape, dt), grad_vertex=((b, 2 * ncls * vn, H, W), dt)), backward, P.check))
    tp, fp, fn = (fwd["counts"][..., j] for j in range(3))
    tpf, fpf, fnf = (x.astype(np.float32) for x in (tp, fp, fn))
    got = dict(fwd, **bwd, tp=tp, fp=fp, fn=fn, precision=(tpf + 1) / (tpf + fpf + 1), recall=(tpf + 1) / (tpf + fnf + 1))
    compare(got, seg, vertex, target, label, ncls, vn, 1.0, g_seg, g_ver, f"memory contract {shape} f16={half}")


# ---------------------------------------------------------------- augment
AUG_SHAPES = [(1, 1, 1, 1, 1), (2, 6, 10, 5, 9), (2, 40, 56, 37, 53)]
AUG_KINDS = [("u8", False), ("i32", True), ("i64", False), ("u8", True)]       # (label kind, f16 output)
AUG_KW = dict(rot_deg=(-180.0, 180.0), scale=(0.6, 1.7), margin=0.2, jitter=(0.4, 0.4, 0.4, 0.3))
AUG_SEED, AUG_FIRST = 0x0123456789ABCDEF, 2 ** 64 - 1           # the sample index wraps inside a batch of two


@functools.lru_cache(maxsize=None)
def aug_scene(shape):
    b, H, W, Ho, Wo = shape
    rng = np.random.default_rng([H, W, Ho, Wo])
    image = rng.integers(0, 256, (b, H, W, 3), dtype=np.uint8)
    label = rng.integers(0, 4, (b, H, W)).astype(np.int64)
    label[:, -1, -1] = 2                                        # the last pixel is foreground
    if b > 1:
        label[1] = np.where(label[1] > 0, 9, 0)                 # an image without foreground of the 3 classes
    background = rng.integers(0, 256, (b, Ho, Wo, 3), dtype=np.uint8)
    stats = AR.label_stats(label, 3)
    fwd, inv, color, _ = AR.params(stats, AUG_SEED, AUG_FIRST, H, W, Ho, Wo, **AUG_KW)
    return dict(image=image, label=label, background=background, stats=stats, fwd=fwd, inv=inv, color=color)


@pytest.mark.parametrize("kind", ["u8", "i32", "i64"])
@pytest.mark.parametrize("shape", AUG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_stats(device, shape, kind):
    from pvnet_amd import _augment_lib as P
    L = P.load()
    b, H, W, _, _ = shape
    s = aug_scene(shape)

    def call(p, ws, nbytes, stream):
        d = P.AugLabel(p["label"], (ctypes.c_int64 * 3)(H * W, W, 1), LABEL_KIND[kind], b, H, W)
        return L.pv_label_stats(ctypes.byref(d), 3, p["stats"], stream)

    def parity(got):
        np.testing.assert_array_equal(got["stats"], s["stats"])

    label = np.where(s["label"] == 9, 200, s["label"]).astype(LABEL_NP[kind])
    contract(device, Spec(f"pv_label_stats {shape} {kind}", dict(label=label), dict(stats=((b, 8), np.int64)), call, P.check),
             parity)


@pytest.mark.parametrize("shape", AUG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_augment_params(device, shape):
    from pvnet_amd import _augment_lib as P
    L = P.load()
    b, H, W, Ho, Wo = shape
    s = aug_scene(shape)

    def call(p, ws, nbytes, stream):
        r = P.AugRanges((ctypes.c_double * 2)(*AUG_KW["rot_deg"]), (ctypes.c_double * 2)(*AUG_KW["scale"]), AUG_KW["margin"],
                        (ctypes.c_double * 4)(*AUG_KW["jitter"]), b, H, W, Ho, Wo, 0)
        return L.pv_augment_params(ctypes.byref(r), p["stats"], p["state"], p["fwd"], p["inv"], p["color"], stream)

    def parity(got):
        # tests/test_gpu_augment.py::test_params_draws_and_matrices: the draws bit-equal, the matrices to the
        # device's cos and sin
        np.testing.assert_array_equal(got["color"], s["color"])
        for k in ("fwd", "inv"):
            assert (np.abs(got[k] - s[k]) <= 1e-12 * np.abs(s[k]).max((1, 2), keepdims=True)).all(), k

    state = np.array([AUG_SEED, AUG_FIRST], np.uint64).view(np.int64)
    contract(device, Spec(f"pv_augment_params {shape}", dict(stats=s["stats"], state=state),
                          dict(fwd=((b, 2, 3), np.float64), inv=((b, 2, 3), np.float64), color=((b, 4), np.float32)),
                          call, P.check), parity)


@pytest.mark.parametrize("kind,half", AUG_KINDS, ids=[f"{k}-{'f16' if h else 'f32'}" for k, h in AUG_KINDS])
@pytest.mark.parametrize("contrast", [True, False], ids=["contrast", "no_contrast"])
@pytest.mark.parametrize("shape", AUG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_augment_apply(device, shape, contrast, kind, half):
    """(37, 53) outputs: 37 * ceil(53 / 8) = 259 lanes, two blocks an image, the second with three lanes;
    the contrast step alone uses the workspace (one partial per block and image)."""
    from pvnet_amd import _augment_lib as P
    from tests.test_gpu_augment import FILL, MEAN, STD, check_image
    L = P.load()
    h = defines("pvaugment.h")
    b, H, W, Ho, Wo = shape
    lanes = Ho * cdiv(Wo, h["PV_AUG_PIXELS"])
    if (Ho, Wo) == (37, 53):
        assert (lanes, cdiv(lanes, h["PV_AUG_THREADS"]), lanes % h["PV_AUG_THREADS"]) == (259, 2, 3)
    else:
        assert lanes < h["PV_AUG_THREADS"]
    s = aug_scene(shape)
    flags = AR.ALL if contrast else AR.ALL & ~AR.CONTRAST
    assert h["PV_AUG_CONTRAST"] == AR.CONTRAST
    label = np.where(s["label"] == 9, 200, s["label"]).astype(LABEL_NP[kind])
    need = int(L.pv_augment_workspace_size(b, Ho, Wo)) if contrast else None

    def call(p, ws, nbytes, stream):
        d = P.AugDesc()
        d.image, d.label, d.inv, d.color, d.background = p["image"], p["label"], p["inv"], p["color"], p["background"]
        d.out_image, d.out_label = p["out_image"], p["out_label"]
        d.image_strides[:] = (H * W * 3, W * 3, 3, 1)
        d.label_strides[:] = (H * W, W, 1)
        d.background_strides[:] = (Ho * Wo * 3, Wo * 3, 3, 1)
        d.out_image_strides[:] = (3 * Ho * Wo, Ho * Wo, Wo, 1)
        d.out_label_strides[:] = (Ho * Wo, Wo, 1)
        d.fill[:], d.mean[:], d.std[:] = FILL, MEAN, STD
        d.label_kind, d.out_kind, d.flags = LABEL_KIND[kind], P.PV_AUG_F16 if half else P.PV_AUG_F32, flags
        d.b, d.H, d.W, d.Ho, d.Wo = b, H, W, Ho, Wo
        return L.pv_augment_apply(ctypes.byref(d), ws, nbytes, stream)

    def parity(got):
        ref, ref_lab = AR.apply(s["image"], label, s["inv"], s["color"], Ho, Wo, s["background"], FILL, MEAN, STD, flags)
        np.testing.assert_array_equal(got["out_label"], ref_lab)
        check_image(f"memory contract {shape} flags {flags} f16 {half}", got["out_image"].astype(np.float64), ref, s["color"],
                    flags, half)

    spec = Spec(f"pv_augment_apply {shape} flags {flags}",
                dict(image=s["image"], label=label, inv=s["inv"], color=s["color"], background=s["background"]),
                dict(out_image=((b, 3, Ho, Wo), np.float16 if half else np.float32), out_label=((b, Ho, Wo), LABEL_NP[kind])),
                call, P.check, ws=need)
    contract(device, spec, parity)


# ---------------------------------------------------------------- model preparation
@functools.lru_cache(maxsize=None)
def model_table(which):
    """(points f32 [total, 3], off i32, max_pn, start_idx, the diameters where they are known without n^2 work)."""
    rng = np.random.default_rng(17)
    if which == "small":
        sizes = [1, MR.TILE, MR.TILE + 1]
        models = [rng.normal(size=(n, 3)).astype(np.float32) for n in sizes]
        known = None
    else:
        from tests.test_gpu_model import ball
        n = MR.BLOCK_MAX_PN + 1                                 # the per-step form, two chunks
        big = ball(rng, n)
        big[n // 3], big[n - 1] = [2.0, 0.0, 0.0], [-2.0, 0.0, 0.0]     # every other pair is at most 3 apart
        models = [rng.normal(size=(5, 3)).astype(np.float32), big]
        sizes = [5, n]
        known = {1: 4.0}
    off = np.cumsum([0] + sizes).astype(np.int32)
    return np.concatenate(models), off, max(sizes), np.array([s - 1 for s in sizes], np.int32), known


def model_points(P, p, points, off, max_pn):
    return P.ModelPoints(p["points"], p["off"], len(off) - 1, len(points), max_pn, 0)


@pytest.mark.parametrize("which", ["small", "large"])
def test_model_extent_and_diameter(device, which):
    from pvnet_amd import _model_lib as P
    from tests.test_gpu_model import same_bits
    L = P.load()
    h = defines("pvmodel.h")
    points, off, max_pn, _, known = model_table(which)
    nm = len(off) - 1
    sizes = np.diff(off)
    if which == "small":                                        # 257 points: two tiles, three tile pairs
        assert sizes.tolist() == [1, h["PV_MODEL_TILE"], h["PV_MODEL_TILE"] + 1] and cdiv(257, h["PV_MODEL_TILE"]) == 2
    else:
        assert sizes.tolist() == [5, h["PV_MODEL_BLOCK_MAX_PN"] + 1] and cdiv(int(sizes[1]), h["PV_MODEL_CHUNK"]) == 2
    inputs = dict(points=points, off=off)

    def extent(p, ws, nbytes, stream):
        mp = model_points(P, p, points, off, max_pn)
        return L.pv_model_extent(ctypes.byref(mp), p["bbox"], p["centroid"], p["count"], stream)

    def diameter(p, ws, nbytes, stream):
        mp = model_points(P, p, points, off, max_pn)
        return L.pv_model_diameter(ctypes.byref(mp), p["diameter"], ws, nbytes, stream)

    def extent_parity(got):
        ref = MR.table_extent(points, off, max_pn)
        np.testing.assert_array_equal(got["count"], ref["count"])
        same_bits(got["bbox"][:, 0], ref["bbox_min"], "bbox_min")
        same_bits(got["bbox"][:, 1], ref["bbox_max"], "bbox_max")
        same_bits(got["centroid"], ref["centroid"], "centroid")

    def diameter_parity(got):
        want = [known[m] if known and m in known else MR.diameter(MR.model_rows(points, off, m, max_pn)) for m in range(nm)]
        same_bits(got["diameter"], np.array(want), "diameter")

    contract(device, Spec(f"pv_model_extent {which}", inputs, dict(bbox=((nm, 2, 3), np.float64), centroid=((nm, 3), np.float64),
                                                                   count=((nm,), np.int32)), extent, P.check), extent_parity)
    need = int(L.pv_model_workspace_size(nm, len(points), 1))
    contract(device, Spec(f"pv_model_diameter {which}", inputs, dict(diameter=((nm,), np.float64)), diameter, P.check, ws=need),
             diameter_parity)


@pytest.mark.parametrize("start", [MR.START_CENTROID, MR.START_CENTROID_KEPT, MR.START_INDEX], ids=["centroid", "kept", "index"])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("which", ["small", "large"])
def test_farthest_points(device, which, k, start):
    from pvnet_amd import _model_lib as P
    from tests.test_gpu_model import same_bits
    L = P.load()
    h = defines("pvmodel.h")
    assert (h["PV_FPS_START_CENTROID"], h["PV_FPS_START_CENTROID_KEPT"], h["PV_FPS_START_INDEX"]) == \
        (MR.START_CENTROID, MR.START_CENTROID_KEPT, MR.START_INDEX)
    points, off, max_pn, sidx, _ = model_table(which)
    nm = len(off) - 1
    inputs = dict(points=points, off=off)
    if start == MR.START_INDEX:
        inputs["start_idx"] = sidx
    need = int(L.pv_model_workspace_size(nm, len(points), k))

    def call(p, ws, nbytes, stream):
        mp = model_points(P, p, points, off, max_pn)
        return L.pv_farthest_points(ctypes.byref(mp), k, start, p.get("start_idx"), p["idx"], p["picked"], p["pick_d2"], ws,
                                    nbytes, stream)

    def parity(got):
        ref = MR.table_farthest_points(points, off, max_pn, k, start, sidx if start == MR.START_INDEX else None)
        np.testing.assert_array_equal(got["idx"], ref["idx"])
        same_bits(got["picked"], ref["picked"], "picked")
        same_bits(got["pick_d2"], ref["pick_d2"], "pick_d2")

    contract(device, Spec(f"pv_farthest_points {which} k={k} start={start}", inputs,
                          dict(idx=((nm, k), np.int32), picked=((nm, k, 3), np.float64), pick_d2=((nm, k), np.float64)),
                          call, P.check, ws=need), parity)


# ---------------------------------------------------------------- evaluation
@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (3, 65, 513, 3), (2, 513, 511, 2)], ids=lambda s: "x".join(map(str, s)))
def test_nearest_point_idx(device, shape):
    """Q = 512 queries a block, tiles of T = 512 references in sub-tiles of S = 64: 513 queries are a second
    block of one query, 513 references a second tile of one reference, 65 a second sub-tile of one."""
    from pvnet_amd import _eval_lib as P
    from tests.test_eval_abi import nearest_f32
    from tests.test_gpu_eval import Q, S, T
    L = P.load()
    b, pn1, pn2, dim = shape
    assert (Q, T, S) == (512, 512, 64) and shape in [(1, 1, 1, 2), (3, S + 1, Q + 1, 3), (2, T + 1, Q - 1, 2)]
    rng = np.random.default_rng([pn1, pn2, dim])
    ref = rng.standard_normal((b, pn1, dim)).astype(np.float32)
    que = rng.standard_normal((b, pn2, dim)).astype(np.float32)
    que[:, -1] = ref[:, -1]                                     # the last query's nearest is the last reference

    def call(p, ws, nbytes, stream):
        return L.pv_nearest_point_idx(p["ref"], p["que"], p["idx"], b, pn1, pn2, dim, stream)

    def parity(got):
        for i in range(b):
            np.testing.assert_array_equal(got["idx"][i], nearest_f32(ref[i], que[i])[0])
        assert (got["idx"][:, -1] == pn1 - 1).all()

    contract(device, Spec(f"pv_nearest_point_idx {shape}", dict(ref=ref, que=que), dict(idx=((b, pn2), np.int32)), call, P.check),
             parity)


@functools.lru_cache(maxsize=None)
def metrics_scene(b):
    """Models of 1, 512 and 513 points in one table; b poses over them (b = 1: the largest alone, so the
    others' rows of the table are never the pose's), every rotation at least 0.05 rad from its truth."""
    from tests.test_eval_abi import make_pose, rodrigues, symmetric_cloud
    rng = np.random.default_rng(b)
    mods = [(rng.standard_normal((1, 3)) * 0.04).astype(np.float32), symmetric_cloud(rng, 256),
            np.concatenate([symmetric_cloud(rng, 256), np.array([[0, 0, 0.03]], np.float32)])]
    mid = np.array([2] if b == 1 else [i % 3 for i in range(b)], np.int32)
    gt, pred = [], []
    for i in range(b):
        g = make_pose(rng.standard_normal(3), rng.uniform(0.2, 2.9),
                      [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.3)])
        dR = rodrigues(rng.standard_normal(3), rng.uniform(0.05, 0.3))
        gt.append(g)
        pred.append(np.concatenate([dR @ g[:, :3], g[:, 3:] + rng.uniform(-0.02, 0.02, (3, 1))], 1))
    return mods, np.stack(pred), np.stack(gt), mid


@pytest.mark.parametrize("metrics", ["all", "add"])
@pytest.mark.parametrize("b", [1, 65])
def test_pose_metrics(device, b, metrics):
    """65 poses: a second k_pose_finish block (64 poses each) of one pose.  max_pn = 513 gives every pose two
    partial blocks of 512 points; the 1- and 512-point models need one."""
    from pvnet_amd import _eval_lib as P
    from tests.test_eval_abi import COLS, K_LM
    from tests.test_gpu_eval import Q, check_columns, reference
    L = P.load()
    h = defines("pveval.h")
    mods, pred, gt, mid = metrics_scene(b)
    sizes = [len(m) for m in mods]
    assert sizes == [1, Q, Q + 1] and cdiv(max(sizes), Q) == 2 and (b == 1 or cdiv(b, 64) == 2)
    bits = h["PV_EVAL_ALL"] if metrics == "all" else h["PV_EVAL_ADD"]
    assert (h["PV_EVAL_ALL"], h["PV_EVAL_ADD"], h["PV_EVAL_NCOL"]) == (P.PV_EVAL_ALL, P.PV_EVAL_ADD, len(COLS))
    off = np.cumsum([0] + sizes).astype(np.int32)
    model = np.concatenate(mods)
    need = int(L.pv_eval_workspace_size(b, max(sizes)))

    def call(p, ws, nbytes, stream):
        bt = P.EvalBatch(b, len(model), p["pose_pred"], p["pose_gt"], p["model"], p["model_off"], p["model_id"], len(mods),
                         max(sizes), p["K"], 0, bits)
        return L.pv_pose_metrics(ctypes.byref(bt), p["out"], ws, nbytes, stream)

    def parity(got):
        want, Ms, pns = reference(pred, gt, mid, [(m,) for m in mods], K_LM)
        out = got["out"]
        if metrics == "all":
            check_columns(out, want, Ms, pns)
        else:                                                   # the column asked for, and the others untouched
            assert (np.abs(out[:, 0] - want[:, 0]) <= 1e-12 * np.array(pns) * np.abs(want[:, 0])).all()
            assert untouched(out[:, 1:])

    spec = Spec(f"pv_pose_metrics b={b} {metrics}",
                dict(pose_pred=pred, pose_gt=gt, model=model, model_off=off, model_id=mid, K=K_LM.astype(np.float64)),
                dict(out=((b, len(COLS)), np.float64)), call, P.check, ws=need)
    contract(device, spec, parity)


# ---------------------------------------------------------------- the voting entries
class GuardedBuffers:
    """tests/test_gpu_entry_matrix.py::run's allocator on guarded buffers."""

    def __init__(self, device, surround=0x00, ws_fill=0x00):
        self.g, self.surround, self.ws_fill = Guarded(device), surround, ws_fill

    def inp(self, a):
        return self.g.inp(np.asarray(a), surround=self.surround)

    def empty(self, shape, dtype):
        return self.g.out(shape, dtype, fill=OUT_FILL)

    def full(self, shape, value, dtype):
        t = self.g.out(shape, dtype)
        t.fill_(value)
        return t

    def workspace(self, nbytes):
        return self.g.workspace(nbytes, fill=self.ws_fill)

    def done(self):
        pass


def pipeline_cases():
    """One single-object and one multi-object case of tests/entry_cases.py per entry (parts B, C and L), all at
    37 x 51 with b = 2."""
    from tests import entry_cases as EC
    by = {c.name: c for c in EC.part_b() + EC.part_c() + EC.part_layers()}
    names = ["L-v3-seg_f16-from_network", "L-v3-seg_f32-multi_from_network", "L-v5-i64", "C-v5-i32", "B-evd_mean-seg_f32",
             "C-evd_mean-seg_f16", "B-evd_topk-seg_f16", "C-evd_topk-i32"]
    cases = [by[n] for n in names]
    assert all((c.H, c.W, c.b) == (37, 51, 2) for c in cases)
    assert sorted((c.entry, c.ncls > 0) for c in cases) == sorted((e, m) for e in ("v3", "v5", "evd_mean", "evd_topk")
                                                                  for m in (False, True))
    return cases


@pytest.mark.parametrize("case", pipeline_cases(), ids=lambda c: c.name)
def test_voting_pipelines(case, device):
    """pv_ransac_voting_v3 / _v5, pv_estimate_voting_distribution / _with_mean, single- and multi-object: kp,
    conf, mean, cov and all eight diag arrays guarded, the workspace exactly pv_v3_workspace_size."""
    from pvnet_amd import ransac_voting_gpu as rvg
    from tests import entry_cases as EC
    from tests.test_gpu_entry_matrix import check, run

    def go(**kw):
        a = GuardedBuffers(device, **kw)
        got = run(case, device, rvg, alloc=a)
        a.g.check()
        # counts, tn and hyp of the EVD entries and the class words are read out of the workspace: those of a
        # skipped virtual image are whatever the workspace held
        voted = got["tn"] > 0
        for k in ("words",) + (("counts", "hyp") if case.entry.startswith("evd") else ()):
            got[k] = got[k][voted]
        return got

    base = go()
    same(base, go(), f"{case.name}: two plain runs")
    for fill in (0xFF, 0xA5):
        same(base, go(ws_fill=fill), f"{case.name}: workspace prefilled with {fill:#04x}")
    same(base, go(surround=0xFF), f"{case.name}: inputs surrounded by 0xFF")
    assert (base["tn"] > 0).any()
    check(case, run(case, device, rvg, alloc=GuardedBuffers(device)), EC.reference(case))


def motion_close(ref):
    def close(a, b, what):
        # tests/test_gpu_tail_stages.py: the kernel adds the same f32 terms in f64 in another order (here: in
        # arrival order, by atomicAdd) and rounds once: within one f32 ulp of the oracle's f64 mean
        for r in (a, b):
            assert (np.abs(r["out"].astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref))).all(), what
    return close


@pytest.mark.parametrize("vn", [1, 9])
def test_motion_voting(device, vn):
    """W, R and I; its scratch is internal, so D does not apply."""
    from oracle import oracle as O
    from pvnet_amd import _lib
    L = _lib.load()
    b, H, W = 2, 37, 51
    rng = np.random.default_rng(70 + vn)
    mask = (rng.random((b, H, W)) < 0.5).astype(np.int64) * 3
    mask[:, -1, -1] = 3
    vertex = rng.normal(0, 3, (b, H, W, vn, 2)).astype(np.float32)
    ref = O.ransac_motion_voting(mask, vertex)

    def call(p, ws, nbytes, stream):
        d = _lib.ImageDesc()
        d.mask, d.mask_kind, d.vertex, d.vertex_kind = p["mask"], _lib.PV_MASK_I64, p["vertex"], _lib.PV_VERTEX_F32
        d.mask_strides[:] = (H * W, W, 1, 0)
        d.vertex_strides[:] = (H * W * vn * 2, W * vn * 2, vn * 2, 2, 1)
        d.b, d.H, d.W, d.vn, d.ncls = b, H, W, vn, 0
        return L.pv_ransac_motion_voting(ctypes.byref(d), p["out"], stream)

    close = motion_close(ref)
    spec = Spec(f"pv_ransac_motion_voting vn={vn}", dict(mask=mask, vertex=vertex), dict(out=((b, vn, 2), np.float32)), call,
                _lib.check, exact=False, close=close)
    contract(device, spec, lambda got: close(got, got, "parity"))


# ---------------------------------------------------------------- the byte vote and the API kernels
@functools.lru_cache(maxsize=None)
def vote_inputs(tn, vn, hn):
    rng = np.random.default_rng([tn, vn, hn])
    coords = np.stack([rng.integers(0, 640, tn), rng.integers(0, 480, tn)], 1).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, (tn, vn))
    direct = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)
    hyp = np.stack([rng.uniform(-50, 690, (hn, vn)), rng.uniform(-50, 530, (hn, vn))], -1).astype(np.float32)
    idxs = rng.integers(0, tn, (hn, vn, 2)).astype(np.int32)
    init = (rng.random((hn, vn, tn)) < 0.3).astype(np.uint8) * 7
    return direct, coords, hyp, idxs, init


@pytest.mark.parametrize("offset", [0, 1, 5])
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "or"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 2, 37), (513, 2, 80), (1029, 3, 256)], ids=lambda s: "x".join(map(str, s)))
def test_vote_bytes(device, shape, dense, offset):
    """k_vote_bytes stores rows of tn bytes with unaligned 8-byte stores and byte tails: tn = 7, 513 and 1029 end
    every row but the first off an 8-byte boundary, and the header sets no alignment for `inliers`, so it also
    sits 1 and 5 bytes past one.  hn = 256 is the block-shared staging path.  In OR mode the bytes that hold 7
    and are no inlier stay 7."""
    from oracle import oracle as O
    from pvnet_amd import _lib
    L = _lib.load()
    tn, vn, hn = shape
    thr = 0.9
    direct, coords, hyp, _, init = vote_inputs(tn, vn, hn)
    assert tn == 1 or tn % 8 != 0
    ref = np.zeros((hn, vn, tn), np.uint8) if dense else init.copy()
    O.voting_for_hypothesis(direct, coords, hyp, ref, thr)
    if ref.size > 100:
        assert 0 < (ref == 1).sum() < ref.size // 2 and (dense or (ref == 7).any())

    def call(p, ws, nbytes, stream):
        return L.pv_voting_for_hypothesis(p["direct"], p["coords"], p["hypo"], p["inliers"], tn, vn, hn, thr,
                                          _lib.PV_VOTE_DENSE if dense else _lib.PV_VOTE_OR, stream)

    out = ((hn, vn, tn), np.uint8, offset) if dense else ((hn, vn, tn), np.uint8, offset, init)
    spec = Spec(f"pv_voting_for_hypothesis {shape} dense={dense} +{offset}", dict(direct=direct, coords=coords, hypo=hyp),
                dict(inliers=out), call, _lib.check)
    contract(device, spec, lambda got: np.testing.assert_array_equal(got["inliers"], ref))


def test_vote_bytes_balanced_grid_writes(device):
    """W alone at the CU-balanced shape of tests/test_gpu_parity.py (tn = 15,000, vn = 9, hn = 256: full and
    quarter blocks), the 34.6 MB of bytes between guards; every row sums to pv_vote_counts' count."""
    from oracle import oracle as O
    from pvnet_amd import _lib
    from tests import golden_io as G
    L = _lib.load()
    g = G.load("synth_v3_512")
    mask, vertex = G.synth_inputs(g)[:2]
    coords, direct = O.compact(O.fg_mask_v3(mask[0]), vertex[0])
    tn, vn, hn = 15000, 9, 256
    sel = np.sort(np.random.default_rng(11).choice(coords.shape[0], tn, replace=False))
    coords, direct = np.ascontiguousarray(coords[sel]), np.ascontiguousarray(direct[sel])
    idxs = np.random.default_rng(12).integers(0, tn, (hn, vn, 2)).astype(np.int32)
    hyp = O.generate_hypothesis(direct, coords, idxs)
    inputs = dict(direct=direct, coords=coords, hypo=hyp)
    counts = execute(device, Spec("pv_vote_counts balanced", inputs, dict(counts=((hn, vn), np.int32)),
                                  lambda p, ws, n, st: L.pv_vote_counts(p["direct"], p["coords"], p["hypo"], p["counts"], tn, vn,
                                                                        hn, 0.99, st), _lib.check))["counts"]
    got = execute(device, Spec("pv_voting_for_hypothesis balanced", inputs, dict(inliers=((hn, vn, tn), np.uint8)),
                               lambda p, ws, n, st: L.pv_voting_for_hypothesis(p["direct"], p["coords"], p["hypo"], p["inliers"],
                                                                               tn, vn, hn, 0.99, _lib.PV_VOTE_DENSE, st),
                               _lib.check))["inliers"]
    assert got.max() == 1 and counts.max() > 100
    np.testing.assert_array_equal(got.sum(2, dtype=np.int32), counts)


def canon(a):
    """f32 bits with every NaN the same."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


@pytest.mark.parametrize("hn,vn", [(1, 1), (85, 3), (257, 1)], ids=["1", "255", "257"])
def test_api_kernels(device, hn, vn):
    """pv_generate_hypothesis, _vp, pv_vote_counts and pv_voting_for_hypothesis_vp launch 256 lanes a block over
    hn * vn items: one item, one short of a block, one past it."""
    from oracle import oracle as O
    from pvnet_amd import _lib
    L = _lib.load()
    tn = 37
    assert hn * vn in (1, 255, 257)
    direct, coords, hyp, idxs, init = vote_inputs(tn, vn, hn)
    base = dict(direct=direct, coords=coords)

    got = contract(device, Spec(f"pv_generate_hypothesis {hn}x{vn}", dict(base, idxs=idxs), dict(hypo=((hn, vn, 2), np.float32)),
                                lambda p, ws, n, st: L.pv_generate_hypothesis(p["direct"], p["coords"], p["idxs"], p["hypo"], tn,
                                                                              vn, hn, st), _lib.check))
    np.testing.assert_array_equal(canon(got["hypo"]), canon(O.generate_hypothesis(direct, coords, idxs)))

    got = contract(device, Spec(f"pv_generate_hypothesis_vp {hn}x{vn}", dict(base, idxs=idxs), dict(hypo=((hn, vn, 3), np.float32)),
                                lambda p, ws, n, st: L.pv_generate_hypothesis_vp(p["direct"], p["coords"], p["idxs"], p["hypo"],
                                                                                 tn, vn, hn, st), _lib.check))
    hyp3 = O.generate_hypothesis_vanishing_point(direct, coords, idxs)
    np.testing.assert_array_equal(canon(got["hypo"]), canon(hyp3))

    got = contract(device, Spec(f"pv_vote_counts {hn}x{vn}", dict(base, hypo=hyp), dict(counts=((hn, vn), np.int32)),
                                lambda p, ws, n, st: L.pv_vote_counts(p["direct"], p["coords"], p["hypo"], p["counts"], tn, vn, hn,
                                                                      0.9, st), _lib.check))
    np.testing.assert_array_equal(got["counts"], O.vote_counts(direct, coords, hyp, 0.9))

    vp_vote(device, direct, coords, hyp3, init, tn, vn, hn)


def vp_vote(device, direct, coords, hyp3, init, tn, vn, hn):
    from oracle import oracle as O
    from pvnet_amd import _lib
    L = _lib.load()
    ref = init.copy()
    O.voting_for_hypothesis_vanishing_point(direct, coords, hyp3, ref, 0.9)
    got = contract(device, Spec(f"pv_voting_for_hypothesis_vp {tn}x{vn}x{hn}", dict(direct=direct, coords=coords, hypo=hyp3),
                                dict(inliers=((hn, vn, tn), np.uint8, 0, init)),
                                lambda p, ws, n, st: L.pv_voting_for_hypothesis_vp(p["direct"], p["coords"], p["hypo"],
                                                                                   p["inliers"], tn, vn, hn, 0.9, st), _lib.check))
    np.testing.assert_array_equal(got["inliers"], ref)
    return ref


def test_vp_vote_small(device):
    """The vanishing-point vote at (tn, vn, hn) = (37, 2, 7)."""
    from oracle import oracle as O
    tn, vn, hn = 37, 2, 7
    direct, coords, _, idxs, init = vote_inputs(tn, vn, hn)
    ref = vp_vote(device, direct, coords, O.generate_hypothesis_vanishing_point(direct, coords, idxs), init, tn, vn, hn)
    assert (ref == 1).any() and (ref == 7).any()


# ---------------------------------------------------------------- plain PnP
@pytest.mark.parametrize("b,pn,f64", [(1, 6, True), (3, 9, False), (65, 64, True)], ids=["1x6", "3x9", "65x64"])
def test_epnp(device, b, pn, f64):
    """One 64-lane block per image over pn points: the fewest the entry takes (PV_EPNP_MIN_POINTS; 4 points are
    refused, below), 9, and all 64 lanes with a 65th image.  Rt, rt6 and every diag output guarded."""
    from pvnet_amd import _pose_lib as P
    from tests import epnp_ref as E
    from tests.test_gpu_epnp import TOL, make_batch, reference
    from oracle import pnp as OP
    L = P.load()
    h = defines("pvpose.h")
    assert pn in (h["PV_EPNP_MIN_POINTS"], 9, h["PV_EPNP_MAX_POINTS"]) and h["PV_EPNP_MAX_POINTS"] == 64
    bt = make_batch(100 * pn + b, pn, b, b > 1)
    p2 = bt["p2"] if f64 else bt["p2"].astype(np.float32)
    per = bt["per_image"]

    def call(p, ws, nbytes, stream):
        cb = P.EpnpBatch(b, pn, None if f64 else p["p2"], p["p2"] if f64 else None, p["p3"], p["K"], pn * 3 if per else 0,
                         9 if per else 0)
        dg = P.EpnpDiag(p["status"], p["n_used"], p["cand_err"])
        return L.pv_epnp(ctypes.byref(cb), p["Rt"], p["rt6"], ctypes.byref(dg), stream)

    def parity(got):
        for i, r in enumerate(reference(bt, p2.astype(np.float64))):
            assert r["status"] == E.OK and got["status"][i] == E.OK and 1 <= got["n_used"][i] <= 3, i
            assert np.abs(got["Rt"][i] - r["Rt"]).max() < TOL, i
            assert np.abs(OP.rodrigues_vec_to_mat(got["rt6"][i, :3]) - r["Rt"][:, :3]).max() < TOL, i
            assert np.abs(got["rt6"][i, 3:] - r["Rt"][:, 3]).max() < TOL, i
            assert np.abs(got["cand_err"][i] - r["cand_err"]).max() < TOL, i

    spec = Spec(f"pv_epnp b={b} pn={pn}", dict(p2=p2, p3=np.ascontiguousarray(bt["p3"]), K=np.ascontiguousarray(bt["K"])),
                dict(Rt=((b, 3, 4), np.float64), rt6=((b, 6), np.float64), status=((b,), np.int32), n_used=((b,), np.int32),
                     cand_err=((b, 3), np.float64)), call, P.check)
    contract(device, spec, parity)


def test_epnp_refuses_four_points_and_writes_nothing(device):
    """(b, pn) = (1, 4) is below PV_EPNP_MIN_POINTS: PV_EINVAL on the host, and no output byte changes."""
    from pvnet_amd import _pose_lib as P
    from tests.test_gpu_epnp import make_batch
    L = P.load()
    bt = make_batch(7, 6, 1, False)
    codes = []

    def call(p, ws, nbytes, stream):
        cb = P.EpnpBatch(1, 4, None, p["p2"], p["p3"], p["K"], 0, 0)
        dg = P.EpnpDiag(p["status"], p["n_used"], p["cand_err"])
        codes.append(L.pv_epnp(ctypes.byref(cb), p["Rt"], p["rt6"], ctypes.byref(dg), stream))
        return 0

    spec = Spec("pv_epnp pn=4", dict(p2=bt["p2"][:, :4], p3=bt["p3"][:4], K=np.ascontiguousarray(bt["K"])),
                dict(Rt=((1, 3, 4), np.float64), rt6=((1, 6), np.float64), status=((1,), np.int32), n_used=((1,), np.int32),
                     cand_err=((1, 3), np.float64)), call, P.check)
    got = execute(device, spec)
    assert codes == [P.PV_EINVAL] and all(untouched(v) for v in got.values())


@pytest.mark.parametrize("b", [1, 63, 65])
def test_rt6_to_Rt(device, b):
    from oracle import pnp as OP
    from pvnet_amd import _pose_lib as P
    L = P.load()
    r = np.random.default_rng(b).standard_normal((b, 6))
    r[0, :3] = np.array([0.6, 0.0, 0.8]) * (np.pi - 1e-9)
    r[-1, :3] = 1e-9

    def parity(got):
        for i in range(b):                                      # tests/test_gpu_epnp.py::test_rt6_to_Rt
            assert np.abs(got["Rt"][i, :, :3] - OP.rodrigues_vec_to_mat(r[i, :3])).max() < 1e-12, i
            np.testing.assert_array_equal(got["Rt"][i, :, 3], r[i, 3:])

    contract(device, Spec(f"pv_rt6_to_Rt b={b}", dict(rt6=r), dict(Rt=((b, 3, 4), np.float64)),
                          lambda p, ws, n, st: L.pv_rt6_to_Rt(p["rt6"], p["Rt"], b, st), P.check), parity)


# ---------------------------------------------------------------- uncertainty PnP
@functools.lru_cache(maxsize=None)
def pnp_batch(b, pn):
    """Noisy images of one model (tests/test_pnp_oracle.py's noisy_case, for any pn): p2 f32 [b, pn, 2], cov f32
    [b, pn, 2, 2], p3 f64 [pn, 3]."""
    from oracle import pnp as OP
    from tests import epnp_ref as E
    from tests.test_pnp_oracle import K_LM, box_keypoints, project
    rng = np.random.default_rng([b, pn])
    p3 = box_keypoints()[:pn] if pn <= 9 else E.random_model(rng, pn)
    p2, cov = [], []
    for _ in range(b):
        R = OP.rodrigues_vec_to_mat(rng.normal(size=3))
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.0)])
        a = rng.normal(size=(pn, 2, 2)) * (0.0 if pn == 4 else 1.0)     # four points: P3P alone, on exact data
        c = a @ a.transpose(0, 2, 1) + 0.05 * np.eye(2)
        noise = np.array([rng.multivariate_normal([0, 0], ci) for ci in c]) * (0.0 if pn == 4 else 1.0)
        p2.append(project(R, t, p3, K_LM) + noise)
        cov.append(c)
    return np.array(p2, np.float32), np.array(cov, np.float32), p3


PNP_DIAG = dict(init_rt=(6,), p3p_ok=(), iterations=(), status=(), cost=())


def pnp_outputs(b, first):
    dt = dict(init_rt=np.float64, p3p_ok=np.int32, iterations=np.int32, status=np.int32, cost=np.float64)
    return dict(first, **{k: ((b, *s), dt[k]) for k, s in PNP_DIAG.items()})


@pytest.mark.parametrize("mode", ["weights", "cov", "cov_v2"])
@pytest.mark.parametrize("b,pn", [(1, 4), (3, 9), (2, 64)], ids=["1x4", "3x9", "2x64"])
def test_uncertainty_pnp(device, b, pn, mode):
    """One wave per image over pn <= kMaxPts = 64 points: P3P alone (4), the usual 9, and every lane."""
    from oracle import pnp as OP
    from pvnet_amd import _lib
    from tests.test_gpu_pnp import TOL
    from tests.test_pnp_oracle import K_LM
    L = _lib.load()
    p2, cov, p3 = pnp_batch(b, pn)
    kind = {"weights": _lib.PV_PNP_WEIGHTS, "cov": _lib.PV_PNP_COV, "cov_v2": _lib.PV_PNP_COV_V2}[mode]
    wgt = np.stack([OP.weights_from_cov(c) for c in cov]).astype(np.float64) if mode == "weights" else cov

    def call(p, ws, nbytes, stream):
        bt = _lib.PnpBatch(b, pn, kind, p["p2"], p["wgt"], p["p3"], p["K"], 0, 0, None)
        dg = _lib.PnpDiag(*(p[k] for k in PNP_DIAG))
        return L.pv_uncertainty_pnp(ctypes.byref(bt), p["Rt"], ctypes.byref(dg), stream)

    def parity(got):
        for i in range(b):
            d = {}
            if mode == "cov_v2":
                ref = OP.uncertainty_pnp_v2(p2[i], cov[i], p3, K_LM, diag=d)
            else:
                ref = OP.uncertainty_pnp(p2[i], OP.weights_from_cov(cov[i]), p3, K_LM, diag=d)
            assert bool(got["p3p_ok"][i]) == bool(d["p3p_ok"]) and got["status"][i] > 0, i
            np.testing.assert_allclose(got["init_rt"][i], d["init"], atol=1e-6, err_msg=f"init {i}")
            # tests/test_gpu_pnp.py: 1e-7 against the oracle, 1e-6 for the P3P pose of four points
            np.testing.assert_allclose(got["Rt"][i], ref, atol=1e-6 if pn == 4 else TOL, err_msg=f"image {i}")

    spec = Spec(f"pv_uncertainty_pnp b={b} pn={pn} {mode}", dict(p2=p2, wgt=wgt, p3=p3, K=K_LM.astype(np.float64)),
                pnp_outputs(b, dict(Rt=((b, 3, 4), np.float64))), call, _lib.check)
    contract(device, spec, parity)


@pytest.mark.parametrize("b,pn", [(1, 4), (3, 9), (2, 64)], ids=["1x4", "3x9", "2x64"])
def test_uncertainty_pnp_refine(device, b, pn):
    """The least squares alone from given starts (PV_PNP_WEIGHTS is its only mode)."""
    from oracle import pnp as OP
    from pvnet_amd import _lib
    from tests.test_gpu_pnp import TOL
    from tests.test_pnp_oracle import K_LM
    L = _lib.load()
    p2, cov, p3 = pnp_batch(b, pn)
    wgt = np.stack([OP.weights_from_cov(c) for c in cov]).astype(np.float64)
    x0 = []
    for i in range(b):                                          # starts near the full call's answer
        Rt = OP.uncertainty_pnp(p2[i], wgt[i], p3, K_LM)
        x0.append(np.concatenate([OP.rodrigues_mat_to_vec(Rt[:, :3]), Rt[:, 3]]))
    x0 = np.array(x0) + np.random.default_rng(pn).uniform(0, 0.02, (b, 6))

    def call(p, ws, nbytes, stream):
        bt = _lib.PnpBatch(b, pn, _lib.PV_PNP_WEIGHTS, p["p2"], p["wgt"], p["p3"], p["K"], 0, 0, None)
        dg = _lib.PnpDiag(*(p[k] for k in PNP_DIAG))
        return L.pv_uncertainty_pnp_refine(ctypes.byref(bt), p["init"], p["result"], ctypes.byref(dg), stream)

    def parity(got):
        for i in range(b):
            ref = OP.ceres_lm(x0[i], p2[i].astype(np.float64), p3, wgt[i], K_LM)
            np.testing.assert_allclose(got["result"][i], ref, atol=TOL, err_msg=f"image {i}")
            assert got["status"][i] > 0

    spec = Spec(f"pv_uncertainty_pnp_refine b={b} pn={pn}", dict(p2=p2, wgt=wgt, p3=p3, K=K_LM.astype(np.float64), init=x0),
                pnp_outputs(b, dict(result=((b, 6), np.float64))), call, _lib.check)
    contract(device, spec, parity)
