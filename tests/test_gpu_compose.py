"""libpvcompose.so on the device (include/pvcompose.h) against its numpy restatement tests/compose_ref.py:
every output bit for bit, no tolerance anywhere but the two gates taken from the renderer's tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import augment_ref as AR
from tests import compose_ref as R

I32 = np.iinfo(np.int32)
FILL = (12, 200, 77)
NCLS = 3
LABEL_DTYPES = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
LABEL_NP = {"u8": np.uint8, "i32": np.int32, "i64": np.int64}
LABEL_KIND = {"i64": 0, "u8": 1, "i32": 2}
SHAPES = {"37x53": (29, 41, 37, 53), "48x64": (48, 64, 48, 64)}       # (H, W, Ho, Wo)


@pytest.fixture(scope="module")
def C(device):
    import __graft_entry__ as g
    g.build()
    from pvnet_amd import compose
    return compose


def cu(a, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(device)


def same(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)


# ---- 1. the constructed scene ----------------------------------------------------------------------------------
def make_bank(H, W, seed=0):
    """Six single-object frames.  0 and 1: the same ellipse with holes, other colours (1 over 0 hides it whole);
    2: a smaller ellipse marked 2 among distractors marked 1; 3: a rectangle; 4: a thin diagonal; 5: no foreground."""
    rng = np.random.default_rng([H, W, seed])
    image = rng.integers(0, 256, (6, H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[:H, :W]
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    ell = ((x - cx) / (W / 3.2)) ** 2 + ((y - cy) / (H / 3.2)) ** 2 <= 1.0
    label = np.zeros((6, H, W), np.int64)
    label[0] = label[1] = ell & ((3 * y + x) % 7 != 0)
    label[2] = np.where(((x - cx) / (W / 5.0)) ** 2 + ((y - cy) / (H / 4.0)) ** 2 <= 1.0, 2, (x + y) % 5 == 0)
    label[3, H // 4:H - H // 4, W // 3:W - W // 4] = 1
    label[4] = np.abs((x - cx) * H - (y - cy) * W) <= 1.5 * W
    return image, label


def box_of(label, src, src_label):
    ys, xs = np.nonzero(label[src] == src_label)
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def groups(label, Ho, Wo):
    """Sixteen slots in four groups of four: (src, src_label, cls, box, (dx, dy)).  Each shift puts the box's
    centre (rounded down) on a chosen point of the output frame; +1 where the parity is wanted."""
    def slot(src, sl, cls, at, box=None, odd=None):
        bx = box or (box_of(label, src, sl) if 0 <= src < 6 and (label[src] == sl).any() else (0, 0, 5, 5))
        dx, dy = at[0] - (bx[0] + bx[2]) // 2, at[1] - (bx[1] + bx[3]) // 2
        if odd is not None:
            dx += (dx % 2) != odd[0]
            dy += (dy % 2) != odd[1]
        return (src, sl, cls, bx, (dx, dy))

    mx, my = Wo // 2, Ho // 2
    b3 = box_of(label, 3, 1)
    return [
        # the four frame edges; classes 1, 2, 1, 2: two slots of one class in a frame
        [slot(0, 1, 1, (0, my)), slot(2, 2, 2, (mx, 0)), slot(3, 1, 1, (Wo - 1, my), odd=(1, 0)), slot(4, 1, 2, (mx, Ho - 1))],
        # wholly outside, src = -1, a source without foreground, one plain object at an even shift
        [slot(0, 1, 1, (2 * Wo + 40, my)), slot(-1, 1, 2, (mx, my)), slot(5, 1, 3, (mx, my)), slot(3, 1, 2, (mx, my), odd=(0, 0))],
        # 0 fully hidden by 1 (the same mask), 1 partly hidden by 2, a class outside 1..ncls
        [slot(0, 1, 1, (mx, my)), slot(1, 1, 2, (mx, my)), slot(3, 1, 3, (mx + 5, my + 3)), slot(4, 1, NCLS + 1, (mx, my))],
        # an inverted box, a box that cuts its object, the same class again over it, an odd dy
        [slot(0, 1, 1, (mx, my), box=(b3[2], b3[1], b3[0], b3[3])), slot(3, 1, 2, (mx - 6, my), box=(b3[0] + 2, b3[1] + 1, b3[2] - 3, b3[3])),
         slot(2, 2, 2, (mx + 4, my - 2)), slot(4, 1, 1, (mx - 3, my + 4), odd=(0, 1))],
    ]


@functools.lru_cache(maxsize=None)
def scene(shape, S):
    """The bank, and b frames of S slots holding the sixteen constructed slots: S = 4: one group a frame;
    S = 16: frame 0 all sixteen, frame 1 the groups in reverse order; S = 1: one slot a frame.  The properties
    the issue lists are asserted here, on the reference, before any test looks at the device (those that need
    two slots in one frame for S >= 4 only)."""
    H, W, Ho, Wo = SHAPES[shape]
    image, label = make_bank(H, W)
    gs = groups(label, Ho, Wo)
    flat = [s for g in gs for s in g]
    frames = {1: [[s] for s in flat], 4: gs, 16: [flat, [s for g in gs[::-1] for s in g]]}[S]
    b = len(frames)
    pick = np.zeros((b, S, 8), np.int32)
    shift = np.zeros((b, S, 2), np.int32)
    for f, fr in enumerate(frames):
        for s, (src, sl, cls, bx, d) in enumerate(fr):
            pick[f, s] = (src, sl, cls, *bx, 0)
            shift[f, s] = d
    rng = np.random.default_rng(7)
    background = rng.integers(0, 256, (b, Ho, Wo, 3), dtype=np.uint8)
    sc = dict(image=image, label=label, pick=pick, shift=shift, background=background, b=b, S=S, shape=shape)

    # what each slot would show alone in its frame
    alone = np.zeros((b, S), np.int64)
    for s in range(S):
        only = pick.copy()
        only[:, np.arange(S) != s, 0] = -1
        alone[:, s] = R.compose(image, label, only, shift, NCLS, Ho, Wo)[3][:, s]
    _, _, _, vis = R.compose(image, label, pick, shift, NCLS, Ho, Wo)
    sc["alone"], sc["visible"] = alone, vis
    count = lambda f, s: int((label[pick[f, s, 0]] == pick[f, s, 1]).sum())
    where = {}
    for f, fr in enumerate(frames):
        for i, sl in enumerate(fr):
            where.setdefault(id(sl), (f, i))                                                         # its first place
    at = lambda g, i: where[id(gs[g][i])]
    # a slot cut by each of the four frame edges: its shifted box crosses the edge, and it shows less than it has
    for i, crosses in enumerate((lambda x0, y0, x1, y1: x0 < 0 <= x1, lambda x0, y0, x1, y1: y0 < 0 <= y1,
                                 lambda x0, y0, x1, y1: x0 <= Wo - 1 < x1, lambda x0, y0, x1, y1: y0 <= Ho - 1 < y1)):
        f, s = at(0, i)
        bx, d = pick[f, s, 3:7], shift[f, s]
        assert crosses(bx[0] + d[0], bx[1] + d[1], bx[2] + d[0], bx[3] + d[1]) and 0 < alone[f, s] < count(f, s), ("edge", i)
    f, s = at(1, 0)
    assert alone[f, s] == 0 and pick[f, s, 3] + shift[f, s, 0] > Wo - 1 and count(f, s) > 0          # wholly outside
    f, s = at(1, 1)
    assert pick[f, s, 0] == -1 and alone[f, s] == 0
    f, s = at(1, 2)
    assert not (label[pick[f, s, 0]] > 0).any() and alone[f, s] == 0                                  # no foreground
    f, s = at(2, 3)
    assert pick[f, s, 2] == NCLS + 1 and alone[f, s] == 0
    f, s = at(3, 0)
    assert pick[f, s, 3] > pick[f, s, 5] and alone[f, s] == 0                                         # inverted
    f, s = at(3, 1)
    assert 0 < alone[f, s] < count(f, s)                                                              # cut by its box
    assert {tuple(shift[at(g, i)] % 2) for g, i in ((0, 2), (1, 3), (3, 3))} == {(1, 0), (0, 0), (0, 1)}
    if S >= 4:
        f, s = at(2, 0)
        assert vis[f, s] == 0 < alone[f, s]                                                           # fully hidden
        f, s = at(2, 1)
        assert 0 < vis[f, s] < alone[f, s]                                                            # partly hidden
        live_cls = [[int(pick[f, s, 2]) for s in range(S) if alone[f, s] > 0] for f in range(b)]
        assert any(len(c) > len(set(c)) for c in live_cls)                                            # one class twice
    return sc


def run_compose(C, device, sc, kind, bg, want_instance, erase=None, fill=FILL):
    H, W, Ho, Wo = SHAPES[sc["shape"]] if isinstance(sc["shape"], str) else sc["shape"]
    label = sc["label"].astype(LABEL_NP[kind])
    background = {None: None, "shared": sc["background"][:1], "each": sc["background"]}[bg]
    got = C.compose(cu(sc["image"], device), cu(label, device), cu(sc["pick"], device), cu(sc["shift"], device), NCLS, (Ho, Wo),
                    background=None if background is None else cu(background, device), fill=fill,
                    erase=None if erase is None else cu(erase, device), want_instance=want_instance)
    ref = R.compose(sc["image"], label, sc["pick"], sc["shift"], NCLS, Ho, Wo, background, fill, erase)
    what = f"{sc['shape']} S={sc['S']} {kind} bg={bg}"
    same(got[0], ref[0], what + " image")
    same(got[1], ref[1], what + " label")
    assert (got[2] is None) == (not want_instance)
    if want_instance:
        same(got[2], ref[2], what + " instance")
    same(got[3], ref[3], what + " visible")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(LABEL_DTYPES))
@pytest.mark.parametrize("S", [1, 4, 16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity(device, C, shape, S, kind):
    sc = scene(shape, S)
    Ho, Wo = SHAPES[shape][2:]
    if shape == "37x53":
        assert -(-Ho * -(-Wo // 8) // 256) == 2 and Wo % 8          # two blocks a frame, a ragged last group
    for bg in (None, "shared", "each"):
        for want_instance in (False, True):
            ref = run_compose(C, device, sc, kind, bg, want_instance)
    np.testing.assert_array_equal(ref[3], sc["visible"])


# ---- 2. small and odd sizes, strides ------------------------------------------------------------------------------
def random_scene(shape, S, seed, N=3):
    H, W, Ho, Wo = shape
    rng = np.random.default_rng([seed, H, W, Ho, Wo])
    image = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    label = rng.integers(0, 3, (N, H, W)).astype(np.int64)
    b = 3
    pick = np.zeros((b, S, 8), np.int32)
    pick[..., 0] = rng.integers(0, N, (b, S))
    pick[..., 1] = rng.integers(1, 3, (b, S))
    pick[..., 2] = rng.integers(1, NCLS + 1, (b, S))
    pick[..., 3:5] = rng.integers(-1, 2, (b, S, 2))
    pick[..., 5] = rng.integers(0, W + 1, (b, S))
    pick[..., 6] = rng.integers(0, H + 1, (b, S))
    shift = np.stack([rng.integers(-(W // 2) - 1, Wo // 2 + 2, (b, S)), rng.integers(-(H // 2) - 1, Ho // 2 + 2, (b, S))], -1).astype(np.int32)
    background = rng.integers(0, 256, (b, Ho, Wo, 3), dtype=np.uint8)
    return dict(image=image, label=label, pick=pick, shift=shift, background=background, b=b, S=S, shape=shape)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(1, 1, 1, 1), (1, 9, 1, 9), (9, 1, 9, 1), (5, 6, 4, 7), (6, 10, 5, 9), (6, 10, 3, 15),
                                   (6, 10, 3, 17), (3, 30, 2, 23), (3, 30, 2, 25)], ids=str)
def test_small_and_odd_sizes(device, C, sizes):
    """Wo = 7 is less than one lane's 8 pixels; 9, 15, 17, 23, 25 are 8 k +- 1."""
    for seed in (1, 3):
        sc = random_scene(sizes, 3, seed)
        ref = run_compose(C, device, sc, "u8", "each", True)
        assert sizes[3] < 4 or (ref[1] > 0).any()
        run_compose(C, device, sc, "i64", None, True)


@pytest.mark.gpu
def test_strided_operands(device, C):
    sc = scene("37x53", 4)
    H, W, Ho, Wo = SHAPES["37x53"]
    b, S = sc["b"], sc["S"]
    ref = R.compose(sc["image"], sc["label"].astype(np.int32), sc["pick"], sc["shift"], NCLS, Ho, Wo, sc["background"], FILL)
    chw = cu(sc["image"].transpose(0, 3, 1, 2), device)                     # a CHW bank viewed as HWC
    assert chw.is_contiguous() and tuple(chw.shape) == (6, 3, H, W)
    wide = torch.zeros((6, H, W + 5), dtype=torch.int32, device=device)     # label views with a row pitch
    wide[:, :, :W] = cu(sc["label"].astype(np.int32), device)
    out_chw = torch.zeros((b, 3, Ho, Wo), dtype=torch.uint8, device=device)  # a channel-planar output
    out_cl = torch.zeros((b, 3, Ho, Wo), dtype=torch.uint8, device=device).contiguous(memory_format=torch.channels_last)
    out_lab = torch.full((b, Ho, Wo + 3), -7, dtype=torch.int32, device=device)
    bg = cu(sc["background"].transpose(0, 3, 1, 2), device).permute(0, 2, 3, 1)
    for out_img in (out_chw, out_cl):
        got = C.compose(chw.permute(0, 2, 3, 1), wide[:, :, :W], cu(sc["pick"], device), cu(sc["shift"], device), NCLS, (Ho, Wo),
                        background=bg, fill=FILL, out=(out_img.permute(0, 2, 3, 1), out_lab[:, :, :Wo]))
        same(out_img.permute(0, 2, 3, 1).contiguous(), ref[0], "strided image")
        same(out_lab[:, :, :Wo].contiguous(), ref[1], "strided label")
        assert bool((out_lab[:, :, Wo:] == -7).all())
        same(got[3], ref[3], "visible")


# ---- 3. erasers and hostile device data ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_erasers(device, C):
    H, W, Ho, Wo = SHAPES["48x64"]
    image, label = make_bank(H, W)
    b3, b2 = box_of(label, 3, 1), box_of(label, 2, 2)
    pick = np.zeros((2, 2, 8), np.int32)
    pick[:, 0] = (3, 1, 1, *b3, 0)
    pick[:, 1] = (2, 2, 2, *b2, 0)
    shift = np.array([[[-14, 0], [12, 2]]] * 2, np.int32)           # side by side, touching
    sc = dict(image=image, label=label, pick=pick, shift=shift, b=2, S=2, shape="48x64",
              background=np.random.default_rng(3).integers(0, 256, (2, Ho, Wo, 3), dtype=np.uint8))
    o3 = (b3[0] - 14, b3[1], b3[2] - 14, b3[3])
    o2 = (b2[0] + 12, b2[1] + 2, b2[2] + 12, b2[3] + 2)
    none = (0, 0, -1, -1)
    erase = np.array([
        [(o3[0] + 2, o3[1] + 2, o3[0] + 6, o3[1] + 5),              # inside one object
         (o3[2] - 3, o3[1] + 4, o2[0] + 4, o3[1] + 9),              # across two objects
         (Wo + 3, Ho + 3, Wo + 9, Ho + 9), (-20, -20, -2, -2),      # outside the frame
         (10, 5, 9, 8), (10, 9, 12, 8),                             # empty: x1 < x0, y1 < y0
         (o2[0] + 6, o2[1] + 6, o2[0] + 10, o2[1] + 10), (o2[0] + 8, o2[1] + 8, o2[0] + 14, o2[1] + 12)],   # two overlapping
        [(o2[0] - 1, o2[1] - 1, o2[2] + 1, o2[3] + 1), none, none, none, none, none, none, (I32.min, I32.min, -1, I32.max)],
    ], np.int32)
    assert erase.shape == (2, R.MAX_ERASE, 4)
    plain = R.compose(image, label, pick, shift, NCLS, Ho, Wo)
    for bg in (None, "each"):
        ref = run_compose(C, device, sc, "u8", bg, True, erase=erase)
    assert (plain[3] > 0).all()
    assert 0 < ref[3][0, 0] < plain[3][0, 0] and 0 < ref[3][0, 1] < plain[3][0, 1]
    assert ref[3][1, 1] == 0 and ref[3][1, 0] <= plain[3][1, 0]                          # the whole object erased
    e = erase[0, 1]
    hit = plain[2][0, e[1]:e[3] + 1, e[0]:e[2] + 1]
    assert {1, 2} <= set(hit.ravel().tolist())                                           # that one lies across both
    assert (ref[0][0, e[1]:e[3] + 1, e[0]:e[2] + 1] == FILL).all() and (ref[1][0, e[1]:e[3] + 1, e[0]:e[2] + 1] == 0).all()
    for E in (1, 3):
        run_compose(C, device, sc, "i32", "shared", False, erase=erase[:, :E].copy())


def desc_of(P, p, kind, N, H, W, b, Ho, Wo, S, E, background=True, instance=True):
    """A pv_cmp_desc over dense operands at the addresses p[name]."""
    d = P.CmpDesc()
    d.image, d.label, d.pick, d.shift, d.erase = p["image"], p["label"], p["pick"], p["shift"], p["erase"] if E else None
    d.background = p["background"] if background else None
    d.out_image, d.out_label, d.visible = p["out_image"], p["out_label"], p["visible"]
    d.out_instance = p["out_instance"] if instance else None
    d.image_strides[:] = (H * W * 3, W * 3, 3, 1)
    d.label_strides[:] = (H * W, W, 1)
    d.background_strides[:] = (Ho * Wo * 3, Wo * 3, 3, 1)
    d.out_image_strides[:] = (Ho * Wo * 3, Wo * 3, 3, 1)
    d.out_label_strides[:] = (Ho * Wo, Wo, 1)
    d.out_instance_strides[:] = (Ho * Wo, Wo, 1)
    d.fill[:] = FILL
    d.label_kind = LABEL_KIND[kind]
    d.N, d.H, d.W, d.b, d.Ho, d.Wo, d.S, d.E, d.ncls = N, H, W, b, Ho, Wo, S, E, NCLS
    return d


def contract_apply(device, name, sc, kind, erase, extra=None):
    """pv_compose_apply between guards, as tests/test_gpu_memory_contract.py treats the seven libraries."""
    from pvnet_amd import _compose_lib as P
    from tests.test_gpu_memory_contract import Spec, contract
    L = P.load()
    H, W, Ho, Wo = SHAPES[sc["shape"]]
    b, S, E = sc["b"], sc["S"], erase.shape[1]
    label = sc["label"].astype(LABEL_NP[kind])
    N = label.shape[0]

    def call(p, ws, nbytes, stream):
        return L.pv_compose_apply(ctypes.byref(desc_of(P, p, kind, N, H, W, b, Ho, Wo, S, E)), stream)

    ref = R.compose(sc["image"], label, sc["pick"], sc["shift"], NCLS, Ho, Wo, sc["background"], FILL, erase)

    def parity(got):
        for k, r in zip(("out_image", "out_label", "out_instance", "visible"), ref):
            same(got[k], r, f"{name}: {k}")
        if extra:
            extra(ref)

    spec = Spec(name, dict(image=sc["image"], label=label, pick=sc["pick"], shift=sc["shift"], erase=erase, background=sc["background"]),
                dict(out_image=((b, Ho, Wo, 3), np.uint8), out_label=((b, Ho, Wo), LABEL_NP[kind]),
                     out_instance=((b, Ho, Wo), LABEL_NP[kind]), visible=((b, S), np.int32)), call, P.check)
    contract(device, spec, parity)


@pytest.mark.gpu
def test_hostile_device_data(device, C):
    """INT32_MIN / INT32_MAX shifts, src = N, inverted boxes, boxes of the whole integer range, erasers with
    x1 < x0: nothing is read or written out of bounds (the guards), and the frames are background."""
    sc = dict(scene("37x53", 4))
    H, W, Ho, Wo = SHAPES["37x53"]
    N = sc["label"].shape[0]
    full = (I32.min, I32.min, I32.max, I32.max)
    bx = box_of(sc["label"], 3, 1)
    pick = np.zeros((4, 4, 8), np.int32)
    shift = np.zeros((4, 4, 2), np.int32)
    pick[0] = [(0, 1, 1, *full, 0), (1, 1, 2, *full, 0), (3, 1, 3, *bx, 0), (2, 2, 1, *full, 0)]
    shift[0] = [(I32.min, 0), (I32.max, I32.max), (0, I32.min), (I32.min, I32.min)]
    pick[1] = [(N, 1, 1, *full, 0), (I32.max, 1, 1, *bx, 0), (I32.min, 1, 1, *bx, 0), (-1, 1, 1, *bx, 0)]
    pick[2] = [(0, 1, 1, bx[2], bx[1], bx[0], bx[3], 0), (0, 1, 1, I32.max, I32.max, I32.min, I32.min, 0),
               (0, 1, I32.max, *bx, 0), (0, 1, I32.min, *bx, 0)]
    shift[2] = [(3, 3), (I32.max, I32.min), (1, 1), (I32.max, 0)]
    pick[3] = [(3, 1, 2, *full, 0), (0, 1, 1, *bx, 0), (0, 1, 1, *bx, 0), (0, 1, 1, *bx, 0)]       # one honest slot among hostile ones
    shift[3] = [(5, 4), (I32.max, 1), (1, I32.max), (I32.min, I32.max)]
    erase = np.array([[(9, 0, 8, Ho), (I32.max, I32.max, I32.min, I32.min)]] * 4, np.int32)        # both empty
    sc.update(pick=pick, shift=shift, b=4)
    sc["background"] = np.random.default_rng(11).integers(0, 256, (4, Ho, Wo, 3), dtype=np.uint8)

    def extra(ref):
        np.testing.assert_array_equal(ref[0][:3], sc["background"][:3])                  # background everywhere
        assert not ref[1][:3].any() and not ref[2][:3].any() and not ref[3][:3].any()
        assert ref[3][3].tolist() == [int((sc["label"][3] == 1).sum()), 0, 0, 0]         # and the honest slot whole

    contract_apply(device, "pv_compose_apply hostile", sc, "i32", erase, extra)


# ---- 4. the memory contract of the three entries ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(LABEL_DTYPES))
@pytest.mark.parametrize("shape,S", [("37x53", 4), ("48x64", 16)])
def test_contract_apply(device, C, shape, S, kind):
    sc = scene(shape, S)
    Ho, Wo = SHAPES[shape][2:]
    erase = np.array([[(3, 2, 9, 6), (Wo - 4, Ho - 3, Wo + 5, Ho + 5)]] * sc["b"], np.int32)
    contract_apply(device, f"pv_compose_apply {shape} S={S} {kind}", sc, kind, erase)


PARAM_KW = dict(margin=0.2, erase_frac=(0.2, 0.7), p_blur=0.6, noise=(1.0, 9.0))
SEED, FIRST = 0x0123456789ABCDEF, 2 ** 64 - 2            # the sample index wraps inside a batch


def param_pick(b=5):
    """b frames of four slots over a bank of 6 frames of 29 x 41: two live, one with src = N, one with an empty box."""
    _, label = make_bank(29, 41)
    pick = np.zeros((b, 4, 8), np.int32)
    pick[:, 0] = (0, 1, 1, *box_of(label, 0, 1), 0)
    pick[:, 1] = (3, 1, 2, -4, -4, 100, 100, 0)          # clipped to the frame
    pick[:, 2] = (6, 1, 1, 0, 0, 9, 9, 0)
    pick[:, 3] = (2, 2, 3, 9, 0, 8, 9, 0)
    pick[1:, 0, 3] += np.arange(1, b, dtype=np.int32)    # boxes of even and odd widths
    return pick


@pytest.mark.gpu
def test_contract_params(device, C):
    from pvnet_amd import _compose_lib as P
    from tests.test_gpu_memory_contract import Spec, contract
    L = P.load()
    b, S, E, N, H, W, Ho, Wo = 5, 4, 6, 6, 29, 41, 37, 53
    pick = param_pick(b)
    ref = R.params(pick, SEED, FIRST, N, H, W, Ho, Wo, NCLS, E, **PARAM_KW)

    def call(p, ws, nbytes, stream):
        r = P.CmpRanges(PARAM_KW["margin"], (ctypes.c_double * 2)(*PARAM_KW["erase_frac"]), PARAM_KW["p_blur"],
                        (ctypes.c_double * 2)(*PARAM_KW["noise"]), b, N, H, W, Ho, Wo, S, E, NCLS, 0)
        return L.pv_compose_params(ctypes.byref(r), p["pick"], p["state"], p["shift"], p["erase"], p["ksel"], p["amp"], stream)

    def parity(got):
        for k, r in zip(("shift", "erase", "ksel", "amp"), ref):
            same(got[k], r, f"pv_compose_params: {k}")

    state = np.array([SEED, FIRST], np.uint64).view(np.int64)
    contract(device, Spec("pv_compose_params", dict(pick=pick, state=state),
                          dict(shift=((b, S, 2), np.int32), erase=((b, E, 4), np.int32), ksel=((b,), np.int32), amp=((b,), np.float32)),
                          call, P.check), parity)


FINISH_SIZES = [(7, 5), (1, 1), (1, 12), (12, 1), (37, 53), (2 * R.TILE + 3, 2 * R.TILE + 3)]


@functools.lru_cache(maxsize=None)
def finish_case(size, seed=0):
    """Six frames: every k, and ksel = 7, which is 0; amplitudes from 0 to large."""
    H, W = size
    rng = np.random.default_rng([seed, H, W])
    image = rng.integers(0, 256, (6, H, W, 3), dtype=np.uint8)
    ksel = np.array([0, 1, 2, 3, 4, 7], np.int32)
    amp = np.array([3.5, 0.0, 11.0, 2.25, 60.0, 0.0], np.float32)
    return image, ksel, amp, R.finish(image, ksel, amp, SEED, FIRST)


def finish_desc(P, p, b, H, W):
    d = P.CmpFinish()
    d.image, d.out, d.ksel, d.amp, d.state = p["image"], p["out"], p["ksel"], p["amp"], p["state"]
    d.image_strides[:] = (H * W * 3, W * 3, 3, 1)
    d.out_strides[:] = (H * W * 3, W * 3, 3, 1)
    for j, row in enumerate(R.kernels().tolist()):
        d.w[j][:] = row
    d.b, d.H, d.W = b, H, W
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("size", FINISH_SIZES, ids=str)
def test_contract_finish(device, C, size):
    from pvnet_amd import _compose_lib as P
    from tests.test_gpu_memory_contract import Spec, contract
    L = P.load()
    H, W = size
    image, ksel, amp, ref = finish_case(size)

    def call(p, ws, nbytes, stream):
        return L.pv_compose_finish(ctypes.byref(finish_desc(P, p, 6, H, W)), stream)

    state = np.array([SEED, FIRST], np.uint64).view(np.int64)
    contract(device, Spec(f"pv_compose_finish {size}", dict(image=image, ksel=ksel, amp=amp, state=state),
                          dict(out=((6, H, W, 3), np.uint8)), call, P.check), lambda got: same(got["out"], ref, "finish"))


# ---- 5. params ------------------------------------------------------------------------------------------------------
def state_of(device, seed=SEED, first=FIRST):
    return cu(np.array([seed, first], np.uint64).view(np.int64), device)


@pytest.mark.gpu
def test_params(device, C):
    b, S, E, N, H, W, Ho, Wo = 5, 4, 6, 6, 29, 41, 37, 53
    pick = param_pick(b)
    state = state_of(device)
    kw = dict(margin=PARAM_KW["margin"], erasers=E, erase_frac=PARAM_KW["erase_frac"], blur_p=PARAM_KW["p_blur"],
              noise=PARAM_KW["noise"], class_num=NCLS)
    got = C.random_placement(cu(pick, device), (N, H, W), (Ho, Wo), state, **kw)
    ref = R.params(pick, SEED, FIRST, N, H, W, Ho, Wo, NCLS, E, **PARAM_KW)
    for g, r, name in zip(got, ref, got._fields):
        same(g, r, name)
    assert (ref[0][:, 2:] == 0).all() and (ref[0][:, :2] != 0).any(-1).all()
    # every drawn eraser lies inside its slot's shifted box; dead slots' are empty
    for f in range(b):
        for e in range(E):
            s = e % S
            if s >= 2:
                assert ref[1][f, e].tolist() == [0, 0, -1, -1]
                continue
            x0, y0, x1, y1 = R.clipped_box(pick[f, s], H, W)
            dx, dy = ref[0][f, s]
            ex0, ey0, ex1, ey1 = ref[1][f, e]
            assert x0 + dx <= ex0 <= ex1 <= x1 + dx and y0 + dy <= ey0 <= ey1 <= y1 + dy
    # advancing state[1] by b: every frame's draws change, and equal the reference at the new index
    state[1] += b
    again = C.random_placement(cu(pick, device), (N, H, W), (Ho, Wo), state, **kw)
    ref2 = R.params(pick, SEED, (FIRST + b) % 2 ** 64, N, H, W, Ho, Wo, NCLS, E, **PARAM_KW)
    for g, r, name in zip(again, ref2, again._fields):
        same(g, r, name + " after the advance")
    assert (ref2[0][:, :2] != ref[0][:, :2]).any((1, 2)).all() and (ref2[3] != ref[3]).all()
    # margin = 0.5: every box centre within half a pixel of the frame's centre
    mid = C.random_placement(cu(pick, device), (N, H, W), (Ho, Wo), state, margin=0.5, class_num=NCLS).shift.cpu().numpy()
    for f in range(b):
        for s in range(2):
            x0, y0, x1, y1 = R.clipped_box(pick[f, s], H, W)
            assert abs((x0 + x1) / 2 + mid[f, s, 0] - (Wo - 1) / 2) <= 0.5 and abs((y0 + y1) / 2 + mid[f, s, 1] - (Ho - 1) / 2) <= 0.5
    # E = 0 and b = 0
    none = C.random_placement(cu(pick, device), (N, H, W), (Ho, Wo), state, class_num=NCLS)
    assert tuple(none.erase.shape) == (b, 0, 4)
    assert tuple(C.random_placement(cu(pick[:0], device), (N, H, W), (Ho, Wo), state).shift.shape) == (0, S, 2)


# ---- 6. finish ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", FINISH_SIZES, ids=str)
def test_finish(device, C, size):
    """7 x 5 is narrower than the 9 taps (the reflection folds more than once); 67 x 67 crosses tile seams and
    halos in both directions; the batch's frames have different k and amp, amp = 0 with a blur, a blur off
    with amp > 0, and ksel = 7 acting as 0."""
    image, ksel, amp, ref = finish_case(size)
    state = state_of(device)
    got = C.finish(cu(image, device), cu(ksel, device), cu(amp, device), state)
    same(got, ref, f"finish {size}")
    np.testing.assert_array_equal(ref[5], image[5])                       # ksel out of range and amp = 0: the identity
    if size[0] * size[1] >= 35:
        assert (ref[0] != image[0]).any() and (ref[1] != image[1]).any()
    # strided: a CHW input and a CHW output, viewed as HWC
    chw = cu(image.transpose(0, 3, 1, 2), device)
    out = torch.zeros_like(chw)
    C.finish(chw.permute(0, 2, 3, 1), cu(ksel, device), cu(amp, device), state, out=out.permute(0, 2, 3, 1))
    same(out.permute(0, 2, 3, 1).contiguous(), ref, f"finish {size} strided")


@pytest.mark.gpu
def test_finish_identity_and_clamps(device, C):
    H, W = 37, 53
    image, _, _, _ = finish_case((H, W))
    state = state_of(device)
    zero_k, zero_a = torch.zeros(6, dtype=torch.int32, device=device), torch.zeros(6, device=device)
    got = C.finish(cu(image, device), zero_k, zero_a, state)
    same(got, image, "identity")
    for k in (-1, 5, int(I32.max), int(I32.min)):
        same(C.finish(cu(image, device), torch.full((6,), k, dtype=torch.int32, device=device), zero_a, state), image, f"ksel {k}")
    # an amplitude large enough that both clamps act, with a blur
    ksel, amp = np.full(6, 2, np.int32), np.full(6, 300.0, np.float32)
    ref = R.finish(image, ksel, amp, SEED, FIRST)
    c = R.blurred(image[0], 2) + np.float32(300.0) * R.noise_field(SEED, FIRST, H, W)
    assert (c < 0).any() and (c > 255).any() and (ref[0][c < 0] == 0).all() and (ref[0][c > 255] == 255).all()
    same(C.finish(cu(image, device), cu(ksel, device), cu(amp, device), state), ref, "clamps")
    # constant frames stay constant under every k
    for v in (0, 1, 127, 254, 255):
        const = np.full((5, 9, 40, 3), v, np.uint8)
        same(C.finish(cu(const, device), torch.arange(5, dtype=torch.int32, device=device), torch.zeros(5, device=device), state),
             const, f"constant {v}")
    assert tuple(C.finish(cu(image[:0], device), zero_k[:0], zero_a[:0], state).shape) == (0, H, W, 3)


# ---- 7. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_runs_and_two_replays_give_the_same_bits(device, C):
    sc = scene("48x64", 4)
    H, W, Ho, Wo = SHAPES["48x64"]
    image, label, pick = cu(sc["image"], device), cu(sc["label"].astype(np.uint8), device), cu(sc["pick"], device)
    bg = cu(sc["background"], device)
    state = state_of(device, 77, 0)

    def run():
        pl = C.random_placement(pick, (6, H, W), (Ho, Wo), state, erasers=3, blur_p=0.7, noise=(2.0, 9.0), class_num=NCLS)
        img, lab, inst, vis = C.compose(image, label, pick, pl.shift, NCLS, (Ho, Wo), background=bg, erase=pl.erase, want_instance=True)
        return [C.finish(img, pl.ksel, pl.amp, state), lab, inst, vis, pl.shift]

    a, b2 = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b2))
    shift, erase, ksel, amp = R.params(sc["pick"], 77, 0, 6, H, W, Ho, Wo, NCLS, 3, p_blur=0.7, noise=(2.0, 9.0))
    ref = R.compose(sc["image"], sc["label"].astype(np.uint8), sc["pick"], shift, NCLS, Ho, Wo, sc["background"], (0, 0, 0), erase)
    same(a[0], R.finish(ref[0], ksel, amp, 77, 0), "the chain's image")
    same(a[3], ref[3], "the chain's visible")
    stream = torch.cuda.Stream(device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        run()
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            out = run()
        replays = []
        for _ in range(2):
            for t in out:
                t.zero_()
            g.replay()
            stream.synchronize()
            replays.append([t.clone() for t in out])
        state[1] += sc["b"]
        g.replay()
        stream.synchronize()
    for r in replays:
        assert all(torch.equal(x, y) for x, y in zip(r, a))
    assert not torch.equal(out[4], a[4]) and not torch.equal(out[0], a[0])        # fresh draws after the advance


# ---- 8. against the renderer ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_against_the_renderer(device, C):
    """A convention the kernel and its restatement could share (which slot is on top, the shift's sign, a
    half-pixel offset) shows against the z-buffer of the renderer."""
    from pvnet_amd import render as Rn
    from tests import render_ref as RR
    from tests.test_gpu_augment import band
    from tests.test_gpu_render import loop_scene
    s = loop_scene()
    H, W = 96, 128
    K = np.array([[200.0, 0.0, 63.5], [0.0, 200.0, 47.5], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(4)
    far, near = RR.pose(RR.random_rotation(rng), (0.0, 0.0, 0.62)), RR.pose(RR.random_rotation(rng), (0.03, 0.01, 0.40))
    radius = [float(np.linalg.norm(m[0].astype(np.float64), axis=1).max()) for m in s["models"]]
    assert far[2, 3] - radius[0] > near[2, 3] + radius[1]                  # depth ranges disjoint: the near one wins wherever both cover
    table = Rn.MeshTable(s["models"], device=device)
    mid = torch.tensor([[0], [1]], dtype=torch.int32, device=device)
    singles = Rn.render_labels(table, cu(np.array([far, near]).reshape(2, 1, 3, 4), device), mid, None, cu(K, device), H, W,
                               want=("label",))["label"]
    diag = {}
    joint = Rn.render_labels(table, cu(np.array([far, near]).reshape(1, 2, 3, 4), device), mid.reshape(1, 2), None, cu(K, device),
                             H, W, want=("label",), diag=diag)["label"]
    stats = AR.label_stats(singles.cpu().numpy(), 2)
    assert stats[:, 0].min() > 300
    pick = C.make_picks(torch.tensor([[0, 1]], device=device), torch.tensor([[1, 2]], device=device),
                        cu(stats, device), src_label=torch.tensor([[1, 2]], device=device))      # the far one first
    bank_image = torch.zeros((2, H, W, 3), dtype=torch.uint8, device=device)
    zero = torch.zeros((1, 2, 2), dtype=torch.int32, device=device)
    _, lab, _, vis = C.compose(bank_image, singles, pick, zero, 2, (H, W))
    assert torch.equal(lab, joint)
    won = diag["won"].cpu().numpy().reshape(2)
    assert vis.cpu().numpy().reshape(2).tolist() == won.tolist() and 0 < won[0] < stats[0, 0] and won[1] == stats[1, 0]
    # shifted: the render under shift_camera(K, shift), outside the one-pixel boundary band
    shift = torch.tensor([[[7, -5], [-12, 5]]], dtype=torch.int32, device=device)
    Ks = C.shift_camera(cu(K, device), shift)
    moved = Rn.render_labels(table, cu(np.array([far, near]).reshape(2, 1, 3, 4), device), mid, None, Ks[0], H, W,
                             want=("label",))["label"].cpu().numpy()
    want = np.where(moved[1] > 0, moved[1], moved[0])
    _, lab2, _, vis2 = C.compose(bank_image, singles, pick, shift, 2, (H, W))
    lab2 = lab2.cpu().numpy()[0]
    for st in (stats, AR.label_stats(moved, 2)):                               # every object whole, before and after
        assert (st[:, 3:5] >= 1).all() and (st[:, 5] <= W - 2).all() and (st[:, 6] <= H - 2).all()
    differ = lab2 != want
    outside = int((differ & ~(band(moved[0] > 0) | band(moved[1] > 0))).sum())
    print(f"shifted compose against the shifted cameras: {int(differ.sum())} differ, {outside} outside the band")
    assert outside == 0 and (lab2 == 1).sum() > 100 and (lab2 == 2).sum() > 300
    same(lab2[None], R.compose(np.zeros((2, H, W, 3), np.uint8), singles.cpu().numpy(), pick.cpu().numpy(), shift.cpu().numpy(), 2, H, W)[1],
         "shifted label")


# ---- 9. the loop closes, and a training step --------------------------------------------------------------------------
def rendered_bank(device, frame=2):
    """The two objects of loop_scene()'s frame 2, each alone in a 480 x 640 frame: the box first, so the
    ellipsoid (pasted later) occludes it."""
    from pvnet_amd import render as Rn
    from tests.test_gpu_render import loop_scene
    s = loop_scene()
    H, W, K = s["H"], s["W"], cu(s["K"], device)
    table = Rn.MeshTable(s["models"], device=device)
    order = [1, 0]
    poses = cu(s["poses"][frame][order].reshape(2, 1, 3, 4), device)
    mid = torch.tensor(order, dtype=torch.int32, device=device).reshape(2, 1)
    label, _, kp = Rn.render_ground_truth(table, s["p3"], poses, mid, K, H, W)
    bank_kp = torch.stack([kp[i, c] for i, c in enumerate(order)])                       # [2, 9, 2]
    gen = torch.Generator(device=device).manual_seed(5)
    image = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, device=device, generator=gen)
    return s, image, label, bank_kp, order


@pytest.mark.gpu
def test_loop_closes_through_the_composition(device, C):
    from pvnet_amd import augment as A
    from pvnet_amd import ransac_voting_gpu as rvg
    from pvnet_amd import render as Rn
    from tests.test_gpu_render import CPU_WORST
    s, image, label, bank_kp, order = rendered_bank(device)
    H, W = s["H"], s["W"]
    stats = A.label_stats(label, 2)
    b = 4
    src = torch.tensor([[0, 1]] * b, device=device)
    cls = torch.tensor([[c + 1 for c in order]] * b, device=device)
    pick = C.make_picks(src, cls, stats, src_label=cls)
    state = torch.tensor([2024, 0], dtype=torch.int64, device=device)
    out = C.compose_ground_truth(image, label, bank_kp, pick, 2, (H, W), state, margin=0.45, layout="bhwk2")
    assert tuple(out["image"].shape) == (b, H, W, 3) and out["image"].dtype == torch.uint8
    assert tuple(out["vertex"].shape) == (b, H, W, 18, 2) and tuple(out["keypoints_2d"].shape) == (b, 2, 9, 2)
    assert bool(out["present"].all())
    # the pieces are the documented ones
    pl = C.random_placement(pick, (2, H, W), (H, W), state, margin=0.45, class_num=2)
    assert all(torch.equal(x, y) for x, y in zip(pl, out["placement"]))
    kp, _ = C.shift_keypoints(bank_kp, pick, pl.shift, 2)
    assert torch.equal(kp, out["keypoints_2d"])
    assert torch.equal(kp[:, 0], bank_kp[1][None].double() + pl.shift[:, 1, None].double())
    img, lab, _, vis = C.compose(image, label, pick, pl.shift, 2, (H, W))
    assert torch.equal(lab, out["label"]) and torch.equal(vis, out["visible"])
    assert torch.equal(C.finish(img, pl.ksel, pl.amp, state), out["image"])
    assert torch.equal(out["vertex"], Rn.vertex_field(lab, kp, 2))
    # real occlusion: the box shows in part, the ellipsoid whole, and both have enough pixels to vote
    frac = C.visible_fraction(vis, stats[src, 0]).cpu().numpy()
    print("visible fractions (box, ellipsoid):", frac.round(3).tolist(), "visible pixels:", vis.cpu().numpy().tolist())
    assert ((frac[:, 0] > 0) & (frac[:, 0] < 1)).all() and (frac[:, 1] == 1).all()
    assert int(vis.min()) >= 500
    area = torch.stack([(lab == c + 1).sum((1, 2)) for c in range(2)], 1)
    assert torch.equal(area[:, [1, 0]].to(torch.int32), vis)
    got = rvg.ransac_voting_layer_v3_multi(lab, out["vertex"], 2, 512, _seed=20240)
    kp_err = float((got.to(torch.float64) - kp).norm(dim=-1).max())
    print(f"loop through the composition: keypoints {kp_err:.3e} px (bound {4 * CPU_WORST['keypoint_px']:.3e})")
    assert kp_err <= 4 * CPU_WORST["keypoint_px"]


@pytest.mark.gpu
def test_a_training_step_on_a_composed_batch(device, C):
    from pvnet_amd import augment as A
    from pvnet_amd.net_utils import pvnet_loss
    from pvnet_amd.network import PVNet
    s, image, label, bank_kp, order = rendered_bank(device)
    H, W = s["H"], s["W"]
    stats = A.label_stats(label, 2)
    src = torch.tensor([[0, 1]] * 2, device=device)
    cls = torch.tensor([[c + 1 for c in order]] * 2, device=device)
    pick = C.make_picks(src, cls, stats, src_label=cls)
    state = torch.tensor([7, 0], dtype=torch.int64, device=device)
    out = C.compose_ground_truth(image, label, bank_kp, pick, 2, (H, W), state, margin=0.4, erasers=2, blur_p=1.0, noise=(2.0, 6.0))
    assert bool((out["placement"].ksel > 0).all()) and int(out["visible"].min()) > 500
    img, lab, vertex, kp = A.augment_ground_truth(out["image"], out["label"], out["keypoints_2d"], 2, state, out_size=(64, 96),
                                                  scale=(0.2, 0.3), margin=0.4)
    assert tuple(img.shape) == (2, 3, 64, 96) and tuple(vertex.shape) == (2, 36, 64, 96)
    assert int((lab > 0).sum()) > 50
    torch.manual_seed(0)
    net = PVNet(ver_dim=36, seg_dim=3).to(device).train()
    seg_pred, ver_pred = net(img)
    loss_seg, loss_vertex, _ = pvnet_loss(seg_pred, ver_pred, lab, vertex, class_num=2)
    loss = loss_seg.mean() + loss_vertex.mean()
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)


# ---- 10. the Python layer on the device ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_errors_and_empty_batches(device, C):
    sc = scene("37x53", 4)
    H, W, Ho, Wo = SHAPES["37x53"]
    image, label = cu(sc["image"], device), cu(sc["label"].astype(np.uint8), device)
    pick, shift = cu(sc["pick"], device), cu(sc["shift"], device)
    with pytest.raises(RuntimeError, match="device"):
        C.compose(image, label.cpu(), pick, shift, NCLS, (Ho, Wo))
    with pytest.raises(RuntimeError, match="device"):
        C.random_placement(pick, (6, H, W), (Ho, Wo), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="alias"):
        C.finish(image, torch.zeros(6, dtype=torch.int32, device=device), torch.zeros(6, device=device), state_of(device), out=image)
    img, lab, inst, vis = C.compose(image, label, pick[:0], shift[:0], NCLS, (Ho, Wo), want_instance=True)
    assert tuple(img.shape) == (0, Ho, Wo, 3) and tuple(lab.shape) == (0, Ho, Wo) == tuple(inst.shape) and tuple(vis.shape) == (0, 4)
