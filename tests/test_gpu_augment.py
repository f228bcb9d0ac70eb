"""libpvaugment.so on the device (include/pvaugment.h, pvnet_amd/augment.py) against tests/augment_ref.py.

Labels are compared exactly in every case: the geometry is fp64 in a fixed order.  The image is compared
with the numpy f64 evaluation of the same chain under a bound worked out from the chain's f32 roundings
(``image_bound``), set before any run; every check prints the fraction of the bound it used."""
import functools

import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests import render_ref as RR

EPS = 2.0 ** -24                    # half an ulp of an f32 in [1, 2): the relative error of one rounding
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL = (12.0, 200.0, 77.0)
LABEL_DTYPES = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
SHAPES = {"37x53": (37, 53, 29, 41), "48x64": (48, 64, 48, 64)}
USED = {}                           # check -> the largest fraction of its bound seen (printed per check)


@pytest.fixture(scope="module")
def A(device):
    import __graft_entry__ as g
    g.build()
    from pvnet_amd import augment
    return augment


def cu(a, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(device)


def image_bound(color, flags):
    """The absolute error of the device's f32 chain on [0, 1] values, per image, from its roundings.

    warp: on the 0..255 scale top and bot take 2 roundings each of values <= 255 (the tap differences
    are exact: integers), bot - top 1, the product 1, the sum 1, and carry 4 + 2 of top / bot: 10 in all,
    then the constant 1/255 and the product, 2: 12 EPS.  Each photometric step multiplies the error it
    inherits by its own Lipschitz factor and adds its roundings (clamp and grey, whose weights sum to 1,
    do not expand):
      brightness  beta (e + EPS)
      contrast    kappa e + |1 - kappa| (e + 6 EPS) + (kappa + 4) EPS    (grey: 5, the mean's cast: 1; the sum is f64)
      saturation  sigma e + |1 - sigma| (e + 5 EPS) + (sigma + 4) EPS
      hue         12 e + 50 EPS: the hue's error is e / delta, delta = max - min, and returns multiplied by
                  6 s v = 6 delta (8 e), s and v add 3 e + e, and about 50 roundings of values <= 6
    """
    beta, kappa, sigma, _ = (abs(float(v)) for v in color)
    e = 12 * EPS
    if flags & R.BRIGHTNESS:
        e = beta * (e + EPS)
    if flags & R.CONTRAST:
        e = kappa * e + abs(1 - kappa) * (e + 6 * EPS) + (kappa + 4) * EPS
    if flags & R.SATURATION:
        e = sigma * e + abs(1 - sigma) * (e + 5 * EPS) + (sigma + 4) * EPS
    if flags & R.HUE:
        e = 12 * e + 50 * EPS
    return e


def check_image(name, got, ref, color, flags, half):
    """got [b][3][Ho][Wo] from the device (as float64), ref the numpy f64 evaluation."""
    worst = 0.0
    for i in range(ref.shape[0]):
        # the normalisation: (c - mean) rounds once, the product once, 1 / std is the same f32 on both sides
        bound = (image_bound(color[i], flags) + 2 * EPS) / min(STD) + 2 * EPS * np.abs(ref[i])
        if half:
            bound = bound + np.abs(ref[i]) * 2.0 ** -11 + 2.0 ** -25      # half an f16 ulp of the value
        worst = max(worst, float((np.abs(got[i] - ref[i]) / bound).max()))
    USED[name] = max(USED.get(name, 0.0), worst)
    print(f"{name}: {worst:.3f} of the bound")
    assert worst <= 1.0, f"{name}: {worst} of the bound"


@functools.lru_cache(maxsize=None)
def scene(shape, seed=0, b=3):
    """u8 image, label (0..3), per-image matrices and jitters from the restatement's own draw."""
    H, W, Ho, Wo = SHAPES[shape]
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (b, H, W, 3), dtype=np.uint8)
    image[0, : H // 2] = image[0, : H // 2, :, :1]                         # greys: the hue's flat branch
    label = np.zeros((b, H, W), np.uint8)
    for i in range(b):
        label[i, 5 + i:H - 9, 7:W - 11 - i] = rng.integers(0, 4, (H - 14 - i, W - 18 - i))
    background = rng.integers(0, 256, (b, Ho, Wo, 3), dtype=np.uint8)
    _, inv, color, _ = R.params(R.label_stats(label, 3), 11 + seed, 5, H, W, Ho, Wo, rot_deg=(-180.0, 180.0),
                                scale=(0.6, 1.7), margin=0.2, jitter=(0.4, 0.4, 0.4, 0.3))
    return dict(image=image, label=label, background=background, inv=inv, color=color)


@functools.lru_cache(maxsize=None)
def reference(shape, with_bg, fill, flags):
    s = scene(shape)
    _, _, Ho, Wo = SHAPES[shape]
    return R.apply(s["image"], s["label"], s["inv"], s["color"], Ho, Wo, s["background"] if with_bg else None, fill,
                   MEAN, STD, flags)


def params_of(A, s, device):
    inv = cu(s["inv"], device)
    return A.AugmentParams(inv.clone(), inv, cu(s["color"], device))


STEPS = {0: (), 1: ("brightness",), 2: ("contrast",), 4: ("saturation",), 8: ("hue",),
         15: ("brightness", "contrast", "saturation", "hue")}


# ---- 1. parity -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["dense", "channels_last"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", list(LABEL_DTYPES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity(device, A, shape, kind, dtype, layout):
    s = scene(shape)
    H, W, Ho, Wo = SHAPES[shape]
    ref, ref_lab = reference(shape, True, FILL, R.ALL)
    img, lab = A.apply(cu(s["image"], device), cu(s["label"], device, LABEL_DTYPES[kind]), params_of(A, s, device),
                       background=cu(s["background"], device), fill=FILL, dtype=dtype, out_size=(Ho, Wo),
                       channels_last=layout == "channels_last")
    assert img.dtype == dtype and tuple(img.shape) == (3, 3, Ho, Wo) and lab.dtype == LABEL_DTYPES[kind]
    assert img.is_contiguous(memory_format=torch.channels_last if layout == "channels_last" else torch.contiguous_format)
    np.testing.assert_array_equal(lab.cpu().numpy(), ref_lab)
    assert (ref_lab > 0).any() and (ref_lab == 0).any()
    check_image(f"parity {shape} {dtype} {layout}", img.double().cpu().numpy(), ref, s["color"], R.ALL, dtype == torch.float16)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bg", [False, True], ids=["no_bg", "bg"])
@pytest.mark.parametrize("flags", list(STEPS))
def test_parity_each_step(device, A, flags, with_bg):
    s = scene("37x53")
    H, W, Ho, Wo = SHAPES["37x53"]
    fill = FILL if flags in (0, 15) else (0.0, 0.0, 0.0)
    ref, ref_lab = reference("37x53", with_bg, fill, flags)
    bg = cu(s["background"][:1] if flags == 4 else s["background"], device) if with_bg else None     # one shared, or one each
    if with_bg and flags == 4:
        ref, ref_lab = R.apply(s["image"], s["label"], s["inv"], s["color"], Ho, Wo, s["background"][:1], fill, MEAN, STD, flags)
    img, lab = A.apply(cu(s["image"], device), cu(s["label"], device), params_of(A, s, device), background=bg, fill=fill,
                       out_size=(Ho, Wo), steps=STEPS[flags])
    np.testing.assert_array_equal(lab.cpu().numpy(), ref_lab)
    check_image(f"steps {flags} bg {with_bg}", img.double().cpu().numpy(), ref, s["color"], flags, False)


@pytest.mark.gpu
def test_strided_sources_and_outputs(device, A):
    """A cropped view of a larger CHW batch and of a larger label map, and outputs that are views."""
    s = scene("37x53")
    H, W, Ho, Wo = SHAPES["37x53"]
    ref, ref_lab = reference("37x53", True, FILL, R.ALL)
    big = torch.full((3, 3, H + 5, W + 7), 255, dtype=torch.uint8, device=device)
    big[:, :, 2:2 + H, 3:3 + W] = cu(s["image"], device).permute(0, 3, 1, 2)
    big_lab = torch.full((3, H + 5, 2 * (W + 7)), 3, dtype=torch.int32, device=device)
    big_lab[:, 2:2 + H, 6:6 + 2 * W:2] = cu(s["label"], device, torch.int32)
    image = big[:, :, 2:2 + H, 3:3 + W].permute(0, 2, 3, 1)
    label = big_lab[:, 2:2 + H, 6:6 + 2 * W:2]
    assert not image.is_contiguous() and not label.is_contiguous()
    out_img = torch.full((3, 3, Ho + 2, Wo + 3), 7.0, device=device)
    out_lab = torch.full((3, Ho + 1, Wo + 2), 9, dtype=torch.int32, device=device)
    bg = cu(s["background"], device).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    img, lab = A.apply(image, label, params_of(A, s, device), background=bg, fill=FILL, out_size=(Ho, Wo),
                       out=(out_img[:, :, 1:1 + Ho, 2:2 + Wo], out_lab[:, 1:, 1:1 + Wo]))
    np.testing.assert_array_equal(lab.cpu().numpy(), ref_lab)
    check_image("strided", img.double().cpu().numpy(), ref, s["color"], R.ALL, False)
    # nothing outside the views was written
    out_img[:, :, 1:1 + Ho, 2:2 + Wo] = 7.0
    out_lab[:, 1:, 1:1 + Wo] = 9
    assert bool((out_img == 7.0).all()) and bool((out_lab == 9).all())


# ---- 2. exact geometric cases ----------------------------------------------------------------------------------
def normalised(c255):
    """The header's f32 chain without a photometric step: u8 values [..., 3] -> f32 [..., 3]."""
    c = c255.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    return (c - np.array(MEAN, np.float32)) * (np.float32(1.0) / np.array(STD, np.float32))


def run_plain(A, device, image, label, inv, out_size, fill=0, dtype=torch.float32):
    b = image.shape[0]
    inv = cu(np.broadcast_to(np.asarray(inv, np.float64), (b, 2, 3)), device)
    prm = A.AugmentParams(inv, inv, torch.ones((b, 4), device=device))
    img, lab = A.apply(cu(image, device), cu(label, device), prm, fill=fill, out_size=out_size, steps=(), dtype=dtype)
    return img.cpu().numpy().transpose(0, 2, 3, 1), lab.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(37, 53), (48, 64), (5, 7), (3, 9), (1, 1)], ids=str)
def test_identity_is_a_bit_exact_normalised_copy(device, A, shape):
    H, W = shape
    rng = np.random.default_rng(H)
    image = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    label = rng.integers(0, 3, (2, H, W)).astype(np.uint8)
    img, lab = run_plain(A, device, image, label, [[1, 0, 0], [0, 1, 0]], (H, W))
    np.testing.assert_array_equal(lab, label)
    np.testing.assert_array_equal(img, normalised(image))
    half, _ = run_plain(A, device, image, label, [[1, 0, 0], [0, 1, 0]], (H, W), dtype=torch.float16)
    np.testing.assert_array_equal(half, normalised(image).astype(np.float16))


@pytest.mark.gpu
def test_integer_translation_and_quarter_turns_are_exact(device, A):
    H, W = 21, 30
    rng = np.random.default_rng(5)
    image = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    label = rng.integers(1, 4, (1, H, W)).astype(np.uint8)
    fill = (3.0, 250.0, 128.0)

    def expect(src_of, Ho, Wo):
        """src_of(x, y) -> the source pixel (sx, sy) of output (x, y)."""
        img = np.zeros((1, Ho, Wo, 3), np.uint8)
        lab = np.zeros((1, Ho, Wo), np.uint8)
        img[:] = np.array(fill, np.uint8)
        for y in range(Ho):
            for x in range(Wo):
                sx, sy = src_of(x, y)
                if 0 <= sx < W and 0 <= sy < H:
                    img[0, y, x], lab[0, y, x] = image[0, sy, sx], label[0, sy, sx]
        return normalised(img), lab

    cases = [
        ([[1, 0, 4], [0, 1, -3]], (H, W), lambda x, y: (x + 4, y - 3)),                 # a shift
        ([[1, 0, -40], [0, 1, 0]], (H, W), lambda x, y: (x - 40, y)),                   # a shift past the frame
        ([[0, 1, 2], [-1, 0, 18]], (W, H), lambda x, y: (y + 2, 18 - x)),               # a quarter turn about a pixel
        ([[0, -1, 25], [1, 0, -1]], (W, H), lambda x, y: (25 - y, x - 1)),              # the other way
        ([[-1, 0, 29], [0, -1, 20]], (H, W), lambda x, y: (29 - x, 20 - y)),            # a half turn
        ([[1, 0, 0], [0, 1, 0]], (H + 4, W + 13), lambda x, y: (x, y)),                 # padding to a larger frame
        ([[1, 0, 6], [0, 1, 5]], (9, 7), lambda x, y: (x + 6, y + 5)),                  # a crop, Wo < 8
    ]
    for inv, (Ho, Wo), src_of in cases:
        img, lab = run_plain(A, device, image, label, inv, (Ho, Wo), fill=fill)
        want_img, want_lab = expect(src_of, Ho, Wo)
        np.testing.assert_array_equal(lab, want_lab, err_msg=str(inv))
        np.testing.assert_array_equal(img, want_img, err_msg=str(inv))


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(1, 1, 6, 11), (9, 13, 1, 1), (1, 1, 1, 1), (6, 10, 5, 7), (6, 10, 5, 9), (6, 10, 3, 17)], ids=str)
def test_small_and_odd_sizes(device, A, sizes):
    """A 1 x 1 source, a 1 x 1 output, and output widths that are no multiple of a lane's 8 pixels."""
    H, W, Ho, Wo = sizes
    rng = np.random.default_rng(sum(sizes))
    image = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    label = rng.integers(1, 4, (2, H, W)).astype(np.uint8)
    inv = np.array([[[0.61803, -0.27183, 0.31416 - 1.0], [0.14142, 0.57722, -0.69315]],
                    [[0.41421, 0.10101, -0.12345], [-0.05772, 0.33333, 0.23456]]])
    color = np.array([[1.2, 0.8, 1.1, 0.1], [0.9, 1.3, 0.7, -0.2]], np.float32)
    ref, ref_lab = R.apply(image, label, inv, color, Ho, Wo, None, FILL, MEAN, STD, R.ALL)
    prm = A.AugmentParams(cu(inv, device), cu(inv, device), cu(color, device))
    img, lab = A.apply(cu(image, device), cu(label, device), prm, fill=FILL, out_size=(Ho, Wo))
    np.testing.assert_array_equal(lab.cpu().numpy(), ref_lab)
    check_image(f"sizes {sizes}", img.double().cpu().numpy(), ref, color, R.ALL, False)


# ---- 3. outside ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_outside_and_non_finite_matrices(device, A):
    """Everything outside, and matrices holding NaN, +-inf and 1e300: the range check is made in fp64
    before any conversion to an integer, so these read nothing and give fill (or background) and label 0."""
    H, W, Ho, Wo = 19, 27, 23, 21
    rng = np.random.default_rng(9)
    base = np.array([[0.9, -0.3, 2.0], [0.3, 0.9, -1.0]])
    mats = [np.array([[1.0, 0.0, 1e6], [0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, -1e6]]),
            np.array([[1.0, 0.0, float(W)], [0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, -(Ho + 1.0)]])]
    for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300):
        for pos in ((0, 2), (1, 2), None):
            M = base.copy()
            if pos is None:
                M[:] = bad
            else:
                M[pos] = bad
            mats.append(M)
    mats.append(np.array([[np.inf, -np.inf, np.nan], [1e300, 1e300, -1e300]]))
    mats.append(np.array([[1e300, 1e300, 1e300], [np.nan, 0.0, 0.0]]))
    inv = np.stack(mats)
    b = len(mats)
    image = np.broadcast_to(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8), (b, H, W, 3))
    label = np.broadcast_to(rng.integers(1, 4, (1, H, W)).astype(np.uint8), (b, H, W))
    background = rng.integers(0, 256, (1, Ho, Wo, 3), dtype=np.uint8)
    color = np.ones((b, 4), np.float32)
    color[:, 3] = 0
    for kind in LABEL_DTYPES.values():
        prm = A.AugmentParams(cu(inv, device), cu(inv, device), cu(color, device))
        img, lab = A.apply(cu(image, device), cu(label, device, kind), prm, fill=FILL, out_size=(Ho, Wo), steps=())
        assert not bool(lab.any())
        want = normalised(np.array(FILL, np.uint8)[None, None, None])
        np.testing.assert_array_equal(img.cpu().numpy().transpose(0, 2, 3, 1), np.broadcast_to(want, (b, Ho, Wo, 3)))
    img, lab = A.apply(cu(image, device), cu(label, device), prm, background=cu(background, device), fill=FILL,
                       out_size=(Ho, Wo), steps=())
    assert not bool(lab.any())
    np.testing.assert_array_equal(img.cpu().numpy().transpose(0, 2, 3, 1), np.broadcast_to(normalised(background), (b, Ho, Wo, 3)))
    # with every step on, the all-fill image is still what the restatement says (its contrast mean included)
    ref, ref_lab = R.apply(image[:4], label[:4], inv[:4], color[:4] * np.float32(1.1), Ho, Wo, None, FILL, MEAN, STD, R.ALL)
    prm = A.AugmentParams(cu(inv[:4], device), cu(inv[:4], device), cu(color[:4] * np.float32(1.1), device))
    img, lab = A.apply(cu(image[:4], device), cu(label[:4], device), prm, fill=FILL, out_size=(Ho, Wo))
    assert not ref_lab.any() and not bool(lab.any())
    check_image("outside, all steps", img.double().cpu().numpy(), ref, color[:4] * np.float32(1.1), R.ALL, False)


# ---- 4. statistics and parameters ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(LABEL_DTYPES))
def test_label_stats_exact(device, A, kind):
    H, W = 67, 131                                    # 2 blocks of 8,192 pixels an image, the second one partial
    rng = np.random.default_rng(12)
    label = rng.integers(0, 6, (5, H, W)).astype(np.int64)
    label[1] = 0                                      # the empty map
    label[2] = 0
    label[2, 40, 77] = 2                              # a one-pixel object
    label[3] = np.where(label[3] == 1, 1, 5)          # only labels outside 1..ncls besides class 1 ...
    label[4, :, :50] = 0
    label[4, 60:] = 0
    if kind != "u8":
        label[0, 0, 0], label[0, 1, 1] = -1, 2 ** 20  # ... and, where the kind holds them, negative and huge ones
    for ncls in (1, 3, 5):
        got = A.label_stats(cu(label, device, LABEL_DTYPES[kind]), ncls).cpu().numpy()
        np.testing.assert_array_equal(got, R.label_stats(label, ncls))
    assert got[1].tolist() == [0, 0, 0, W, H, -1, -1, 0] and got[2].tolist() == [1, 77, 40, 77, 40, 77, 40, 0]
    # a strided view; a second call overwrites (nothing accumulates across calls)
    view = cu(label, device, LABEL_DTYPES[kind])[:, 3:60:2, 5:120:3]
    for _ in range(2):
        np.testing.assert_array_equal(A.label_stats(view, 4).cpu().numpy(), R.label_stats(label[:, 3:60:2, 5:120:3], 4))


@pytest.mark.gpu
def test_params_draws_and_matrices(device, A):
    H, W, Ho, Wo = 67, 131, 48, 80
    rng = np.random.default_rng(13)
    b = 70                                             # more than one block of one-thread-per-image
    label = np.zeros((b, H, W), np.uint8)
    for i in range(b - 1):                             # the last image has no foreground
        x0, y0 = rng.integers(0, W - 20), rng.integers(0, H - 20)
        label[i, y0:y0 + rng.integers(1, 20), x0:x0 + rng.integers(1, 20)] = rng.integers(1, 3)
    seed, first = 0x0123456789ABCDEF, 2 ** 64 - 30     # the sample index wraps inside the batch
    kw = dict(rot_deg=(-180.0, 180.0), scale=(0.5, 2.0), margin=0.1, jitter=(0.4, 0.3, 0.2, 0.5))
    state = torch.from_numpy(np.array([seed, first], np.uint64).view(np.int64)).to(device)
    lab = cu(label, device)
    p = A.random_params(lab, 2, (Ho, Wo), state, **kw)
    fwd, inv, color, info = R.params(R.label_stats(label, 2), seed, first, H, W, Ho, Wo, **kw)
    got_f, got_i, got_c = p.fwd.cpu().numpy(), p.inv.cpu().numpy(), p.color.cpu().numpy()
    # the draws are bit-equal: the colour factors and the target involve no cos / sin
    np.testing.assert_array_equal(got_c, color)
    c = info["c"]
    np.testing.assert_allclose(np.einsum("bij,bj->bi", got_f, np.concatenate([c, np.ones((b, 1))], 1)), info["t"], rtol=0, atol=1e-10)
    # the matrices: the device's cos and sin may differ from libm in the last ulps
    scale_f = np.abs(fwd).max((1, 2), keepdims=True)
    scale_i = np.abs(inv).max((1, 2), keepdims=True)
    assert (np.abs(got_f - fwd) <= 1e-12 * scale_f).all() and (np.abs(got_i - inv) <= 1e-12 * scale_i).all()
    eye = np.broadcast_to(np.eye(2), (b, 2, 2))
    np.testing.assert_allclose(got_f[:, :, :2] @ got_i[:, :, :2], eye, atol=1e-12)
    np.testing.assert_allclose(info["c"][-1], [(W - 1) / 2, (H - 1) / 2])
    # the same state: the same bits; the state is not written
    q = A.random_params(lab, 2, (Ho, Wo), state, **kw)
    for x, y in zip(p, q):
        assert torch.equal(x, y)
    assert state.cpu().numpy().view(np.uint64).tolist() == [seed, first % 2 ** 64]
    # a state advanced by b: all-different draws
    state2 = state.clone()
    state2[1] += b
    r = A.random_params(lab, 2, (Ho, Wo), state2, **kw)
    np.testing.assert_array_equal(r.color.cpu().numpy(), R.params(R.label_stats(label, 2), seed, (first + b) % 2 ** 64, H, W, Ho, Wo, **kw)[2])
    for j, k in ((0, 0), (1, 0), (0, 2), (1, 2)):       # the angle, the scale and the two targets
        assert not np.isin(r.fwd.cpu().numpy()[:, j, k], got_f[:, j, k]).any()
    # the defaults are ColorJitter(0.1, 0.1, 0.05, 0.05), +-30 degrees, 0.8..1.2
    d = A.random_params(lab, 2, (Ho, Wo), state)
    np.testing.assert_array_equal(d.color.cpu().numpy(), R.params(R.label_stats(label, 2), seed, first, H, W, Ho, Wo)[2])


# ---- 5. determinism --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_runs_and_two_replays_give_the_same_bits(device, A):
    s = scene("48x64")                                  # 48 x 8 groups: two blocks an image; contrast is on
    H, W, Ho, Wo = SHAPES["48x64"]
    image, label, bg, prm = cu(s["image"], device), cu(s["label"], device), cu(s["background"], device), params_of(A, s, device)
    assert -(-Ho * -(-Wo // 8) // 256) > 1

    def run(out=None):
        return A.apply(image, label, prm, background=bg, fill=FILL, dtype=torch.float16, out_size=(Ho, Wo), out=out)

    a_img, a_lab = run()
    b_img, b_lab = run()
    assert torch.equal(a_img, b_img) and torch.equal(a_lab, b_lab)
    stream = torch.cuda.Stream(device)
    out = (torch.zeros_like(a_img), torch.zeros_like(a_lab))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        run(out)
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            run(out)
        replays = []
        for _ in range(2):
            out[0].zero_()
            out[1].zero_()
            g.replay()
            stream.synchronize()
            replays.append((out[0].clone(), out[1].clone()))
    for r_img, r_lab in replays:
        assert torch.equal(r_img, a_img) and torch.equal(r_lab, a_lab)


# ---- 6. geometry against the renderer --------------------------------------------------------------------------
WARPS = [(25.0, 0.9, (5.25, -3.5)), (-140.0, 1.2, (-7.5, 4.0)), (90.0, 1.0, (0.0, 0.0)), (7.0, 0.6, (20.3, 11.9))]


def band(mask):
    """3 x 3 dilation minus 3 x 3 erosion of a boolean [H][W] mask."""
    p = np.pad(mask, 1)
    H, W = mask.shape
    sh = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    q = np.pad(mask, 1, constant_values=True)
    er = np.stack([q[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return sh.any(0) & ~er.all(0)


@pytest.mark.gpu
def test_geometry_against_the_renderer(device, A):
    """A convention error the kernel and its restatement could share (forward for inverse, the angle's sign
    with y down, a half-pixel offset) shows against a second render under the transformed camera."""
    from pvnet_amd import render as Rn
    H, W = 96, 128
    K = np.array([[120.0, 0.0, 63.5], [0.0, 120.0, 47.5], [0.0, 0.0, 1.0]])
    t = np.array([0.01, -0.005, 0.4])
    models = [RR.box(), RR.bumpy_ellipsoid(2)]
    table = Rn.MeshTable(models, device=device)
    rng = np.random.default_rng(21)
    poses, poses2, Ks2, invs, mids = [], [], [], [], []
    for mid in range(2):
        for deg, s, d in WARPS:
            Rm = RR.random_rotation(rng)
            th = np.deg2rad(deg)
            c, sn = (0.0, 1.0) if deg == 90.0 else (np.cos(th), np.sin(th))
            Rz = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
            poses.append(RR.pose(Rm, t))
            poses2.append(RR.pose(Rz @ Rm, Rz @ t))
            K2 = K.copy()
            K2[0, 0] = K2[1, 1] = 120.0 * s
            K2[:2, 2] += d
            Ks2.append(K2)
            # forward: p' = s R (p - c) + c + d; the sampler takes its inverse
            sR = s * Rz[:2, :2]
            cc = K[:2, 2]
            Mi = np.linalg.inv(np.vstack([np.column_stack([sR, cc + np.array(d) - sR @ cc]), [0, 0, 1]]))[:2]
            if deg == 90.0:
                # exactly p = R^T (p' - c) + c: the centre is a pair of half-integers, their sum and difference integers
                Mi = np.array([[0.0, 1.0, cc[0] - cc[1]], [-1.0, 0.0, cc[1] + cc[0]]])
            invs.append(Mi)
            mids.append(mid)
    n = len(mids)
    mid_t = cu(np.array(mids, np.int32).reshape(n, 1), device)
    first = Rn.render_labels(table, cu(np.array(poses).reshape(n, 1, 3, 4), device), mid_t, None, cu(K, device), H, W,
                             want=("label",))["label"]
    again = Rn.render_labels(table, cu(np.array(poses2).reshape(n, 1, 3, 4), device), mid_t, None, cu(np.array(Ks2), device),
                             H, W, want=("label",))["label"].cpu().numpy()
    inv = cu(np.array(invs), device)
    image = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=device)
    _, warped = A.apply(image, first, A.AugmentParams(inv, inv, torch.ones((n, 4), device=device)), steps=())
    warped = warped.cpu().numpy()
    first = first.cpu().numpy()
    for i in range(n):
        chain = R.warp_label(first[i], invs[i], H, W)
        np.testing.assert_array_equal(warped[i], chain)                  # both stages are exact
        a, m = warped[i] > 0, again[i] > 0
        assert m.sum() > 150 and (again[i][m] == mids[i] + 1).all()      # the box at scale 0.6 covers about 220 pixels
        iou = (a & m).sum() / (a | m).sum()
        iou_chain = ((chain > 0) & m).sum() / ((chain > 0) | m).sum()
        outside = int(((warped[i] != again[i]) & ~band(m)).sum())
        print(f"model {mids[i]} warp {WARPS[i % 4]}: IoU {iou:.4f}, {int((warped[i] != again[i]).sum())} differ, {outside} outside the band")
        assert iou == iou_chain and outside == 0
        if WARPS[i % 4][0] == 90.0:
            np.testing.assert_array_equal(warped[i], again[i])


# ---- 7. the loop closes ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loop_closes_through_the_augmentation(device, A):
    from pvnet_amd import ransac_voting_gpu as rvg
    from pvnet_amd import render as Rn
    from tests.test_gpu_render import CPU_WORST, loop_scene
    s = loop_scene()
    H, W, K = s["H"], s["W"], cu(s["K"], device)
    table = Rn.MeshTable(s["models"], device=device)
    mid = torch.tensor([0, 1], dtype=torch.int32, device=device)
    label, _, kp_true = Rn.render_ground_truth(table, s["p3"], cu(s["poses"], device), mid, K, H, W)
    gen = torch.Generator(device=device).manual_seed(3)
    image = torch.randint(0, 256, (4, H, W, 3), dtype=torch.uint8, device=device, generator=gen)
    state = torch.tensor([2024, 0], dtype=torch.int64, device=device)
    img, lab, vertex, kp = A.augment_ground_truth(image, label, kp_true, 2, state, layout="bhwk2", scale=(0.9, 1.2),
                                                  dtype=torch.float16)
    assert tuple(img.shape) == (4, 3, H, W) and img.dtype == torch.float16 and tuple(lab.shape) == (4, H, W)
    assert tuple(vertex.shape) == (4, H, W, 18, 2) and tuple(kp.shape) == (4, 2, 9, 2) and kp.dtype == torch.float64
    assert bool(torch.isfinite(img).all())
    # the pieces are the documented ones
    prm = A.random_params(label, 2, (H, W), state, scale=(0.9, 1.2))
    assert torch.equal(kp, A.transform_keypoints(kp_true, prm.fwd))
    assert torch.equal(lab, A.apply(image, label, prm)[1])
    assert torch.equal(vertex, Rn.vertex_field(lab, kp, 2))
    area = torch.stack([(lab == c + 1).sum((1, 2)) for c in range(2)], 1).cpu().numpy()
    assert area.min() > 500
    got = rvg.ransac_voting_layer_v3_multi(lab, vertex, 2, 512, _seed=20240)
    kp_err = float((got.to(torch.float64) - kp).norm(dim=-1).max())
    print(f"loop through the augmentation: keypoints {kp_err:.3e} px (bound {4 * CPU_WORST['keypoint_px']:.3e})")
    assert kp_err <= 4 * CPU_WORST["keypoint_px"]


@pytest.mark.gpu
def test_a_training_step_on_an_augmented_batch(device, A):
    from pvnet_amd import render as Rn
    from pvnet_amd.net_utils import pvnet_loss
    from pvnet_amd.network import PVNet
    from tests.test_gpu_render import loop_scene
    s = loop_scene()
    K = cu(s["K"], device)
    table = Rn.MeshTable(s["models"], device=device)
    mid = torch.tensor([0, 1], dtype=torch.int32, device=device)
    label, _, kp_true = Rn.render_ground_truth(table, s["p3"], cu(s["poses"][:2], device), mid, K, s["H"], s["W"])
    image = torch.randint(0, 256, (2, s["H"], s["W"], 3), dtype=torch.uint8, device=device)
    state = torch.tensor([7, 0], dtype=torch.int64, device=device)
    img, lab, vertex, kp = A.augment_ground_truth(image, label, kp_true, 2, state, out_size=(64, 96), scale=(0.2, 0.3),
                                                  margin=0.4)
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


# ---- 8. the Python layer's errors ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_errors(device, A):
    b, H, W = 2, 6, 8
    img = torch.zeros(b, H, W, 3, dtype=torch.uint8, device=device)
    lab = torch.zeros(b, H, W, dtype=torch.uint8, device=device)
    state = torch.zeros(2, dtype=torch.int64, device=device)
    prm = A.random_params(lab, 1, (H, W), state)
    kp = torch.zeros(b, 1, 9, 2, dtype=torch.float64, device=device)
    A.apply(img, lab, prm)                                                  # the baseline is accepted
    with pytest.raises(RuntimeError, match="device"):
        A.apply(img.cpu(), lab.cpu(), A.AugmentParams(*(t.cpu() for t in prm)))
    with pytest.raises(RuntimeError, match="image's device"):
        A.apply(img, lab.cpu(), prm)
    with pytest.raises(RuntimeError, match="image's device"):
        A.apply(img, lab, A.AugmentParams(prm.fwd, prm.inv.cpu(), prm.color))
    with pytest.raises(RuntimeError, match="image's device"):
        A.apply(img, lab, prm, background=torch.zeros(1, H, W, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="image's device"):
        A.apply(img, lab, prm, out=(torch.zeros(b, 3, H, W), torch.zeros(b, H, W, dtype=torch.uint8)))
    with pytest.raises(RuntimeError, match="label's device"):
        A.random_params(lab, 1, (H, W), state.cpu())
    with pytest.raises(RuntimeError, match="same device"):
        A.transform_keypoints(kp.cpu(), prm.fwd)
    with pytest.raises(RuntimeError, match="device"):
        A.augment_ground_truth(img, lab, kp.cpu(), 1, state)
    with pytest.raises(RuntimeError, match="image"):
        A.apply(img[:1], lab, prm)
    with pytest.raises(RuntimeError, match="image"):
        A.apply(img.int(), lab, prm)
    with pytest.raises(RuntimeError, match="label"):
        A.apply(img, lab.float(), prm)
    with pytest.raises(RuntimeError, match="params"):
        A.apply(img, lab, A.AugmentParams(prm.fwd, prm.inv, prm.color.double()))
    with pytest.raises(RuntimeError, match="dtype"):
        A.apply(img, lab, prm, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="out must"):
        A.apply(img, lab, prm, out=(torch.zeros(b, 3, H, W, device=device, dtype=torch.float16),
                                    torch.zeros(b, H, W, dtype=torch.uint8, device=device)))
    with pytest.raises(RuntimeError, match="out must"):
        A.apply(img, lab, prm, out=torch.zeros(b, 3, H, W, device=device))
    with pytest.raises(RuntimeError, match="out_size"):
        A.apply(img, lab, prm, out_size=(H, 0))
    with pytest.raises(RuntimeError, match="class_num"):
        A.random_params(lab, 2000, (H, W), state)
    # an empty batch is not an error
    e_img, e_lab = A.apply(img[:0], lab[:0], A.AugmentParams(prm.fwd[:0], prm.inv[:0], prm.color[:0]))
    assert tuple(e_img.shape) == (0, 3, H, W) and tuple(e_lab.shape) == (0, H, W)
    assert tuple(A.label_stats(lab[:0], 1).shape) == (0, 8)
