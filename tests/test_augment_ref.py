"""tests/augment_ref.py (the numpy restatement of include/pvaugment.h) against independent yardsticks:
torch's grid_sample on the CPU in f64, the standard library's colorsys, and the generator written a
second time in Python integers."""
import colorsys

import numpy as np
import torch
import torch.nn.functional as F

from tests import augment_ref as R

H, W, HO, WO = 37, 53, 29, 41
# every source coordinate of these stays at least 1e-6 away from a half-integer (asserted below):
# torch computes through a normalised grid, so its nearest differs at exact ties
MATS = np.array([[[0.83171937, -0.41290713, 9.30713391], [0.39110291, 0.88230517, -4.71130873]],     # partly outside
                 [[1.27130619, 0.19310337, -3.14170459], [-0.22170893, 1.18730271, 5.64190147]],
                 [[-0.61310773, 0.79190231, 30.21830919], [-0.77230417, -0.63110159, 40.11770633]],  # beyond 90 degrees
                 [[0.41110357, 0.01370911, 40.11930279], [0.01710533, 0.39170197, 2.71310861]]])     # mostly outside


def scene(seed=0):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    label = rng.integers(0, 4, (H, W)).astype(np.uint8)
    return image, label


def torch_sample(src, M, mode):
    """src f64 [C][H][W] -> [C][HO][WO] through F.grid_sample with align_corners=True and zero padding."""
    sx, sy = R.source_coords(M, HO, WO)
    grid = np.stack([2.0 * sx / (W - 1) - 1.0, 2.0 * sy / (H - 1) - 1.0], -1)
    out = F.grid_sample(torch.from_numpy(src)[None], torch.from_numpy(grid)[None], mode=mode, padding_mode="zeros",
                        align_corners=True)
    return out[0].numpy()


def test_geometry_against_grid_sample():
    image, label = scene()
    for M in MATS:
        sx, sy = R.source_coords(M, HO, WO)
        for s in (sx, sy):
            assert np.abs((s - np.floor(s)) - 0.5).min() >= 1e-6
        ref = torch_sample(image.astype(np.float64).transpose(2, 0, 1), M, "bilinear").transpose(1, 2, 0)
        # the restatement with its weights left in f64 is what grid_sample computes ...
        assert np.abs(R.warp_image(image, M, HO, WO, weights=np.float64) - ref).max() <= 1e-10
        # ... and the header's f32 weights move a value by at most 255 * 2^-24 each
        assert np.abs(R.warp_image(image, M, HO, WO) - ref).max() <= 2 * 255 * 2.0 ** -24 + 1e-10
        lab = R.warp_label(label, M, HO, WO)
        ref_l = torch_sample(label.astype(np.float64)[None], M, "nearest")[0]
        np.testing.assert_array_equal(lab, ref_l.astype(np.uint8))
        assert (lab > 0).any() and (lab == 0).any()


def test_fill_and_non_finite_matrices():
    image, label = scene(1)
    fill = (12.0, 200.0, 77.0)
    for bad in (np.nan, np.inf, -np.inf, 1e300):
        for pos in ((0, 2), (1, 2), None):            # a translation, or every entry
            M = MATS[0].copy()
            if pos is None:
                M[:] = bad
            else:
                M[pos] = bad
            c = R.warp_image(image, M, HO, WO, fill)
            lab = R.warp_label(label, M, HO, WO)
            assert (lab == 0).all() and (c == np.array(fill)).all()
    M = MATS[0].copy()
    M[:, 2] = (1e6, -1e6)
    assert (R.warp_label(label, M, HO, WO) == 0).all() and (R.warp_image(image, M, HO, WO, fill) == np.array(fill)).all()
    # a tap outside takes the fill: the identity shifted by half a pixel mixes the border with it
    M = np.array([[1.0, 0.0, -0.5], [0.0, 1.0, 0.0]])
    c = R.warp_image(image, M, H, W, fill)
    np.testing.assert_allclose(c[:, 0], 0.5 * (np.array(fill) + image[:, 0]), atol=1e-12)


def test_hue_against_colorsys():
    rng = np.random.default_rng(2)
    cols = np.concatenate([rng.random((4000, 3)), np.repeat(rng.random((50, 1)), 3, 1),
                           np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1],
                                     [0.5, 0.5, 0.2], [0.2, 0.5, 0.5], [0.5, 0.2, 0.5]], np.float64)])
    h, s, v = R.rgb_to_hsv(cols)
    ref = np.array([colorsys.rgb_to_hsv(*c) for c in cols])
    assert np.abs(np.stack([h, s, v], 1) - ref).max() <= 1e-12
    back = R.hsv_to_rgb(h, s, v)
    ref_back = np.array([colorsys.hsv_to_rgb(*x) for x in ref])
    assert np.abs(back - ref_back).max() <= 1e-12 and np.abs(back - cols).max() <= 1e-12
    for eta in (-0.5, -0.05, 0.0, 0.03, 0.5):
        got = R.hue_shift(cols, eta)
        want = np.array([colorsys.hsv_to_rgb((x[0] + eta) % 1.0, x[1], x[2]) for x in ref])
        assert np.abs(got - want).max() <= 1e-12, eta
    # sector 6 (a hue that rounds up to 1) is sector 0
    np.testing.assert_allclose(R.hsv_to_rgb(np.array([1.0]), np.array([0.5]), np.array([0.8])),
                               [colorsys.hsv_to_rgb(0.0, 0.5, 0.8)], atol=1e-15)


def test_draws_against_python_integers():
    seed, first = 0x1234567890ABCDEF, 2 ** 63 + 5          # the sample index wraps like any uint64
    u = R.draws(seed, first, 512)
    assert u.shape == (512, 8) and u.size == 4096
    for n in (0, 1, 17, 511):
        for k in range(8):
            assert u[n, k] == R.draw_int(seed, (first + n) % 2 ** 64, k)
    assert (u >= 0.0).all() and (u < 1.0).all()
    assert abs(u.mean() - 0.5) <= 0.03                    # > 6 sigma of 0.289 / 64
    assert len(np.unique(u)) == u.size
    # another seed, another first index: other draws; the same state: the same bits
    assert not np.isin(R.draws(seed + 1, first, 512), u).any()
    np.testing.assert_array_equal(R.draws(seed, first + 512, 4), R.draws(seed, first, 516)[512:])
    np.testing.assert_array_equal(R.draws(seed, first, 512), u)


def test_maps_invert_and_centroid_lands_on_target():
    rng = np.random.default_rng(3)
    label = np.zeros((6, H, W), np.uint8)
    for i in range(5):                                   # image 5 has no foreground
        x0, y0 = rng.integers(0, W - 8), rng.integers(0, H - 8)
        label[i, y0:y0 + rng.integers(1, 8), x0:x0 + rng.integers(1, 8)] = rng.integers(1, 3)
    label[0, 0, 0] = 3                                   # above ncls: not foreground
    stats = R.label_stats(label, 2)
    assert stats[5].tolist() == [0, 0, 0, W, H, -1, -1, 0] and stats[0, 0] == (label[0] > 0).sum() - 1
    fwd, inv, color, info = R.params(stats, 7, 100, H, W, HO, WO, rot_deg=(-180.0, 180.0), scale=(0.5, 2.0), margin=0.1)
    eye = np.eye(3)
    for i in range(6):
        A, B = np.vstack([fwd[i], [0, 0, 1]]), np.vstack([inv[i], [0, 0, 1]])
        assert np.abs(A @ B - eye).max() <= 1e-12
        c = info["c"][i]
        np.testing.assert_allclose(fwd[i] @ [c[0], c[1], 1.0], info["t"][i], atol=1e-11)
        t = info["t"][i]
        assert 0.1 * (WO - 1) <= t[0] <= 0.9 * (WO - 1) and 0.1 * (HO - 1) <= t[1] <= 0.9 * (HO - 1)
        s, th = info["s"][i], info["theta"][i]
        np.testing.assert_allclose(fwd[i][:, :2], s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), atol=1e-15)
        assert 0.5 <= s <= 2.0 and -np.pi <= th <= np.pi
    np.testing.assert_allclose(info["c"][5], [(W - 1) / 2, (H - 1) / 2])
    ys, xs = np.nonzero((label[1] >= 1) & (label[1] <= 2))
    np.testing.assert_allclose(info["c"][1], [xs.mean(), ys.mean()], atol=1e-12)
    assert color.dtype == np.float32 and color.shape == (6, 4)
    assert (np.abs(color[:, :2] - 1) <= 0.1 + 1e-7).all() and (np.abs(color[:, 2] - 1) <= 0.05 + 1e-7).all() \
        and (np.abs(color[:, 3]) <= 0.05).all()


def test_photometric_chain_properties():
    rng = np.random.default_rng(4)
    c = rng.random((HO, WO, 3))
    one = np.array([1, 1, 1, 0], np.float32)
    np.testing.assert_allclose(R.photometric(c, one, R.ALL), c, atol=1e-12)       # the neutral jitter changes nothing
    out = R.photometric(c, np.array([1.3, 1.0, 1.0, 0.0], np.float32), R.BRIGHTNESS)
    np.testing.assert_array_equal(out, np.minimum(float(np.float32(1.3)) * c, 1.0))
    out = R.photometric(c, np.array([1.0, 0.0, 1.0, 0.0], np.float32), R.CONTRAST)  # no contrast: the grey mean
    np.testing.assert_allclose(out, R.grey(c).mean(), atol=1e-15)
    out = R.photometric(c, np.array([1.0, 1.0, 0.0, 0.0], np.float32), R.SATURATION)  # no saturation: the grey
    np.testing.assert_allclose(out, np.repeat(R.grey(c)[..., None], 3, -1), atol=1e-15)
    # a flag that is off skips its step
    np.testing.assert_array_equal(R.photometric(c, np.array([1.3, 0.5, 0.5, 0.2], np.float32), 0), c)
