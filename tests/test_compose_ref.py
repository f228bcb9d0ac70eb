"""tests/compose_ref.py (include/pvcompose.h in numpy) against yardsticks that share none of its code:
a per-pixel painter's loop, the generator in pure Python integers, and an f64 separable convolution."""
import numpy as np

from tests import augment_ref as AR
from tests import compose_ref as C

EPS = 2.0 ** -24        # the relative error of one f32 rounding
I32 = np.iinfo(np.int32)


def naive_compose(bank_image, bank_label, pick, shift, ncls, Ho, Wo, background, fill, erase):
    """The header's sentences, pixel by pixel: highest belonging slot, else background or fill, then erasers."""
    N, H, W = bank_label.shape
    b, S = pick.shape[:2]
    image = np.zeros((b, Ho, Wo, 3), np.uint8)
    label = np.zeros((b, Ho, Wo), bank_label.dtype)
    inst = np.zeros((b, Ho, Wo), bank_label.dtype)
    visible = np.zeros((b, S), np.int32)
    for f in range(b):
        for y in range(Ho):
            for x in range(Wo):
                col = background[f if background.shape[0] == b else 0, y, x] if background is not None else fill
                lab = ins = 0
                for s in reversed(range(S)):
                    src, sl, cls, x0, y0, x1, y1, _ = (int(v) for v in pick[f, s])
                    if not (0 <= src < N and 1 <= cls <= ncls):
                        continue
                    sx, sy = x - int(shift[f, s, 0]), y - int(shift[f, s, 1])
                    if not (x0 <= sx <= x1 and y0 <= sy <= y1 and 0 <= sx < W and 0 <= sy < H):
                        continue
                    if int(bank_label[src, sy, sx]) == sl:
                        col, lab, ins = bank_image[src, sy, sx], cls, s + 1
                        break
                if erase is not None and any(e[0] <= x <= e[2] and e[1] <= y <= e[3] for e in erase[f].tolist()):
                    col, lab, ins = fill, 0, 0
                image[f, y, x], label[f, y, x], inst[f, y, x] = col, lab, ins
                if ins:
                    visible[f, ins - 1] += 1
    return image, label, inst, visible


def test_compose_against_a_painters_loop():
    rng = np.random.default_rng(5)
    hostile = [I32.min, I32.max, -1, 0, 1]
    for trial in range(40):
        N, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 10)), int(rng.integers(1, 12))
        Ho, Wo = int(rng.integers(1, 10)), int(rng.integers(1, 12))
        b, S, E, ncls = 2, int(rng.integers(1, 6)), int(rng.integers(0, 4)), 3
        bank_image = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        bank_label = rng.integers(0, 3, (N, H, W)).astype([np.uint8, np.int32, np.int64][trial % 3])
        pick = np.zeros((b, S, 8), np.int32)
        pick[..., 0] = rng.integers(-1, N + 1, (b, S))
        pick[..., 1] = rng.integers(0, 3, (b, S))
        pick[..., 2] = rng.integers(0, ncls + 2, (b, S))
        pick[..., 3:5] = rng.integers(-2, 4, (b, S, 2))
        pick[..., 5:7] = rng.integers(-1, 13, (b, S, 2))
        shift = rng.integers(-6, 7, (b, S, 2)).astype(np.int32)
        erase = rng.integers(-2, 12, (b, E, 4)).astype(np.int32) if E else None
        if trial % 4 == 0:
            shift[0, 0] = (hostile[trial % 5], hostile[(trial + 1) % 5])
            pick[1, 0, 3:7] = (I32.min, I32.min, I32.max, I32.max)
        bg = [None, rng.integers(0, 256, (1, Ho, Wo, 3), dtype=np.uint8), rng.integers(0, 256, (b, Ho, Wo, 3), dtype=np.uint8)][trial % 3]
        fill = np.array([9, 200, 77], np.uint8)
        got = C.compose(bank_image, bank_label, pick, shift, ncls, Ho, Wo, bg, fill, erase)
        want = naive_compose(bank_image, bank_label, pick, shift, ncls, Ho, Wo, bg, fill, erase)
        for g, w, name in zip(got, want, ("image", "label", "instance", "visible")):
            np.testing.assert_array_equal(g, w, err_msg=f"trial {trial}: {name}")
            assert g.dtype == w.dtype


def test_draws_are_the_augmentation_generators():
    seed, first = 0x0123456789ABCDEF, 2 ** 64 - 2           # the sample index wraps
    for k in (64, 71, 192, 256, 258):
        for i in range(4):
            n = (first + i) % 2 ** 64
            assert float(C.u(seed, n, k)) == AR.draw_int(seed, n, k), (k, i)
    # vectorised over k, and disjoint from the augmentation's draw numbers
    np.testing.assert_array_equal(C.u(seed, 5, np.arange(8)), AR.draws(seed, 5, 1)[0])
    assert C.DRAW0 >= AR.DRAWS and C.DRAW0 + 8 * C.MAX_SLOTS <= 192 and 192 + 8 * C.MAX_ERASE <= 256


def test_params_rules():
    N, H, W, Ho, Wo, ncls, S, E = 3, 20, 30, 40, 50, 2, 4, 5
    pick = np.zeros((6, S, 8), np.int32)
    pick[:, :, 0] = [0, 1, 3, 2]                            # slot 2: src = N, dead
    pick[:, :, 1] = 1
    pick[:, :, 2] = [1, 2, 1, 3]                            # slot 3: class 3 > ncls, dead
    pick[:, 0, 3:7] = (4, 3, 17, 12)
    pick[:, 1, 3:7] = (-5, -5, 100, 100)                    # clipped to the frame
    pick[:, 2, 3:7] = (0, 0, 5, 5)
    pick[:, 3, 3:7] = (0, 0, 5, 5)
    pick[5, 0, 3:7] = (8, 3, 7, 12)                         # inverted: no shift, its eraser empty
    seed, first = 99, 7
    shift, erase, ksel, amp = C.params(pick, seed, first, N, H, W, Ho, Wo, ncls, E, margin=0.2, erase_frac=(0.3, 0.9),
                                       p_blur=0.5, noise=(1.0, 6.0))
    assert (shift[:, 2:] == 0).all() and (shift[5, 0] == 0).all() and (erase[5, [0, 4]] == (0, 0, -1, -1)).all()
    assert (erase[:, [2, 3]] == (0, 0, -1, -1)).all()
    for f in range(5):
        # slot 0 in pure Python
        u0, u1 = AR.draw_int(seed, first + f, 64), AR.draw_int(seed, first + f, 65)
        assert shift[f, 0, 0] == round((0.2 + u0 * (1 - 2 * 0.2)) * (Wo - 1) - (4 + 17) / 2)
        assert shift[f, 0, 1] == round((0.2 + u1 * (1 - 2 * 0.2)) * (Ho - 1) - (3 + 12) / 2)
        for e in (0, 1, 4):
            s = e % S
            x0, y0, x1, y1 = C.clipped_box(pick[f, s], H, W)
            dx, dy = shift[f, s]
            ex0, ey0, ex1, ey1 = erase[f, e]
            assert x0 + dx <= ex0 <= ex1 <= x1 + dx and y0 + dy <= ey0 <= ey1 <= y1 + dy
            assert 0.3 * (x1 - x0 + 1) - 0.5 <= ex1 - ex0 + 1 <= 0.9 * (x1 - x0 + 1) + 0.5
        assert ksel[f] == (1 + min(3, int(4 * AR.draw_int(seed, first + f, 257))) if AR.draw_int(seed, first + f, 256) < 0.5 else 0)
        assert amp[f] == np.float32(1.0 + AR.draw_int(seed, first + f, 258) * 5.0)
    many = C.params(np.repeat(pick[:1], 64, 0), seed, 0, N, H, W, Ho, Wo, ncls, 0)
    assert set(many[2].tolist()) == {0, 1, 2, 3, 4} and 20 <= np.count_nonzero(many[2]) <= 44


def test_noise_field_in_python_integers():
    M = (1 << 64) - 1
    g = 0x9E3779B97F4A7C15

    def m(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    seed, n, H, W = 0xFEDCBA9876543210, 2 ** 64 - 1, 5, 7
    got = C.noise_field(seed, n, H, W)
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    key = m((m((seed + g) & M) + (n + 1) * g) & M)
    for y in range(H):
        for x in range(W):
            for ch in range(3):
                z = m((key + ((1 << 40) + 3 * (y * W + x) + ch + 1) * g) & M)
                s = sum((z >> sh) & 0xFFFF for sh in (0, 16, 32, 48))
                assert float(got[y, x, ch]) == (s - 131070) / 65536.0          # exact in f32: |s - 131070| < 2^24
    big = C.noise_field(3, 0, 64, 64)
    assert abs(float(big.mean())) < 0.02 and abs(float(big.std()) - np.sqrt(4 / 12)) < 0.01 and np.abs(big).max() < 2.0


def test_kernels():
    w = C.kernels()
    assert w.dtype == np.float32 and w[0, 0] == 1.0
    for j in range(5):
        assert (w[j, j + 1:] == 0).all() and (np.diff(w[j, :j + 1]) < 0).all()
        assert abs(float(w[j, 0]) + 2.0 * float(w[j, 1:].astype(np.float64).sum()) - 1.0) < 4 * EPS
    # cv2.getGaussianKernel(3, 0)'s sigma is 0.8: the centre weight of exp(-t^2 / 1.28) normalised
    assert abs(w[1, 0] - 1.0 / (1.0 + 2.0 * np.exp(-1.0 / 1.28))) < EPS
    from pvnet_amd.compose import blur_kernels
    np.testing.assert_array_equal(blur_kernels().numpy(), w)


def test_identity_and_constant_images():
    rng = np.random.default_rng(1)
    image = rng.integers(0, 256, (3, 6, 9, 3), dtype=np.uint8)
    zero = np.zeros(3, np.float32)
    np.testing.assert_array_equal(C.finish(image, np.zeros(3, np.int32), zero, 5, 0), image)
    np.testing.assert_array_equal(C.finish(image, np.array([5, -1, 2 ** 31 - 1], np.int32), zero, 5, 0), image)   # any other ksel is 0
    for v in (0, 1, 127, 254, 255):
        const = np.full((5, 7, 11, 3), v, np.uint8)
        np.testing.assert_array_equal(C.finish(const, np.arange(5, dtype=np.int32), np.zeros(5, np.float32), 5, 0), const)
    # noise alone: the image plus the rounded field, clamped
    out = C.finish(image[:1], np.zeros(1, np.int32), np.array([40.0], np.float32), 5, 3)
    t = C.noise_field(5, 3, 6, 9).astype(np.float64)
    np.testing.assert_array_equal(out[0], np.rint(np.clip(image[0] + 40.0 * t, 0, 255)).astype(np.uint8))
    assert (out != image[:1]).mean() > 0.9


def blur_bound(j):
    """Written down before the first run.  One pass makes at most 3 j + 1 roundings (the centre product; per
    tap pair a sum, a product, an add), each of a value of at most 255 (1 + 2^-20) (the partial sums of
    non-negative weights that add up to 1 within 4 EPS): (3 j + 1) * 255 * EPS * (1 + 2^-20) a pass.  The
    second pass carries the first's error through weights that sum to at most 1 + 4 EPS and adds its own.
    The factor 1.001 covers both parentheses and the products of errors."""
    return 2 * (3 * j + 1) * 255.0 * EPS * 1.001 if j else 0.0


def test_blur_against_an_f64_convolution():
    rng = np.random.default_rng(2)
    w = C.kernels()
    for H, W in ((7, 5), (3, 4), (12, 13), (1, 6), (6, 1), (1, 1)):
        image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        image[0, 0] = 255
        for j in range(5):
            full = np.concatenate([w[j, j:0:-1], w[j, :j + 1]]).astype(np.float64)          # the 2 j + 1 taps
            v = image.astype(np.float64)
            for axis, n in ((1, W), (0, H)):
                if n == 1:
                    v = v * full.sum()                  # reflect-101 of one pixel is that pixel
                    continue
                pad = [(0, 0)] * 3
                pad[axis] = (j, j)
                p = np.pad(v, pad, mode="reflect")
                v = sum(full[k] * np.take(p, np.arange(k, k + n), axis) for k in range(2 * j + 1))
            got = C.blurred(image, j, w)
            assert got.dtype == np.float32
            err = float(np.abs(got.astype(np.float64) - v).max())
            if j:
                print(f"blur {H}x{W} k={2 * j + 1}: max error {err:.3e}, {err / blur_bound(j):.3f} of the bound {blur_bound(j):.3e}")
            assert err <= blur_bound(j)
