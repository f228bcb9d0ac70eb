"""The voting front half -- k_fg_count / k_label_count, k_compact with its fused compact_hyp,
k_hyp_gen and the vote kernel's hypothesis prologue -- beyond 480x640 and on its seeded RNG path.

  * test_shapes_match_oracle: frames from one partial chunk up to the wide compaction with
    k_hyp_gen (SHAPES), injected pixel pairs, against the CPU oracle.
  * test_seeded_equals_injected (+ _other_entries): a call that draws its own pairs and keep
    decisions (``_seed`` only) equals, bit for bit, the call that is handed tests/front_ref.py's
    restatement of those draws -- so the three sites that draw a pair and the three that decide
    a keep agree with each other and with the documented layout.
  * test_vote_launch_split: a batch that front_half cuts into two vote launches.

Inputs are built here (``inputs``): sparse foreground that holds pixel 0, the last pixel, one
whole 256-pixel chunk, a run across a chunk boundary and, in large frames, two blobs more than
300 empty chunks apart; unit directions towards per-keypoint targets with 0.02 rad of noise, so
nearly every pixel is an inlier of the winner and one wrong record moves the refine sums by ~1/tn.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from pvnet_amd import _lib
from tests import front_ref as R

pytestmark = pytest.mark.gpu

KP_TOL = 1e-2          # the suite's keypoint tolerance (tests/test_gpu_parity.py)
CHUNK = 256
F32 = np.float32

# H, W, vn: each the smallest frame that reaches its path
SHAPES = [
    (10, 10, 3),       # one partial chunk: block 0 is also block nblk - 1
    (16, 16, 9),       # one full chunk
    (37, 51, 9),       # partial tail
    (3, 2000, 5),      # rows far longer than a chunk
    (2000, 3, 9),      # rows far shorter than a chunk
    (512, 768, 9),     # 1536 chunks: the fused hypotheses' upper bound, 6 chunks per thread
    (607, 648, 9),     # 1537 chunks, tail of 120: the first frame on k_hyp_gen
    (1025, 1031, 9),   # 4129 chunks: one image on the wide compaction + k_hyp_gen
]
LARGE = {(512, 768), (607, 648), (1025, 1031)}


@pytest.fixture(scope="module")
def rvg():
    from pvnet_amd import ransac_voting_gpu
    return ransac_voting_gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def cu(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dev) if dtype is None else t.to(device=dev, dtype=dtype)


# ---------------------------------------------------------------- inputs
def make_mask(H, W, rng, shift, dense):
    """bool [H, W].  ``shift`` moves every feature (masks of a batch differ); ``dense`` puts
    5000 or more foreground pixels where the frame has room (the downsampled runs)."""
    P = H * W
    nblk = -(-P // CHUNK)
    m = np.zeros(P, bool)
    if P < 2 * CHUNK:
        if P % CHUNK == 0:
            m[:] = True                                       # the whole chunk
        else:
            m |= rng.random(P) < 0.4
    else:
        cfull = 1 + shift
        m[cfull * CHUNK:(cfull + 1) * CHUNK] = True           # one whole aligned chunk
        for k in range(cfull + 2, nblk):                      # a run across a chunk boundary, mid-row where rows are long enough
            col = (k * CHUNK) % W
            if W < 64 or 20 <= col <= W - 30:
                m[k * CHUNK - 20:k * CHUNK + 30] = True
                break
        else:
            raise AssertionError("no chunk boundary mid-row")
        if P < 100_000:
            m |= rng.random(P) < (0.8 if dense else 0.1 + 0.02 * shift)
        else:
            m2 = m.reshape(H, W)
            hh, ww, dens = (60, 80, 1.0) if dense else (40, 60, 0.5)
            r0, c0 = 8 + 3 * shift, W // 5 + 7 * shift
            m2[r0:r0 + hh, c0:c0 + ww] |= rng.random((hh, ww)) < dens
            r1, c1 = H - hh - 10 - 2 * shift, W // 2 - 5 * shift
            m2[r1:r1 + hh, c1:c1 + ww] |= rng.random((hh, ww)) < dens
            occ = np.nonzero(np.add.reduceat(m, np.arange(0, P, CHUNK)))[0]
            assert np.diff(occ).max() > 300, "two blobs at least 300 empty chunks apart"
    m[0] = m[P - 1] = True
    return m.reshape(H, W)


def make_targets(H, W, vn, rng):
    """Keypoint targets off every pixel centre, spread so that the least squares stays well
    conditioned in strip-shaped frames too."""
    S = max(H, W)
    x = W / 2 + rng.choice([-1.0, 1.0], vn) * rng.uniform(0.15, 0.4, vn) * S + 0.37
    y = H / 2 + rng.choice([-1.0, 1.0], vn) * rng.uniform(0.15, 0.4, vn) * S + 0.41
    return np.stack([x, y], 1).astype(F32)


def fill_field(ver, fg, kp, rng, bg_angle):
    """ver [H, W, vn, 2] in place: a constant off the foreground, unit directions towards kp on it."""
    ver[:] = (np.cos(bg_angle), np.sin(bg_angle))
    rows, cols = np.nonzero(fg)
    d = kp[None].astype(np.float64) - np.stack([cols, rows], 1)[:, None]
    ang = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0, 0.02, d.shape[:2])
    ver[rows, cols] = np.stack([np.cos(ang), np.sin(ang)], -1)


@functools.lru_cache(maxsize=4)
def inputs(b, H, W, vn, dense=(), empty=-1):
    """mask int64 [b,H,W], vertex f32 [b,H,W,vn,2], targets kp [b,vn,2]; image ``empty`` has no
    foreground, images listed in ``dense`` carry 5000 or more pixels where the frame has room."""
    rng = np.random.default_rng([H, W, b, vn])
    mask = np.zeros((b, H, W), np.int64)
    ver = np.empty((b, H, W, vn, 2), F32)
    kp = np.zeros((b, vn, 2), F32)
    for i in range(b):
        if i != empty:
            mask[i] = make_mask(H, W, rng, i, i in dense)
        kp[i] = make_targets(H, W, vn, rng)
        fill_field(ver[i], mask[i], kp[i], rng, 1.0 + i)
    return mask, ver, kp


def network_layout(mask, ver):
    """f16 seg_pred [b,2,H,W] and vertex_pred [b,2vn,H,W] of the same frame, and the f16-rounded
    field (f32, [b,H,W,vn,2]) the oracle votes."""
    b, H, W, vn, _ = ver.shape
    fg = mask != 0
    seg = np.stack([np.where(fg, -2.0, 1.0), np.where(fg, 3.0, -1.0)], 1).astype(np.float16)
    v16 = ver.astype(np.float16)
    nchw = np.ascontiguousarray(v16.reshape(b, H, W, 2 * vn).transpose(0, 3, 1, 2))
    return seg, nchw, v16.astype(F32)


def cover_idxs(tn, nh, vn, rng):
    """int32 [nh, vn, 2]: every compacted index at least once per keypoint where 2 nh >= tn."""
    out = np.zeros((nh, vn, 2), np.int32)
    if tn <= 0:
        return out
    for v in range(vn):
        flat = rng.integers(0, tn, 2 * nh)
        if 2 * nh >= tn:
            flat[:tn] = np.arange(tn)
        out[:, v] = rng.permutation(flat).reshape(nh, 2)
    return out


def voted_tn(fg_counts, kept_counts, min_num, max_num):
    """The compacted count of each image: 0 below min_num, the kept count above max_num."""
    return [0 if f < min_num else (k if f > max_num else f) for f, k in zip(fg_counts, kept_counts)]


# ---------------------------------------------------------------- 1. shapes against the oracle
def shape_cases():
    for H, W, vn in SHAPES:
        for nh in (512, 128):
            for entry in ("v3", "net"):
                if (H, W) in LARGE and nh == 128 and entry == "net":
                    continue                                   # the three largest: nh = 128 with one entry only
                yield pytest.param(H, W, vn, nh, entry, id=f"{H}x{W}-nh{nh}-{entry}")


@functools.lru_cache(maxsize=2)
def shape_reference(H, W, vn, nh, half):
    """The oracle's run of a shape on the f32 field or on its f16 rounding."""
    b = 2 if H * W <= 37 * 51 else 1
    mask, ver, _ = inputs(b, H, W, vn, empty=(0 if (H, W) == (16, 16) else 1) if b == 2 else -1)
    fgn = [int((m != 0).sum()) for m in mask]
    min_num = 1 if any(0 < f < 100 for f in fgn) else 100
    rng = np.random.default_rng([H, W, nh])
    idxs = np.stack([cover_idxs(f if f >= min_num else 0, nh, vn, rng) for f in fgn])
    field = network_layout(mask, ver)[2] if half else ver
    dg = []
    ko = O.ransac_voting_layer_v3(mask, field, nh, min_num=min_num, idxs=list(idxs), diag=dg)
    return min_num, idxs, ko, dg


@pytest.mark.parametrize("H,W,vn,nh,entry", shape_cases())
def test_shapes_match_oracle(H, W, vn, nh, entry, device, rvg):
    """nh = 512 votes pre-generated hypotheses (compact_hyp up to 1536 chunks, k_hyp_gen above),
    nh = 128 the vote prologue's; "v3" takes an f32 [b,H,W,vn,2] field and an int64 mask, "net"
    f16 logits and an f16 NCHW field (the oracle votes the same rounded directions).  Frames up
    to 37x51 run as a batch of two different masks, one of them empty."""
    b = 2 if H * W <= 37 * 51 else 1
    mask, ver, _ = inputs(b, H, W, vn, empty=(0 if (H, W) == (16, 16) else 1) if b == 2 else -1)
    min_num, idxs, ko, dg = shape_reference(H, W, vn, nh, entry == "net")
    assert max(d["foreground"] for d in dg) <= 4500
    diag = {}
    if entry == "v3":
        kp = rvg.ransac_voting_layer_v3(cu(mask, device), cu(ver, device), nh, min_num=min_num, _idxs=idxs, _diag=diag)
    else:
        seg, nchw, _ = network_layout(mask, ver)
        kp = rvg.ransac_voting_layer_v3_from_network(cu(seg, device), cu(nchw, device), nh, min_num=min_num,
                                                     _idxs=idxs, _diag=diag)
    kp = kp.cpu().numpy()
    diag = {k: v.cpu().numpy() for k, v in diag.items()}
    assert any(not d.get("skipped") for d in dg)
    for i, d in enumerate(dg):
        if d.get("skipped"):
            assert int(diag["tn"][i]) == 0 and np.all(kp[i] == 0)
            continue
        assert int(diag["tn"][i]) == d["tn"] == d["foreground"]
        np.testing.assert_array_equal(bits(diag["hyp"][i]), bits(d["hyp"]), err_msg=f"image {i} hyp")
        np.testing.assert_array_equal(diag["counts"][i].T, d["counts"], err_msg=f"image {i} counts")
        np.testing.assert_array_equal(diag["win_idx"][i], d["win_idx"])
        np.testing.assert_allclose(diag["ata"][i].reshape(vn, 2, 2), d["ATA"], rtol=1e-6,
                                   atol=1e-7 * np.abs(d["ATA"]).max())
        np.testing.assert_allclose(diag["atb"][i].reshape(vn, 2), d["ATb"], rtol=1e-6,
                                   atol=1e-7 * np.abs(d["ATb"]).max())
    np.testing.assert_allclose(kp, ko, atol=KP_TOL, rtol=0)


# ---------------------------------------------------------------- 2. seeded == injected
SEEDS = [20240, 0xC0FFEE0123456789]          # below 2^32, and with high bits set
DIAG_KEYS = ("tn", "hyp", "counts", "win_idx", "win_ratio", "iters", "ata", "atb")


def lookback_self(on):
    L = _lib.load()
    L.pv_debug_lookback_self.argtypes = [ctypes.c_int32]
    L.pv_debug_lookback_self.restype = ctypes.c_int32
    assert L.pv_debug_lookback_self(on) == 0


def restated_draws(seed, fg, nh, vn, min_num, max_num, must_downsample=()):
    """(_idxs, _keep, tn) of a call with ``_seed=seed`` over the foreground masks fg [b,H,W], from
    tests/front_ref.py alone, with the conditions that make the run a fair one: images in
    ``must_downsample`` have fg > max_num, keep min_num or more pixels, and their kept count is
    within 5 sigma of max_num (sigma^2 = max_num (1 - max_num / fg))."""
    fgn = [int(f.sum()) for f in fg]
    keep = R.keep_mask(seed, fg, max_num)
    kept = [int((f & (k != 0)).sum()) for f, k in zip(fg, keep)]
    for i in must_downsample:
        assert fgn[i] > max_num, (i, fgn[i], max_num)
        assert kept[i] >= min_num, (i, kept[i], min_num)
        sigma = (max_num * (1 - max_num / fgn[i])) ** 0.5
        assert abs(kept[i] - max_num) <= 5 * sigma, (i, kept[i], max_num, sigma)
    tn = voted_tn(fgn, kept, min_num, max_num)
    return R.pairs(seed, tn, nh, vn), keep, tn


def assert_same_bits(a, b, voted, what):
    """Dicts of [images, ...] arrays equal bit for bit on the voted images (a skipped image's
    diagnostics are not written); its keypoints are zeros in both."""
    for k in a:
        for i, on in enumerate(voted):
            if on or k == "kp":
                np.testing.assert_array_equal(bits(a[k][i]), bits(b[k][i]), err_msg=f"{what}: {k}, image {i}")


SEEDED_CASES = [
    # id, b, H, W, nh
    ("fused-37x51", 2, 37, 51, 512),
    ("fused-480x640", 1, 480, 640, 512),
    ("prologue128-480x640", 1, 480, 640, 128),
    ("prologue40-37x51", 2, 37, 51, 40),
    ("prologue40-480x640", 1, 480, 640, 40),
    ("hypgen-607x648", 1, 607, 648, 512),
    ("wide-hypgen-1025x1031", 1, 1025, 1031, 512),
    ("wide-prologue40-1025x1031", 1, 1025, 1031, 40),
    ("wide-fused-4x480x640", 4, 480, 640, 512),
]


@pytest.mark.parametrize("seed", SEEDS, ids=["seed-lo", "seed-hi"])
@pytest.mark.parametrize("mode", ["full", "ds", "ds-self"])
@pytest.mark.parametrize("case", SEEDED_CASES, ids=[c[0] for c in SEEDED_CASES])
def test_seeded_equals_injected(case, mode, seed, device, rvg):
    """``_seed`` alone against ``_seed`` with front_ref's pairs and keep mask injected: tn,
    hypotheses, counts, winners, ratios, refine sums and keypoints equal bit for bit.  "full":
    max_num above the foreground; "ds": max_num a fifth of the dense images' foreground (5000 or
    more pixels each; 37x51 has room for ~1500), "ds-self" the same with every look-back count
    worked out by the waiter (pv_debug_lookback_self).  In the batch of four, image 1 is the
    sparse one: a lower keep ratio's neighbour in the same call."""
    _, b, H, W, nh = case
    vn = 9
    ds = mode != "full"
    dense = tuple(i for i in range(b) if not (b == 4 and i == 1)) if ds else ()
    mask, ver, _ = inputs(b, H, W, vn, dense=dense)
    fg = mask != 0
    fgn = [int(f.sum()) for f in fg]
    min_num = 100
    max_num = min(fgn[i] for i in dense) // 5 if ds else max(fgn) + 1
    if ds and H * W >= 100_000:
        assert min(fgn[i] for i in dense) >= 5000
    idxs, keep, tn = restated_draws(seed, fg, nh, vn, min_num, max_num, dense)
    md, vd = cu(mask, device), cu(ver, device)

    def call(**kw):
        diag = {}
        kp = rvg.ransac_voting_layer_v3(md, vd, nh, min_num=min_num, max_num=max_num, _seed=seed, _diag=diag, **kw)
        out = {k: diag[k].cpu().numpy() for k in DIAG_KEYS}
        out["kp"] = kp.cpu().numpy()
        return out
    if mode == "ds-self":
        lookback_self(1)
    try:
        seeded = call()
        injected = call(_idxs=idxs, _keep=keep)
    finally:
        if mode == "ds-self":
            lookback_self(0)
    assert seeded["tn"].tolist() == tn, "the device's tn against the restated keep mask's count"
    assert all(t > 0 for t in tn)
    assert_same_bits(seeded, injected, [t > 0 for t in tn], case[0])
    assert np.all(np.isfinite(seeded["kp"]))


# ---------------------------------------------------------------- 3. the other entries
def multi_inputs(b, H, W, vn, ncls):
    """label int64 [b,H,W] in 0..ncls (class 0 dense, the later classes drawn over it) and vertex
    f32 [b,H,W,ncls*vn,2]."""
    rng = np.random.default_rng([H, W, b, vn, ncls])
    label = np.zeros((b, H, W), np.int64)
    ver = np.empty((b, H, W, ncls * vn, 2), F32)
    for i in range(b):
        for c in range(ncls):
            label[i][make_mask(H, W, rng, c + i, c == 0)] = c + 1
        kp = make_targets(H, W, ncls * vn, rng)
        fill_field(ver[i], label[i] != 0, kp, rng, 1.0 + i)
    return label, ver


@pytest.mark.parametrize("seed", SEEDS, ids=["seed-lo", "seed-hi"])
@pytest.mark.parametrize("entry,H,W", [("v5", 37, 51), ("v5", 480, 640), ("evd", 37, 51), ("evd-ds", 480, 640),
                                       ("multi", 37, 51), ("multi", 480, 640)])
def test_seeded_equals_injected_other_entries(entry, H, W, seed, device, rvg):
    """The same equality through ransac_voting_layer_v5 (keypoints and confidences; its default
    max_num = 100 downsamples), estimate_voting_distribution_with_mean (mean and covariance) and
    ransac_voting_layer_v3_multi with three classes (keys on the virtual image bi * ncls + c; class
    0 alone is above max_num)."""
    if entry == "multi":
        b, vn, ncls, nh = 2, 4, 3, 512
        label, ver = multi_inputs(b, H, W, vn, ncls)
        fg = np.stack([label[i] == c + 1 for i in range(b) for c in range(ncls)])        # virtual images
        fgn = np.array([int(f.sum()) for f in fg]).reshape(b, ncls)
        assert np.all(fgn[:, 0] > fgn[:, 1:].max() + 50)
        min_num, max_num = 50, int(fgn[:, 0].min() + fgn[:, 1:].max()) // 2             # class 0 alone downsampled
        idxs, keep, tn = restated_draws(seed, fg, nh, vn, min_num, max_num, [i * ncls for i in range(b)])
        assert all(t > 0 for t in tn)
        ld, vd = cu(label, device), cu(ver, device)
        outs = []
        for kw in ({}, dict(_idxs=idxs.reshape(b, ncls, nh, vn, 2), _keep=keep.reshape(b, ncls, H, W))):
            diag = {}
            kp = rvg.ransac_voting_layer_v3_multi(ld, vd, ncls, nh, min_num=min_num, max_num=max_num, _seed=seed,
                                                  _diag=diag, **kw)
            out = {k: diag[k].cpu().numpy().reshape(b * ncls, *diag[k].shape[2:]) for k in DIAG_KEYS}
            out["kp"] = kp.cpu().numpy().reshape(b * ncls, vn, 2)
            outs.append(out)
        assert outs[0]["tn"].tolist() == tn
        assert_same_bits(outs[0], outs[1], [True] * (b * ncls), entry)
        return
    b, vn = 2, 9
    ds = entry != "evd"
    mask, ver, kp_true = inputs(b, H, W, vn, dense=(0, 1) if ds else ())
    fg = mask != 0
    fgn = [int(f.sum()) for f in fg]
    md, vd = cu(mask, device), cu(ver, device)
    if entry == "v5":
        nh, min_num, max_num = 128, 5, 100
        idxs, keep, tn = restated_draws(seed, fg, nh, vn, min_num, max_num, (0, 1))
        outs = [rvg.ransac_voting_layer_v5(md, vd, nh, _seed=seed, **kw)
                for kw in ({}, dict(_idxs=idxs, _keep=keep))]
    else:
        nh, min_num = 1024, 20                                   # 4 rounds of 256
        max_num = min(fgn) // 5 if ds else max(fgn) + 1
        idxs, keep, tn = restated_draws(seed, fg, nh, vn, min_num, max_num, (0, 1) if ds else ())
        mean = cu(kp_true, device)
        outs = [rvg.estimate_voting_distribution_with_mean(md, vd, mean, round_hyp_num=256, min_hyp_num=1024,
                                                           max_num=max_num, _seed=seed, **kw)
                for kw in ({}, dict(_idxs=idxs, _keep=keep))]
    assert all(t > 0 for t in tn)
    for x, y in zip(*outs):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.all(np.isfinite(x))
        np.testing.assert_array_equal(bits(x), bits(y))
    if entry == "v5":
        assert float(outs[0][1].min()) > 0                      # confidences of real votes, not zeros


# ---------------------------------------------------------------- 4. the vote launch split
@pytest.mark.parametrize("nh", [4096, 3968])
def test_vote_launch_split(nh, device, rvg):
    """front_half cuts a batch into several vote launches when b vn ceil(nh / 128) P reaches 2^31.
    Here b = 17, vn = 64, 256 x 256 (P = 65536): with nh = 4096 (32 groups, pre-generated
    hypotheses) a launch takes floor((2^31 - 1) / 2^27) = 15 images, so 15 + 2; with nh = 3968
    (31 groups, the vote prologue draws the pairs: the launch's offset into idxs and the RNG key's
    image base) it takes 16, so 16 + 1.  ~200 foreground pixels per image, every mask different.
    Seeded == injected bit for bit over the whole batch; images 0, 14, 15 and 16 each equal their
    own single call with their slice of the pairs, and the oracle's hypotheses and counts."""
    b, vn, H, W = 17, 64, 256, 256
    P = H * W
    groups = -(-nh // 128)
    per_launch = (2 ** 31 - 1) // (vn * groups * P)
    assert b > per_launch
    seed = SEEDS[1]
    rng = np.random.default_rng(nh)
    mask = np.zeros((b, H, W), np.int64)
    ver = torch.empty((b, H, W, vn, 2), dtype=torch.float32, device=device)
    pix = []
    for i in range(b):
        m = mask[i].reshape(-1)
        m[1 + rng.choice(P - 2, 190 + i, replace=False)] = 1
        m[0 if i % 2 else P - 1] = 1                          # 191 + i pixels
        rows, cols = np.nonzero(mask[i])
        kp = make_targets(H, W, vn, rng)
        d = kp[None].astype(np.float64) - np.stack([cols, rows], 1)[:, None]
        ang = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0, 0.02, d.shape[:2])
        direct = np.stack([np.cos(ang), np.sin(ang)], -1).astype(F32)
        ver[i] = torch.tensor([np.cos(1.0 + i), np.sin(1.0 + i)], dtype=torch.float32, device=device)
        ver[i, cu(rows, device), cu(cols, device)] = cu(direct, device)
        pix.append((np.stack([cols, rows], 1).astype(F32), direct))
    fg = mask != 0
    idxs, keep, tn = restated_draws(seed, fg, nh, vn, 100, 30000)
    assert tn == [int(f.sum()) for f in fg] and len(set(tn)) == b
    md = cu(mask, device)

    def call(m, v, **kw):
        diag = {}
        kp = rvg.ransac_voting_layer_v3(m, v, nh, _seed=seed, _diag=diag, **kw)
        out = {k: diag[k].cpu().numpy() for k in DIAG_KEYS}
        out["kp"] = kp.cpu().numpy()
        return out
    seeded = call(md, ver)
    injected = call(md, ver, _idxs=idxs)
    assert seeded["tn"].tolist() == tn
    assert_same_bits(seeded, injected, [True] * b, "batch")
    for i in (0, 14, 15, 16):
        single = call(md[i:i + 1], ver[i:i + 1], _idxs=idxs[i:i + 1])
        assert_same_bits({k: v[i:i + 1] for k, v in injected.items()}, single, [True], f"image {i} alone")
        coords, direct = pix[i]
        np.testing.assert_array_equal(bits(injected["hyp"][i]), bits(O.generate_hypothesis(direct, coords, idxs[i])))
        np.testing.assert_array_equal(injected["counts"][i].T, O.vote_counts(direct, coords, injected["hyp"][i], 0.99),
                                      err_msg=f"image {i} counts")
