"""The voting entries' case matrix: entry x mask kind x field layout x class count (host only,
numpy + the CPU oracle).  tests/test_entry_cases.py proves the cases fair on the CPU,
tests/test_gpu_entry_matrix.py runs them through the C ABI.

  * ``cell_scene``: a label map made of a grid of cells, one cell per class, whose fill cycles
    through the states a class can be in (FILLS): above max_num, between the bounds, below
    min_num, empty.  Every class's field channels hold noise off its own pixels.
  * ``logits_for`` / ``argmax_label``: logits whose argmax is a given label map, with the ties
    and NaNs torch.argmax decides planted on pixel runs of their own; the argmax restated as
    the plain loop over the planes.
  * ``field_tensor`` / ``mask_tensor``: the layouts a caller may hand the library (FIELD_LAYOUTS, PLACED, KINDS).
  * ``Case`` / ``inputs`` / ``reference``: one call, its host inputs and what the oracle gives
    per virtual image bv = bi * ncls + c.
  * ``TABLE``: a pairwise covering array over the factors (``generate_table`` made it), and the
    named parts A-E beside it (``part_a`` ...); ``route_scene`` and ``split_scene`` build part D.
"""
import dataclasses
import functools
import itertools

import numpy as np

from oracle import oracle as O
from tests import front_ref as R

F32 = np.float32
FILLS = ("full", "full", "two_thirds", "half", "below", "empty", "full", "above")
EVD_ROUNDS = {40: (40, 1), 128: (64, 2), 512: (256, 2)}      # nh -> (round_hyp_num, rounds)
SEG = ("seg_f32", "seg_f16")
NO_DS = 30000


# ---------------------------------------------------------------- scenes
def grid(H, W, n):
    """(rows, cols, slot height, slot width) of the grid of >= n slots whose slots are the least thin."""
    best = None
    for gr in range(1, min(H, n) + 1):
        gc = -(-n // gr)
        if gc > W:
            continue
        sh, sw = H // gr, W // gc
        key = (min(sh, sw), sh * sw)
        if best is None or key > best[0]:
            best = (key, gr, gc, sh, sw)
    return best[1:]


def strays_for(ncls):
    """Labels of no class: the next one, around a byte's wrap, negative, above 32 bits."""
    return [ncls + 1, 255, 256, 257, 300, -1, -2 ** 31, 2 ** 32 + 1] if ncls >= 1 else [256]


def cell_scene(H, W, ncls, vn, b, seed, min_num=0, max_num=0, fill0=0, cell=None):
    """dict: label int64 [b,H,W], vertex f32 [b,H,W,nc*vn,2] (nc = max(ncls, 1)), kps f32
    [b,nc,vn,2], fills int [b,nc] (index into FILLS), min_num, max_num (what makes a full cell
    downsample) and the cell's pixel count.

    Class c of image bi sits in cell (c + step * bi) mod cells, centred in its grid slot and at
    most 24 x 48 px (``cell``: grid slots of that size instead of the least thin ones); cell j holds
    FILLS[(j + fill0) mod 8] of its pixels, a random subset.
    Keypoint targets lie 3 px from the cell's centre, off the lattice; the class's pixels point
    at them with 0.02 rad of noise, every other pixel of its channels is N(0, 1).  ncls = 0 is the
    single-object scene: values 1 and 2 in the cell (mask.byte() != 0 takes both, mask == 1 only
    the first) and 256 outside it (no foreground for either).  Stray labels sit on pixels of no
    occupied cell, the frame's first pixel among them where it is free; the last pixel belongs to a
    class, so that a tail lane reading it again would count."""
    rng = np.random.default_rng([seed, H, W, ncls, vn, b])
    nc = max(ncls, 1)
    if cell:                                                   # slots of exactly this size
        sh, sw = cell
        gr, gc = H // sh, W // sw
        assert gr * gc > nc
    else:
        gr, gc, sh, sw = grid(H, W, nc + 1 if H * W < 1024 else max(nc + 1, 8))
    bh, bw = min(sh, 24), min(sw, 48)
    A = bh * bw
    min_num = min_num or max(2, A // 4)
    n_fill = {"full": A, "two_thirds": -(-2 * A // 3), "half": -(-A // 2), "below": min_num - 1, "empty": 0,
              "above": min_num + 1}
    # a full cell is above max_num, two thirds of one is not; a single-object cell counts its 1s
    # (every sixth pixel is a 2), so that mask == 1 downsamples it too
    max_num = max_num or ((A if ncls else A - A // 6) + n_fill["two_thirds"]) // 2
    assert n_fill["full"] > max_num >= n_fill["two_thirds"] and n_fill["half"] >= min_num > n_fill["below"] >= 1
    cells = gr * gc
    step = 3 if cells >= 4 else 1
    label = np.zeros((b, H, W), np.int64)
    ver = rng.standard_normal((b, H, W, nc * vn, 2)).astype(F32)
    kps = np.zeros((b, nc, vn, 2), F32)
    fills = np.zeros((b, nc), np.int64)
    for bi in range(b):
        occupied = np.zeros((H, W), bool)
        for c in range(nc):
            j = (c + step * bi) % cells
            fills[bi, c] = (j + fill0) % 8
            r0, c0 = (j // gc) * sh + (sh - bh) // 2, (j % gc) * sw + (sw - bw) // 2
            occupied[r0:r0 + bh, c0:c0 + bw] = True
            pix = rng.permutation(A)[:n_fill[FILLS[fills[bi, c]]]]
            rows, cols = r0 + pix // bw, c0 + pix % bw
            label[bi, rows, cols] = c + 1 if ncls else np.where(np.arange(len(pix)) % 6 == 5, 2, 1)
            theta = 2 * np.pi * (np.arange(vn) + rng.random()) / vn
            kp = np.stack([np.floor(c0 + (bw - 1) / 2 + 3 * np.cos(theta)) + 0.37,
                           np.floor(r0 + (bh - 1) / 2 + 3 * np.sin(theta)) + 0.41], 1)
            kps[bi, c] = kp
            d = kp[None] - np.stack([cols, rows], 1)[:, None]
            ang = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0, 0.02, d.shape[:2])
            ver[bi, rows, cols, c * vn:(c + 1) * vn] = np.stack([np.cos(ang), np.sin(ang)], -1)
        free = np.flatnonzero(~occupied)
        spots = np.unique(np.concatenate([free[:1], free[-1:], rng.choice(free, min(len(free), 14), replace=False)]))
        for k, p in enumerate(spots):
            label[bi].reshape(-1)[p] = strays_for(ncls)[k % len(strays_for(ncls))]
        # the frame's last pixel (what a load clamped to the image reads again) belongs to the image's
        # first class whose cell is at least half full, pointing at its targets like the class's own
        solid = [c for c in range(nc) if FILLS[fills[bi, c]] in ("full", "two_thirds", "half")]
        if solid and not occupied[H - 1, W - 1]:
            c = solid[0]
            label[bi, H - 1, W - 1] = c + 1
            d = kps[bi, c] - np.array([W - 1, H - 1])
            ang = np.arctan2(d[:, 1], d[:, 0]) + rng.normal(0, 0.02, vn)
            ver[bi, H - 1, W - 1, c * vn:(c + 1) * vn] = np.stack([np.cos(ang), np.sin(ang)], -1)
    return dict(label=label, vertex=ver, kps=kps, fills=fills, min_num=min_num, max_num=max_num, cell=A)


def route_scene(H, W, ncls, vn, seed):
    """cell_scene's dict for a frame above the fused hypotheses' 1,536 chunks (part D): each class is two
    16 x 24 blobs 400 rows apart -- far more than 300 chunks -- that see their keypoint targets, to the
    side of both, under different angles; strays on the first two pixels, the last pixel class 0's."""
    rng = np.random.default_rng([seed, H, W, ncls, vn])
    label = np.zeros((1, H, W), np.int64)
    ver = rng.standard_normal((1, H, W, ncls * vn, 2)).astype(F32)
    kps = np.zeros((1, ncls, vn, 2), F32)
    for c in range(ncls):
        own = np.zeros((H, W), bool)
        own[20 + 30 * c:36 + 30 * c, 100 + 250 * c:124 + 250 * c] = True
        own[420 + 30 * c:436 + 30 * c, 140 + 250 * c:164 + 250 * c] = True
        own &= rng.random((H, W)) < 0.8
        label[0][own] = c + 1
        rows, cols = np.nonzero(own)
        kp = np.stack([np.floor(rng.uniform(380, 440, vn)) - 250 * c + 0.37, np.floor(rng.uniform(200, 260, vn)) + 0.41], 1)
        kps[0, c] = kp
        d = kp[None] - np.stack([cols, rows], 1)[:, None]
        ang = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0, 0.02, d.shape[:2])
        ver[0, rows, cols, c * vn:(c + 1) * vn] = np.stack([np.cos(ang), np.sin(ang)], -1)
    label[0, 0, 0], label[0, 0, 1], label[0, -1, -1] = ncls + 1, 255, 1     # the last pixel is class 0's
    d = kps[0, 0] - np.array([W - 1, H - 1])
    ver[0, -1, -1, :vn] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return dict(label=label, vertex=ver, kps=kps, fills=np.full((1, ncls), 3), min_num=100, max_num=NO_DS, cell=384)


def occupied_chunks(label, c):
    """The 256-pixel chunks that hold a pixel of class c."""
    return np.flatnonzero(np.add.reduceat((label.reshape(-1) == c + 1).astype(np.int64), np.arange(0, label.size, 256)))


def label_as(label, kind, ncls):
    """The label map in an integer kind's dtype.  A single-object mask wraps (256 is byte 0, as
    mask.byte()); a stray label that does not fit becomes another label of no class."""
    dt = {"i64": np.int64, "i32": np.int32, "u8": np.uint8}[kind]
    if kind == "i64":
        return label.copy()
    if ncls == 0:
        return label.astype(dt)
    info = np.iinfo(dt)
    return np.where((label < info.min) | (label > info.max), 255 if kind == "u8" else 300, label).astype(dt)


def argmax_label(logits):
    """int64 argmax over axis 1 of [b,C,H,W] logits: the first maximum, NaN the greatest (it beats
    +inf and a later NaN does not replace it) -- the plain loop over the planes."""
    x = np.asarray(logits).astype(F32)
    best = x[:, 0].copy()
    lab = np.zeros(best.shape, np.int64)
    for k in range(1, x.shape[1]):
        v = x[:, k]
        with np.errstate(invalid="ignore"):
            upd = ~np.isnan(best) & (np.isnan(v) | (v > best))
        best = np.where(upd, v, best)
        lab[upd] = k
    return lab


PLANTS = ("tie", "last", "nan_vs_inf", "two_nans", "nan_plane0", "all_equal", "neg_inf", "f16_tie")


def plant_runs(b, H, W):
    """(image, first flat pixel, length) of each planted run: pixels of its own for every plant."""
    P = H * W
    L = max(1, min(8, P // 256))
    return [(k % b, (k + 1) * P // (len(PLANTS) + 1), L) for k in range(len(PLANTS))]


def logits_for(label, ncls, rng):
    """f32 [b,n+1,H,W] (n = max(ncls, 1)) whose argmax is ``label`` (values 0..n), then the PLANTS
    on the runs of plant_runs, in planes >= 4 where n allows (a plane above n is clamped to n):
    a tie of planes 2 and 6; the maximum in the last plane; NaN in plane 5 against +inf in plane 1;
    NaNs in planes 4 and 7; NaN in plane 0; all planes equal; -inf everywhere but plane 5 (and,
    on the run's odd pixels, -inf everywhere); planes 3 and 6 at 2 and 2 + 2^-12, equal in f16."""
    b, H, W = label.shape
    n = max(ncls, 1)
    x = rng.standard_normal((b, n + 1, H, W)).astype(F32)
    np.put_along_axis(x, label[:, None], 6.0, 1)
    flat = x.reshape(b, n + 1, H * W)

    def two(p, q):                                   # two different planes, clamped to n
        p, q = min(p, n), min(q, n)
        return (p - 1, q) if p == q else (p, q)
    for name, (bi, p0, L) in zip(PLANTS, plant_runs(b, H, W)):
        s = flat[bi, :, p0:p0 + L]
        if name == "tie":
            p, q = two(2, 6)
            s[p] = s[q] = 9.0
        elif name == "last":
            s[n] = 9.0
        elif name == "nan_vs_inf":
            p, q = two(1, 5)
            s[p], s[q] = np.inf, np.nan
        elif name == "two_nans":
            p, q = two(4, 7)
            s[p] = s[q] = np.nan
        elif name == "nan_plane0":
            s[0] = np.nan
        elif name == "all_equal":
            s[:] = 1.0
        elif name == "neg_inf":
            keep = s[min(5, n), ::2].copy()
            s[:] = -np.inf
            s[min(5, n), ::2] = keep
        elif name == "f16_tie":
            p, q = two(3, 6)
            s[:] = -1.0
            s[p], s[q] = 2.0, 2.0 + 2.0 ** -12
    return x


# ---------------------------------------------------------------- layouts
FIELD_LAYOUTS = ("f32_nhwc", "f32_nchw", "f16_nchw", "f16_nhwc_crop")
KINDS = ("i64", "i32", "u8", "seg_f32", "seg_f16")          # each mask kind has one layout: mask_tensor
PLACED = ("f32_nhwc_in", "f32_nhwc_end", "f16_nchw_in", "f16_nchw_end")      # part E


def field_is_half(layout):
    return layout.startswith("f16")


def field_tensor(layout, ver, device, place=None):
    """(view [b,H,W,CH,2], the tensor that owns its memory) of the f32 field ``ver`` in a layout.
    Cropped and placed views sit in NaN-filled allocations: "_in" with padding rows, columns and
    channels on every side, "_end" with padding in front only, so that the view's last element is
    the allocation's last.  ``place``: numpy array -> the device tensor that owns it (default: a copy
    to ``device``)."""
    import torch
    b, H, W, CH, _ = ver.shape
    dt = np.float16 if field_is_half(layout) else np.float32

    def dev(a):
        a = np.array(a, order="C")                                          # a copy: the case's inputs stay read-only
        return torch.from_numpy(a).to(device) if place is None else place(a)
    if layout == "f32_nhwc":
        t = dev(ver)
        return t, t
    if layout in ("f32_nchw", "f16_nchw"):
        base = dev(ver.astype(dt).reshape(b, H, W, CH * 2).transpose(0, 3, 1, 2))
        return base.permute(0, 2, 3, 1).unflatten(3, (CH, 2)), base
    if layout == "f16_nhwc_crop":
        big = np.full((b, H + 2, W + 3, CH + 1, 2), np.nan, dt)
        big[:, 1:H + 1, 2:W + 2, 1:] = ver
        base = dev(big)
        return base[:, 1:H + 1, 2:W + 2, 1:], base
    after = 1 if layout.endswith("_in") else 0
    if layout.startswith("f32_nhwc"):
        big = np.full((b, 1 + H + after, 1 + W + after, 1 + CH + after, 2), np.nan, dt)
        big[:, 1:1 + H, 1:1 + W, 1:1 + CH] = ver
        base = dev(big)
        return base[:, 1:1 + H, 1:1 + W, 1:1 + CH], base
    if layout.startswith("f16_nchw"):
        big = np.full((b, 1 + CH + after, 2, 1 + H + after, 1 + W + after), np.nan, dt)
        big[:, 1:1 + CH, :, 1:1 + H, 1:1 + W] = ver.transpose(0, 3, 4, 1, 2)
        base = dev(big)
        return base[:, 1:1 + CH, :, 1:1 + H, 1:1 + W].permute(0, 3, 4, 1, 2), base
    raise ValueError(layout)


def mask_tensor(kind, arr, device, place=None):
    """(view, owner): ``arr`` is the label map [b,H,W] in the kind's dtype, or logits [b,C,H,W].
    i64: dense; i32: a cropped view whose row stride is above W; u8: a transposed-memory view;
    seg_f32: channels-last memory; seg_f16: a cropped NCHW view.
    The int32 view's padding holds label 1 and the f16 logits' padding NaN: a read outside the
    view changes the result.  ``place``: as field_tensor's."""
    import torch

    def dev(a):
        a = np.array(a, order="C")                                          # a copy: the case's inputs stay read-only
        return torch.from_numpy(a).to(device) if place is None else place(a)
    if kind == "i64":
        t = dev(arr)
        return t, t
    if kind == "i32":
        b, H, W = arr.shape
        big = np.ones((b, H + 1, W + 5), np.int32)
        big[:, :H, 3:3 + W] = arr
        base = dev(big)
        return base[:, :H, 3:3 + W], base
    if kind == "u8":
        base = dev(arr.transpose(0, 2, 1))
        return base.transpose(1, 2), base
    if kind == "seg_f32":
        base = dev(arr.astype(F32).transpose(0, 2, 3, 1))
        return base.permute(0, 3, 1, 2), base
    if kind == "seg_f16":
        b, C, H, W = arr.shape
        big = np.full((b, C + 2, H + 1, W + 2), np.nan, np.float16)
        big[:, 1:C + 1, :H, 1:W + 1] = arr
        base = dev(big)
        return base[:, 1:C + 1, :H, 1:W + 1], base
    raise ValueError(kind)


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    entry: str                # v3 | v5 | evd_mean | evd_topk
    kind: str                 # i64 | i32 | u8 | seg_f32 | seg_f16
    field: str                # FIELD_LAYOUTS or PLACED
    ncls: int
    vn: int
    nh: int
    b: int
    H: int
    W: int
    ds: str = "none"          # none | keep | seed
    seed: int = 1
    min_num: int = 0          # 0: from the cell
    max_num: int = 0
    fill0: int = 0
    cell: tuple = None        # (h, w) of the grid's slots; None: the least thin grid
    scene: str = "cells"      # cells: cell_scene; route: route_scene

    @property
    def nc(self):
        return max(self.ncls, 1)

    @property
    def bv(self):
        return self.b * self.nc

    @property
    def rounds(self):
        return EVD_ROUNDS[self.nh] if self.entry.startswith("evd") else (self.nh, 1)

    @property
    def thresh(self):
        return 0.999 if self.entry == "v5" else 0.99

    @property
    def topk(self):
        return max(1, self.nh // 4)


LAYERS = ("ransac_voting_layer_v3", "ransac_voting_layer_v3_from_network", "ransac_voting_layer_v3_multi",
          "ransac_voting_layer_v3_multi_from_network", "ransac_voting_layer_v5",
          "estimate_voting_distribution_with_mean", "estimate_voting_distribution_with_mean_multi",
          "estimate_voting_distribution")


def layer_of(case):
    """The public layer of pvnet_amd.ransac_voting_gpu for the case's combination, or None: logits have
    the two v3 *_from_network layers, which take the NCHW vertex_pred itself; a multi-object call has
    v3 and EVD-with-mean."""
    seg, multi = case.kind in SEG, case.ncls > 0
    if seg:
        if case.entry != "v3" or case.field not in ("f32_nchw", "f16_nchw"):
            return None
        return "ransac_voting_layer_v3_multi_from_network" if multi else "ransac_voting_layer_v3_from_network"
    if multi:
        return {"v3": "ransac_voting_layer_v3_multi", "evd_mean": "estimate_voting_distribution_with_mean_multi"}.get(case.entry)
    return {"v3": "ransac_voting_layer_v3", "v5": "ransac_voting_layer_v5", "evd_mean": "estimate_voting_distribution_with_mean",
            "evd_topk": "estimate_voting_distribution"}[case.entry]


def virtual_masks(case, label):
    """int64 [bv,H,W]: what the oracle votes per virtual image -- label == c + 1, or the
    single-object mask itself (the entry's own foreground rule applies to it)."""
    if case.ncls == 0:
        return label.astype(np.int64)
    return np.stack([(label[bi] == c + 1).astype(np.int64) for bi in range(case.b) for c in range(case.ncls)])


def foreground(case, vmask):
    return np.stack([O.fg_mask_evd(m) if case.entry.startswith("evd") else O.fg_mask_v3(m) for m in vmask])


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The host side of a call: ``mask`` (label map in the kind's dtype, or logits), ``label`` (int64,
    what the device decodes from it), ``field`` (f32, rounded to the device's kind), ``vfield``
    [bv,H,W,vn,2], ``idxs`` [bv,nh,vn,2], ``keep`` [bv,H,W] or None, ``mean`` [bv,vn,2], the bounds."""
    if case.scene == "route":
        sc = route_scene(case.H, case.W, case.ncls, case.vn, case.seed)
    else:
        sc = cell_scene(case.H, case.W, case.ncls, case.vn, case.b, case.seed, case.min_num, case.max_num, case.fill0,
                        case.cell)
    rng = np.random.default_rng([case.seed, 77])
    label = sc["label"]
    if case.kind in SEG:
        clean = O.fg_mask_v3(label).astype(np.int64) if case.ncls == 0 else \
            np.where((label < 0) | (label > case.ncls), 0, label)
        mask = logits_for(clean, case.ncls, rng)
        if case.kind == "seg_f16":
            mask = mask.astype(np.float16)
        label = argmax_label(mask)
    else:
        mask = label_as(label, case.kind, case.ncls)
        label = mask.astype(np.int64)
    field = sc["vertex"].astype(np.float16).astype(F32) if field_is_half(case.field) else sc["vertex"]
    b, H, W, vn, nc = case.b, case.H, case.W, case.vn, case.nc
    vfield = field.reshape(b, H, W, nc, vn, 2).transpose(0, 3, 1, 2, 4, 5).reshape(b * nc, H, W, vn, 2)
    min_num = sc["min_num"]
    max_num = NO_DS if case.ds == "none" else sc["max_num"]
    fg = foreground(case, virtual_masks(case, label))
    fgn = fg.reshape(case.bv, -1).sum(1)
    if case.ds == "seed":
        keep = R.keep_mask(case.seed, fg, max_num)
    elif case.ds == "keep":                                    # drops down to max_num exactly
        keep = np.ones((case.bv, H, W), np.uint8)
        for i in np.flatnonzero(fgn > max_num):
            keep[i].reshape(-1)[rng.choice(np.flatnonzero(fg[i]), fgn[i] - max_num, replace=False)] = 0
    else:
        keep = None
    kept = fgn if keep is None else (fg & (keep != 0)).reshape(case.bv, -1).sum(1)
    tn = np.where(fgn < min_num, 0, np.where(fgn > max_num, kept, fgn))
    if case.ds == "seed":
        idxs = R.pairs(case.seed, tn, case.nh, vn)
    else:
        idxs = np.stack([rng.integers(0, max(t, 1), (case.nh, vn, 2), dtype=np.int32) for t in tn])
    mean = sc["kps"].reshape(case.bv, vn, 2) + F32(0.25)
    for a in (mask, label, field, idxs, mean) + (() if keep is None else (keep,)):
        a.setflags(write=False)
    return dict(mask=mask, label=label, field=field, vfield=vfield, idxs=idxs, keep=keep, mean=mean, min_num=min_num,
                max_num=max_num, fills=sc["fills"], kps=sc["kps"].reshape(case.bv, vn, 2), fgn=fgn, tn=tn)


def oracle_run(entry, vmask, vfield, idxs, keep, mean, nh, rounds, thresh, min_num, max_num, topk):
    """One virtual image through the oracle -> dict (tn = 0: skipped).  v3 / v5 through
    O.ransac_voting_layer_v5; EVD through O.compact / generate_hypothesis / vote_counts (tn, hyp,
    counts, and the winner's refine sums) and O.estimate_voting_distribution[_with_mean]."""
    vn = vfield.shape[2]
    kp1 = None if keep is None else keep[None]
    out = dict(tn=0, kp=np.zeros((vn, 2), F32), conf=np.zeros(vn, F32))
    if not entry.startswith("evd"):
        dg = []
        kp, conf = O.ransac_voting_layer_v5(vmask[None], vfield[None], nh, thresh, min_num=min_num, max_num=max_num,
                                            idxs=idxs[None], keep=kp1, diag=dg)
        d = dg[0]
        out["fg"] = d["foreground"]
        if not d.get("skipped"):
            out.update(tn=d["tn"], hyp=d["hyp"], counts=d["counts"], win_idx=d["win_idx"], ATA=d["ATA"], ATb=d["ATb"],
                       kp=kp[0], conf=conf[0])
        return out
    fg = O.fg_mask_evd(vmask)
    out["fg"] = int(fg.sum())
    rhn, nr = rounds
    if out["fg"] >= min_num:
        if out["fg"] > max_num:
            fg = fg & (keep != 0)
        coords, direct = O.compact(fg, vfield)
        hyp = O.generate_hypothesis(direct, coords, idxs)
        counts = O.vote_counts(direct, coords, hyp, thresh)
        win = O.argmax_first(counts, 0)
        _, ATA, ATb = O.refine(direct, coords, hyp[win, np.arange(vn)], thresh)
        out.update(tn=coords.shape[0], hyp=hyp, counts=counts, win_idx=win, ATA=ATA, ATb=ATb)
    kw = dict(round_hyp_num=rhn, min_hyp_num=nh, inlier_thresh=thresh, min_num=min_num, max_num=max_num,
              idxs=idxs.reshape(1, nr, rhn, vn, 2), keep=kp1)
    if entry == "evd_mean":
        m, cov = O.estimate_voting_distribution_with_mean(vmask[None], vfield[None], mean[None], **kw)
    else:
        m, cov = O.estimate_voting_distribution(vmask[None], vfield[None], topk=topk, **kw)
    out.update(mean=m[0], cov=cov[0])
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """list over the virtual images of oracle_run's dicts."""
    inp = inputs(case)
    vm = virtual_masks(case, inp["label"])
    ref = [oracle_run(case.entry, vm[i], inp["vfield"][i], inp["idxs"][i], None if inp["keep"] is None else inp["keep"][i],
                      inp["mean"][i], case.nh, case.rounds, case.thresh, inp["min_num"], inp["max_num"], case.topk)
           for i in range(case.bv)]
    assert [r["tn"] for r in ref] == inp["tn"].tolist()
    return ref


# ---------------------------------------------------------------- the pairwise table
FACTORS = (
    ("entry", ("v3", "v5", "evd_mean", "evd_topk")),
    ("kind", KINDS),
    ("field", FIELD_LAYOUTS),
    ("ncls", (0, 1, 3, 5)),
    ("nh", (40, 128, 512)),
    ("b", (1, 3)),
    ("ds", ("none", "keep", "seed")),
    ("frame", ((10, 10), (16, 16), (37, 51), (3, 700))),
)


def pairs_of(row):
    return {((i, row[i]), (j, row[j])) for i, j in itertools.combinations(range(len(row)), 2)}


def generate_table(seed=2024, tries=128):
    """Seeded greedy covering array: each new row is the best of ``tries`` random rows by the
    number of level pairs it covers for the first time (ties: the first drawn)."""
    rng = np.random.default_rng(seed)
    levels = [f[1] for f in FACTORS]
    todo = set()
    for i, j in itertools.combinations(range(len(levels)), 2):
        todo |= {((i, a), (j, c)) for a in levels[i] for c in levels[j]}
    rows = []
    while todo:
        cand = [tuple(lv[rng.integers(len(lv))] for lv in levels) for _ in range(tries)]
        gain = [len(pairs_of(r) & todo) for r in cand]
        best = cand[int(np.argmax(gain))]
        if max(gain) == 0:                                      # finish an uncovered pair directly
            (i, a), (j, c) = sorted(todo, key=repr)[0]
            best = tuple(a if k == i else c if k == j else v for k, v in enumerate(best))
        rows.append(best)
        todo -= pairs_of(best)
    return rows


# generate_table() written out: (entry, kind, field, ncls, nh, b, ds, (H, W))
TABLE = [
    ('v3', 'seg_f32', 'f32_nhwc', 0, 40, 1, 'seed', (3, 700)),
    ('evd_topk', 'i64', 'f32_nchw', 0, 128, 3, 'keep', (10, 10)),
    ('v5', 'u8', 'f16_nchw', 3, 40, 3, 'none', (16, 16)),
    ('v5', 'i32', 'f16_nhwc_crop', 1, 512, 1, 'none', (37, 51)),
    ('evd_mean', 'seg_f16', 'f32_nchw', 3, 512, 1, 'seed', (37, 51)),
    ('evd_mean', 'u8', 'f32_nhwc', 5, 512, 3, 'seed', (10, 10)),
    ('v3', 'u8', 'f16_nchw', 5, 128, 1, 'keep', (37, 51)),
    ('evd_mean', 'i32', 'f16_nhwc_crop', 1, 128, 3, 'keep', (16, 16)),
    ('v5', 'seg_f32', 'f16_nhwc_crop', 3, 128, 3, 'keep', (3, 700)),
    ('evd_topk', 'seg_f16', 'f16_nchw', 1, 40, 3, 'seed', (10, 10)),
    ('evd_topk', 'seg_f32', 'f32_nchw', 5, 512, 3, 'none', (3, 700)),
    ('v5', 'seg_f16', 'f32_nhwc', 5, 128, 1, 'none', (16, 16)),
    ('evd_mean', 'i64', 'f16_nhwc_crop', 0, 40, 3, 'seed', (37, 51)),
    ('v3', 'i64', 'f32_nhwc', 0, 512, 1, 'keep', (16, 16)),
    ('v3', 'i32', 'f32_nchw', 1, 128, 3, 'none', (10, 10)),
    ('v5', 'i32', 'f32_nchw', 5, 40, 1, 'seed', (16, 16)),
    ('evd_topk', 'u8', 'f16_nhwc_crop', 0, 40, 1, 'none', (10, 10)),
    ('evd_mean', 'seg_f32', 'f16_nchw', 1, 128, 3, 'seed', (3, 700)),
    ('evd_topk', 'seg_f32', 'f32_nhwc', 3, 128, 1, 'keep', (37, 51)),
    ('v5', 'i64', 'f16_nchw', 5, 512, 3, 'none', (3, 700)),
    ('v3', 'seg_f32', 'f16_nhwc_crop', 3, 40, 1, 'none', (10, 10)),
    ('evd_topk', 'seg_f16', 'f16_nhwc_crop', 3, 40, 3, 'keep', (3, 700)),
    ('evd_topk', 'i32', 'f16_nchw', 0, 128, 1, 'none', (10, 10)),
    ('v5', 'seg_f16', 'f32_nchw', 0, 128, 3, 'seed', (10, 10)),
    ('evd_mean', 'i32', 'f32_nhwc', 1, 128, 1, 'seed', (3, 700)),
    ('v3', 'u8', 'f32_nchw', 1, 128, 3, 'none', (3, 700)),
    ('v3', 'seg_f32', 'f16_nhwc_crop', 5, 512, 1, 'none', (16, 16)),
    ('evd_mean', 'i64', 'f32_nchw', 1, 40, 1, 'none', (37, 51)),
    ('evd_topk', 'i64', 'f16_nhwc_crop', 3, 512, 1, 'keep', (16, 16)),
    ('v3', 'seg_f16', 'f32_nhwc', 1, 512, 1, 'none', (16, 16)),
    ('evd_topk', 'i32', 'f32_nchw', 3, 40, 1, 'keep', (10, 10)),
]

TABLE_VN = (2, 3, 1, 13)          # row i votes TABLE_VN[i mod 4] keypoints per class (13: a second load group)
# rows whose only class below min_num is the last one, which the planted logits' pixels would lift
# over it: the fills start one later, so that the last class's cell is empty and stays skipped
TABLE_FILL0 = {11: 1, 26: 1}


def table_cases():
    return [Case(f"F{i:02d}-{e}-{k}-{f}-c{n}-nh{nh}-b{b}-{ds}-{H}x{W}", e, k, f, n, TABLE_VN[i % 4], nh, b, H, W, ds,
                 seed=100 + i, fill0=TABLE_FILL0.get(i, 0))
            for i, (e, k, f, n, nh, b, ds, (H, W)) in enumerate(TABLE)]


# ---------------------------------------------------------------- the named parts
def part_a():
    """Label reading: 37 x 51 (8 chunks, a tail of 95), vn 2, b 2, nh 128; every class count that
    ends a group of four logit planes differently; 5 and 64 also at nh 40; 64 classes with b 9 on
    the wide label counter."""
    out = []
    for ncls in (1, 3, 4, 5, 7, 8, 64):
        for kind in KINDS:
            for nh in (128, 40) if ncls in (5, 64) else (128,):
                kw = dict(min_num=10, max_num=20, cell=(4, 6)) if ncls == 64 else {}
                out.append(Case(f"A-c{ncls}-{kind}-nh{nh}", "v3", kind, "f32_nhwc", ncls, 2, nh, 2, 37, 51, "keep",
                                seed=7, **kw))
    for kind in ("u8", "seg_f16"):
        out.append(Case(f"A-c64-{kind}-b9-wide", "v3", kind, "f32_nhwc", 64, 2, 128, 9, 37, 51, "keep", seed=8,
                        min_num=10, max_num=20, cell=(4, 6)))
    return out


def part_b():
    """Logits into v5 and both EVD entries, single object: image 1 of the two is below min_num
    (fill0 = 2: image 1's cell is empty, its only foreground the planted logits' pixels); the wide
    form with 520 images of one keypoint."""
    out = [Case(f"B-{e}-{k}", e, k, "f16_nchw", 0, 2, 128, 2, 37, 51, "none", seed=11, fill0=2)
           for e in ("v5", "evd_mean", "evd_topk") for k in SEG]
    out.append(Case("B-v5-seg_f32-b520-wide", "v5", "seg_f32", "f16_nchw", 0, 1, 128, 520, 37, 51, "none", seed=12))
    out.append(Case("B-evd_mean-seg_f16-b520-wide", "evd_mean", "seg_f16", "f16_nchw", 0, 1, 128, 520, 37, 51, "none",
                    seed=13))
    return out


def part_c():
    """Multi-object v5, EVD top-k and EVD-with-mean: conf, mean and cov indexed by the virtual image."""
    return [Case(f"C-{e}-{k}", e, k, "f32_nchw", 5, 3, 128, 2, 37, 51, "keep", seed=21)
            for e in ("v5", "evd_topk", "evd_mean") for k in ("i32", "seg_f16")]


def part_e():
    """Field placement: the view inside a NaN-filled allocation, and ending on its last element."""
    return [Case(f"E-{f}", "v3", "i64", f, 3, 3, 128, 2, 37, 51, "keep", seed=31) for f in PLACED]


def part_d_route():
    """607 x 648 is 1,537 chunks: k_hyp_gen makes the hypotheses and the class words of the virtual images."""
    return [Case(f"D-route-{k}", "v3", k, "f32_nhwc", 2, 2, 512, 1, 607, 648, "none", seed=41, scene="route")
            for k in ("u8", "seg_f32")]


SPLIT = dict(ncls=17, vn=64, H=256, W=256, nh=4096, checked=(0, 14, 15, 16), nonfinite_sets=(5, 9))


def split_fixed(c, W):
    """Class c's five fixed pixels (flat) and their f16 directions: A and B cross exactly on C's
    centre (a lattice hypothesis, exact-only, and a foreground pixel of the class sits on it); D and
    E are almost parallel and cross 9.6e6 px away (finite, beyond the matrix-core form's domain)."""
    px = {"A": (20, 10 + c), "B": (30, 40 + c), "C": (30, 10 + c), "D": (40, 70 + c), "E": (41, 70 + c)}
    dirs = {"A": (1.0, 0.0), "B": (0.0, 1.0), "D": (0.0, 4.0), "E": (float(np.float16(4.17e-7)), 4.0)}
    return {k: y * W + x for k, (x, y) in px.items()}, dirs


@functools.lru_cache(maxsize=None)
def split_scene():
    """Part D's launch split: one image of 17 classes x 64 keypoints at 256 x 256 and nh = 4096 is
    2^27 vote units per virtual image, so front_half votes 15 + 2 of them: the cut falls inside the
    image.  Class c holds 191 + c pixels scattered over the frame, split_fixed's five among them.
    The ``checked`` virtual images hold whole 32-hypothesis sets of lattice and of far hypotheses,
    at different sets before and after the cut (0, 14: sets 5 and 7; 15, 16: sets 1 and 3), so that
    a launch reading another launch's class words votes them in the wrong form -- which still counts
    a finite hypothesis right, so virtual image 1 (the second launch's image 16 would read its words)
    holds sets 5 and 9 of non-finite hypotheses, of neither class and never voted: its pixel A carries
    an f16 infinity.  Image 1 is compared in tn alone.  The field (285 MB
    in f16) is made on the device; here are the label map, each class's pixels with their
    f16-rounded directions, the injected pairs and, for the checked images, the oracle's
    hypotheses, counts and the winners' refine sums."""
    ncls, vn, H, W, nh = (SPLIT[k] for k in ("ncls", "vn", "H", "W", "nh"))
    rng = np.random.default_rng(4096)
    P = H * W
    fixed = [split_fixed(c, W) for c in range(ncls)]
    taken = np.zeros(P, bool)
    for f, _ in fixed:
        taken[list(f.values())] = True
    order = rng.permutation(np.flatnonzero(~taken))
    label = np.zeros(P, np.int32)
    pix, start = [], 0
    for c in range(ncls):
        n = 191 + c - 5
        p = np.sort(np.concatenate([order[start:start + n], list(fixed[c][0].values())]))
        start += n
        label[p] = c + 1
        rows, cols = np.divmod(p, W)
        kp = np.stack([rng.uniform(0.2, 0.8, vn) * W + 0.37, rng.uniform(0.2, 0.8, vn) * H + 0.41], 1)
        d = kp[None] - np.stack([cols, rows], 1)[:, None]
        ang = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0, 0.02, d.shape[:2])
        direct = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float16)
        for k, dv in fixed[c][1].items():
            direct[np.searchsorted(p, fixed[c][0][k])] = np.float16((np.inf, 0.0) if (c, k) == (1, "A") else dv)
        pix.append((rows, cols, direct))
    for k, q in enumerate(order[start:start + 8]):
        label[q] = (ncls + 1, 255, 256, 257, 300, -1, -2 ** 31, 64)[k]
    tn = np.array([len(q[0]) for q in pix])
    idxs = np.stack([rng.integers(0, t, (nh, vn, 2), dtype=np.int32) for t in tn])
    rows, cols, direct = pix[1]
    t = {k: int(np.searchsorted(rows * W + cols, q)) for k, q in fixed[1][0].items()}
    for s_ in SPLIT["nonfinite_sets"]:
        idxs[1, 32 * s_:32 * s_ + 32] = (t["A"], t["B"])
    hyp1 = O.generate_hypothesis(direct.astype(F32), np.stack([cols, rows], 1).astype(F32), idxs[1])
    ref = {}
    for i in SPLIT["checked"]:
        rows, cols, direct = pix[i]
        t = {k: int(np.searchsorted(rows * W + cols, q)) for k, q in fixed[i][0].items()}
        s_lat, s_far = (1, 3) if i >= 15 else (5, 7)
        idxs[i, 32 * s_lat:32 * s_lat + 32] = (t["A"], t["B"])
        idxs[i, 32 * s_far:32 * s_far + 32] = (t["D"], t["E"])
        coords, direct = np.stack([cols, rows], 1).astype(F32), direct.astype(F32)
        hyp = O.generate_hypothesis(direct, coords, idxs[i])
        counts = O.vote_counts(direct, coords, hyp, 0.99)
        _, ATA, _ = O.refine(direct, coords, hyp[O.argmax_first(counts, 0), np.arange(vn)], 0.99)
        ref[i] = dict(hyp=hyp, counts=counts, ATA=ATA, lattice=hyp[32 * s_lat:32 * s_lat + 32],
                      far=hyp[32 * s_far:32 * s_far + 32], sets=(s_lat, s_far))
    return dict(label=label.reshape(1, H, W), pix=pix, tn=tn, idxs=idxs, ref=ref, hyp1=hyp1)


def part_layers():
    """The public layers no other part's combination has: the two *_from_network layers take the NCHW
    vertex_pred itself (parts A and B put logits on other fields), v5's takes a single-object mask."""
    return [Case("L-v3-seg_f16-from_network", "v3", "seg_f16", "f16_nchw", 0, 2, 128, 2, 37, 51, "keep", seed=51),
            Case("L-v3-seg_f32-multi_from_network", "v3", "seg_f32", "f32_nchw", 3, 2, 512, 2, 37, 51, "keep", seed=52),
            Case("L-v5-i64", "v5", "i64", "f32_nhwc", 0, 2, 128, 2, 37, 51, "keep", seed=53)]


def all_cases():
    return part_a() + part_b() + part_c() + part_d_route() + part_e() + table_cases() + part_layers()
