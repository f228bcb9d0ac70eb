"""tests/entry_cases.py proven fair on the CPU, so that the GPU run of the same cases
(tests/test_gpu_entry_matrix.py) cannot hide anything: the table covers every pair of levels,
the restated argmax is torch's, the layouts are views of what they claim, and every case reaches
the states it is there for on a well-conditioned reference."""
import itertools

import numpy as np
import pytest
import torch

from tests import entry_cases as EC
from tests.test_hyp_class import EXACT, FAST, restated

COND_MAX = 50.0


def test_table_is_the_generators_and_covers_every_pair():
    assert EC.TABLE == EC.generate_table()
    assert 30 <= len(EC.TABLE) <= 31
    levels = [f[1] for f in EC.FACTORS]
    seen = set()
    for row in EC.TABLE:
        assert len(row) == len(levels) and all(v in lv for v, lv in zip(row, levels))
        seen |= EC.pairs_of(row)
    for i, j in itertools.combinations(range(len(levels)), 2):
        for a in levels[i]:
            for c in levels[j]:
                assert ((i, a), (j, c)) in seen, (EC.FACTORS[i][0], a, EC.FACTORS[j][0], c)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("ncls", [0, 1, 3, 4, 5, 7, 8, 64])
def test_argmax_label_is_torch_argmax(ncls, half):
    """On every planted run (and the whole frame), with f16 logits widened first; the plants give
    the labels their rule says."""
    b, H, W = 2, 37, 51
    rng = np.random.default_rng(ncls)
    n = max(ncls, 1)
    label = rng.integers(0, n + 1, (b, H, W))
    x = EC.logits_for(label, ncls, rng)
    if half:
        x = x.astype(np.float16)
    got = EC.argmax_label(x)
    want = torch.argmax(torch.from_numpy(x.astype(np.float32)), 1).numpy()
    np.testing.assert_array_equal(got, want)
    planted = np.zeros((b, H * W), bool)
    flat = got.reshape(b, -1)
    rule = {}
    for name, (bi, p0, L) in zip(EC.PLANTS, EC.plant_runs(b, H, W)):
        planted[bi, p0:p0 + L] = True
        rule[name] = flat[bi, p0:p0 + L]
    np.testing.assert_array_equal(flat[~planted], label.reshape(b, -1)[~planted])
    assert planted.sum() == (H * W // 256) * len(EC.PLANTS)     # runs of 7 pixels, none overlapping
    assert np.all(rule["nan_plane0"] == 0) and np.all(rule["all_equal"] == 0) and np.all(rule["last"] == n)
    assert np.all(rule["neg_inf"][::2] == min(5, n)) and np.all(rule["neg_inf"][1::2] == 0)
    if n >= 7:
        assert np.all(rule["tie"] == 2) and np.all(rule["nan_vs_inf"] == 5) and np.all(rule["two_nans"] == 4)
        assert np.all(rule["f16_tie"] == (3 if half else 6))
    if n == 1:
        assert np.all(rule["tie"] == 0) and np.all(rule["nan_vs_inf"] == 1) and np.all(rule["two_nans"] == 0)
        assert np.all(rule["f16_tie"] == (0 if half else 1))


@pytest.mark.parametrize("layout", EC.FIELD_LAYOUTS + EC.PLACED)
def test_field_layouts_are_views_of_the_field(layout):
    rng = np.random.default_rng(1)
    ver = rng.standard_normal((2, 5, 7, 6, 2)).astype(np.float32)
    if EC.field_is_half(layout):
        ver = ver.astype(np.float16).astype(np.float32)
    view, base = EC.field_tensor(layout, ver, "cpu")
    assert tuple(view.shape) == ver.shape and view.dtype == (torch.float16 if EC.field_is_half(layout) else torch.float32)
    np.testing.assert_array_equal(view.float().numpy(), ver)
    assert view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
    if layout != "f32_nhwc":
        assert not view.is_contiguous()
    if layout.endswith("_end"):                                 # the view's last element is the allocation's last
        last = view.storage_offset() + sum((n - 1) * s for n, s in zip(view.shape, view.stride()))
        assert last == base.numel() - 1 and bool(torch.isnan(base.reshape(-1)[0]))
    if layout.endswith("_in") or layout.endswith("_crop"):
        assert bool(torch.isnan(base.reshape(-1)[0])) and bool(torch.isnan(base.reshape(-1)[-1]))


@pytest.mark.parametrize("kind", EC.KINDS)
def test_mask_layouts_are_views_of_the_mask(kind):
    rng = np.random.default_rng(2)
    if kind in EC.SEG:
        arr = rng.standard_normal((2, 4, 5, 7)).astype(np.float16 if kind == "seg_f16" else np.float32)
    else:
        arr = rng.integers(0, 5, (2, 5, 7)).astype({"i64": np.int64, "i32": np.int32, "u8": np.uint8}[kind])
    view, base = EC.mask_tensor(kind, arr, "cpu")
    np.testing.assert_array_equal(view.numpy(), arr)
    assert view.is_contiguous() == (kind == "i64")
    if kind == "i32":
        assert view.stride(1) > arr.shape[2]
    if kind == "u8":
        assert view.stride() == (35, 1, 5)


def test_label_kinds_keep_strays_outside_the_classes():
    sc = EC.cell_scene(37, 51, 3, 2, 2, 5)
    lab = sc["label"]
    assert {4, 255, 256, 257, 300, -1, -2 ** 31, 2 ** 32 + 1} <= set(lab.reshape(-1).tolist())
    for kind in ("i64", "i32", "u8"):
        a = EC.label_as(lab, kind, 3).astype(np.int64)
        for c in (1, 2, 3):
            np.testing.assert_array_equal(a == c, lab == c)
        assert ((a < 0) | (a > 3)).sum() == ((lab < 0) | (lab > 3)).sum()
    one = EC.cell_scene(37, 51, 0, 2, 2, 5)["label"]
    assert {0, 1, 2, 256} == set(one.reshape(-1).tolist())
    assert EC.label_as(one, "u8", 0).max() == 2                 # 256 wraps to 0, as mask.byte()


CASES = EC.all_cases()


def test_case_names_are_unique_and_parts_are_complete():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert len(EC.part_a()) == 7 * 5 + 2 * 5 + 2 and len(EC.part_b()) == 8 and len(EC.part_c()) == 6
    assert len(EC.part_e()) == 4 and len(EC.table_cases()) == len(EC.TABLE) and len(EC.part_d_route()) == 2
    assert len(EC.part_layers()) == 3


def test_every_public_layer_has_a_case():
    assert {EC.layer_of(c) for c in CASES} - {None} == set(EC.LAYERS)
    from pvnet_amd import ransac_voting_gpu as rvg             # the names are the module's
    assert all(callable(getattr(rvg, n)) for n in EC.LAYERS)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_fair(case):
    """>= 1 voted class in the batch; a skipped and a downsampled class where the scene has room
    (a cell below min_num or empty; a full cell and a downsampling case); every downsampled class
    keeps >= min_num pixels; cond(ATA) <= 50 in f64; cov finite."""
    inp, ref = EC.inputs(case), EC.reference(case)
    voted = [r for r in ref if r["tn"] > 0]
    assert voted, "no class voted"
    min_num, max_num = inp["min_num"], inp["max_num"]
    states = {EC.FILLS[f] for f in inp["fills"].reshape(-1)}
    if states & {"below", "empty"}:
        assert any(r["tn"] == 0 for r in ref), "no skipped class"
    down = [r for r in ref if r["fg"] > max_num and r["tn"] > 0]
    if "full" in states and case.ds != "none":
        assert down, "no downsampled class"
    for r in down:
        assert min_num <= r["tn"] < r["fg"]
    for r in voted:
        cond = np.linalg.cond(np.asarray(r["ATA"], np.float64))
        assert cond.max() <= COND_MAX, (cond.max(), r["tn"])
    for r in ref:
        if "cov" in r:
            assert np.isfinite(r["cov"]).all() and np.isfinite(r["mean"]).all()


def test_last_pixel_belongs_to_a_class():
    """What a load clamped to the image reads again counts for a class: in every frame with a partial
    last chunk (16 x 16 and 256 x 256 have none), in every image that holds a class at least half full."""
    tail = [c for c in CASES if c.H * c.W % 256]                # frames with a partial last chunk
    assert {(c.H, c.W) for c in tail} == {(10, 10), (37, 51), (3, 700), (607, 648)}
    for case in tail:
        inp = EC.inputs(case)
        last = inp["label"][:, -1, -1]
        solid = np.isin(inp["fills"], [i for i, f in enumerate(EC.FILLS) if f in ("full", "two_thirds", "half")]).any(1)
        assert solid.any() and np.all((last[solid] >= 1) & (last[solid] <= case.nc)), case.name
        owner = last[solid] - 1 + np.flatnonzero(solid) * case.nc          # the virtual image it counts for
        assert np.all(inp["fgn"][owner] > 0)


def test_named_cases_reach_their_states():
    """Part A / C / E cases hold voted, skipped and downsampled classes in one call (64 classes:
    all eight fills); part B's image 1 is below min_num; the wide cases are wide."""
    for case in EC.part_a() + EC.part_c() + EC.part_e():
        inp, ref = EC.inputs(case), EC.reference(case)
        if case.ncls >= 3:
            assert any(r["tn"] == 0 for r in ref) and any(r["fg"] > inp["max_num"] for r in ref)
        if case.ncls == 64:
            assert set(inp["fills"].reshape(-1).tolist()) == set(range(8))
            assert (inp["min_num"], inp["max_num"], EC.cell_scene(37, 51, 64, 2, 1, 0, 10, 20, 0, (4, 6))["cell"]) == (10, 20, 24)
    for case in EC.part_b():
        ref = EC.reference(case)
        assert ref[0]["tn"] > 0 and (case.b > 2 or ref[1]["tn"] == 0 < ref[1]["fg"])
    chunks = -(-37 * 51 // 256)
    wide = [c for c in CASES if chunks * c.bv > 4096 and (c.H, c.W) == (37, 51)]
    assert {c.name for c in wide} == {"A-c64-u8-b9-wide", "A-c64-seg_f16-b9-wide", "B-v5-seg_f32-b520-wide",
                                      "B-evd_mean-seg_f16-b520-wide"}


def test_route_scenes_are_fair():
    """Part D: each class of the 1,537-chunk frame is two blobs more than 300 chunks apart; the launch
    split's 17 classes all vote, 15 + 2 per launch, on well-conditioned checked images."""
    assert -(-607 * 648 // 256) == 1537
    for case in EC.part_d_route():
        label = EC.inputs(case)["label"]
        for c in range(case.ncls):
            assert np.diff(EC.occupied_chunks(label, c)).max() > 300
        assert all(r["tn"] >= 100 for r in EC.reference(case))
    sp, S = EC.split_scene(), EC.SPLIT
    assert sp["tn"].tolist() == [191 + c for c in range(17)]
    for c in range(17):
        assert int((sp["label"] == c + 1).sum()) == sp["tn"][c]
    per_launch = (2 ** 31 - 1) // (S["vn"] * -(-S["nh"] // 128) * S["H"] * S["W"])
    assert per_launch == 15 and S["ncls"] - per_launch == 2
    assert S["H"] * S["W"] * S["ncls"] * S["vn"] * 2 * 2 == 285_212_672          # the f16 field's bytes
    for i, r in sp["ref"].items():
        assert np.linalg.cond(np.asarray(r["ATA"], np.float64)).max() <= COND_MAX
        c = i                                                   # b = 1: the virtual image is the class
        assert np.all(r["lattice"] == (30.0, 10.0 + c))         # on a foreground pixel's centre
        assert np.all(r["far"][..., 0] == 40.0) and np.all(np.abs(r["far"][..., 1]) > 8e6)
        assert np.isfinite(r["hyp"]).all() and r["sets"] == ((1, 3) if i >= 15 else (5, 7))
        cls = restated(r["hyp"][..., 0], r["hyp"][..., 1])      # [nh, vn]: whole exact-only sets among fast ones
        for s_ in r["sets"]:
            assert np.all(cls[32 * s_:32 * s_ + 32] == EXACT)
        assert (cls == FAST).mean() > 0.9
    for s_ in S["nonfinite_sets"]:                              # image 1: neither class; image 16 votes there
        assert not np.isfinite(sp["hyp1"][32 * s_:32 * s_ + 32]).any()
        assert np.all(sp["ref"][16]["counts"][32 * s_:32 * s_ + 32].max(0) > 0)
    assert np.isfinite(sp["hyp1"]).mean() > 0.9
