"""Every voting entry on every input kind, and the multi-object edge states: the cases of
tests/entry_cases.py (proven fair on the CPU by tests/test_entry_cases.py) through the C ABI.

``run(case)`` builds the descriptor with ransac_voting_gpu._desc / _desc_multi and the parameters with
_params, calls the C entry through pvnet_amd._lib with an explicit VotingWorkspace and returns the
outputs and the pv_v3_diag arrays per virtual image bv = bi * ncls + c.  The EVD entries take no diag:
their tn, hypotheses and counts are read from the workspace (``workspace_views`` restates carve's
layout from both ends of pv_v3_workspace_size's total; the v3 / v5 calls require it equal to their diag).

Every case: tn, hypothesis bits, counts, winners and v5 confidence bits equal the oracle's; the refine
sums, keypoints and the EVD mean and covariance are within the suite's tolerances; a skipped class
gives exact zeros.

  A  label reading: every class count that ends the argmax's groups of four planes differently, 64
     classes, the wide label counter; labels 2 / 256 / 257 are no class of a one-class call
  B  logits into v5 and both EVD entries (single object), the wide k_fg_count on logits
  C  multi-object v5, EVD top-k and EVD-with-mean
  D  k_hyp_gen's class words for virtual images; a vote-launch cut between two classes of one image
  E  the field as a view inside a larger allocation, and ending on its last element
  F  the pairwise table; seeded rows equal the injected restated draws bit for bit
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from pvnet_amd import _lib
from tests import entry_cases as EC
from tests.test_hyp_class import EXACT, FAST, restated

pytestmark = pytest.mark.gpu

KP_TOL = 1e-2          # tests/test_gpu_parity.py
COV_RTOL = 1e-4
F32 = np.float32


@pytest.fixture(scope="module")
def rvg():
    from pvnet_amd import ransac_voting_gpu
    return ransac_voting_gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def cu(x, dev):
    return torch.from_numpy(np.array(x, order="C")).to(dev)    # a copy: the shared inputs stay read-only


def workspace_views(buf, total, bv, H, W, vn, nh):
    """(hypcls [bv,vn,nset,2] u32, counts [bv,vn,nh] i32, tn [bv] i32, hyp [bv,nh,vn,2] f32) of a
    workspace: the zeroed block's first two arrays from its start, the rest from its end (every array
    after the zeroed block starts on a multiple of 256 bytes)."""
    def a256(n):
        return -(-n // 256) * 256
    P = H * W
    nblk = -(-P // 256)
    nset = 4 * (-(-nh // 128))
    ncls_words = -(-(2 * bv * vn * nset) // 4) * 4
    tail = [4 * bv, 4 * bv, 4 * bv * nblk, 4 * bv * (-(-nblk // 8)), 32 * bv * nblk, 32 * bv * nblk, 16 * bv * vn * P,
            8 * bv * nh * vn, 8 * bv * nh * vn]                 # tn fgtot blkcnt grpcnt fgbits keptbits pex hyp hypv
    tn_off = total - sum(a256(n) for n in tail)
    hyp_off = total - 2 * a256(tail[-1])
    assert tn_off >= 4 * (ncls_words + bv * vn * nh) and tn_off % 256 == 0
    head = buf[:4 * (ncls_words + bv * vn * nh)].cpu().numpy()
    words = head.view(np.uint32)[:2 * bv * vn * nset].reshape(bv, vn, nset, 2)
    counts = head.view(np.int32)[ncls_words:].reshape(bv, vn, nh)
    tn = buf[tn_off:tn_off + 4 * bv].cpu().numpy().view(np.int32)
    hyp = buf[hyp_off:hyp_off + 8 * bv * nh * vn].cpu().numpy().view(F32).reshape(bv, nh, vn, 2)
    return words, counts, tn, hyp


def class_words(hyp, nh):
    """hyp [nh,vn,2] -> uint32 [vn,nset,2]: per 32 hypotheses of a keypoint the ballot of the fast
    and of the exact-only ones (hyp_class restated, tests/test_hyp_class.py), as Workspace::hypcls."""
    cls = restated(hyp[..., 0], hyp[..., 1])                    # [nh, vn]
    nset = 4 * (-(-nh // 128))
    out = np.zeros((hyp.shape[1], nset, 2), np.uint32)
    for k, bit in ((0, FAST), (1, EXACT)):
        on = np.zeros((nset * 32, hyp.shape[1]), np.uint64)
        on[:nh] = (cls & bit) != 0
        out[:, :, k] = (on.reshape(nset, 32, -1) << np.arange(32, dtype=np.uint64)[None, :, None]).sum(1).T
    return out


def device_inputs(case, device, place=None):
    inp = EC.inputs(case)
    mask, _ = EC.mask_tensor(case.kind, inp["mask"], device, place)
    field, owner = EC.field_tensor(case.field, inp["field"], device, place)
    return inp, mask, field, owner


class TorchBuffers:
    """run()'s default allocator: inputs copied to the device, outputs from torch.empty / torch.full, the
    workspace a fresh VotingWorkspace's buffer filled with 0xA5.  Another allocator (the guarded buffers of
    tests/test_gpu_memory_contract.py) has the same five methods."""

    def __init__(self, device, rvg):
        self.device, self.ws = device, rvg.VotingWorkspace()

    def inp(self, a):
        return cu(a, self.device)

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def full(self, shape, value, dtype):
        return torch.full(shape, value, dtype=dtype, device=self.device)

    def workspace(self, nbytes):
        buf = self.ws.get(self.device, nbytes)
        buf.fill_(0xA5)                                         # nothing the call reads is its own leftover
        return buf

    def done(self):
        self.ws.done(self.device)


def run(case, device, rvg, draws="inject", alloc=None):
    """The case through its C entry.  ``draws``: "inject" hands the case's pairs and keep mask in,
    "seed" leaves both to the call's RNG.  ``alloc``: where the buffers come from (TorchBuffers).
    -> dict of numpy arrays with leading [bv]."""
    alloc = alloc or TorchBuffers(device, rvg)
    inp, mask, field, _ = device_inputs(case, device, alloc.inp)
    seg = case.kind in EC.SEG
    d = rvg._desc(mask, field, seg=seg) if case.ncls == 0 else rvg._desc_multi(mask, field, case.ncls, seg=seg)
    assert (d.b, d.H, d.W, d.vn, d.ncls) == (case.b, case.H, case.W, case.vn, case.ncls)
    bv, vn, nh = case.bv, case.vn, case.nh
    inject = draws == "inject"
    idxs = alloc.inp(inp["idxs"]) if inject else None
    keep = alloc.inp(inp["keep"]) if inject and inp["keep"] is not None else None
    evd = case.entry.startswith("evd")
    rhn = case.rounds[0]
    prm = rvg._params(rhn, case.thresh, 0.99, 20 if case.entry == "v5" else 100, inp["min_num"], inp["max_num"], case.seed,
                      idxs, keep, min_hyp_num=nh if evd else 0, topk=case.topk if case.entry == "evd_topk" else 0)
    L = _lib.load()
    nbytes = L.pv_v3_workspace_size(bv, case.H, case.W, vn, nh)
    buf = alloc.workspace(nbytes)
    stream = torch.cuda.current_stream(device).cuda_stream
    f32, i32 = torch.float32, torch.int32
    out = {}
    with torch.cuda.device(device):
        try:
            if not evd:
                dt = dict(hyp=alloc.empty((bv, nh, vn, 2), f32), counts=alloc.empty((bv, vn, nh), i32),
                          win_idx=alloc.empty((bv, vn), i32), win_ratio=alloc.empty((bv, vn), f32),
                          tn=alloc.empty((bv,), i32), iters=alloc.empty((bv,), i32), ata=alloc.empty((bv, vn, 2, 2), f32),
                          atb=alloc.empty((bv, vn, 2), f32))
                diag = _lib.V3Diag(**{k: v.data_ptr() for k, v in dt.items()})
                kp = alloc.full((bv, vn, 2), np.nan, f32)
                if case.entry == "v3":
                    code = L.pv_ransac_voting_v3(ctypes.byref(d), ctypes.byref(prm), kp.data_ptr(), buf.data_ptr(), nbytes,
                                                 ctypes.byref(diag), stream)
                else:
                    conf = alloc.full((bv, vn), np.nan, f32)
                    code = L.pv_ransac_voting_v5(ctypes.byref(d), ctypes.byref(prm), 0.999, kp.data_ptr(), conf.data_ptr(),
                                                 buf.data_ptr(), nbytes, ctypes.byref(diag), stream)
                    out["conf"] = conf
                out.update(dt, kp=kp)
            else:
                cov = alloc.full((bv, vn, 2, 2), np.nan, f32)
                if case.entry == "evd_mean":
                    mean = alloc.inp(inp["mean"])
                    code = L.pv_estimate_voting_distribution_with_mean(ctypes.byref(d), ctypes.byref(prm), mean.data_ptr(),
                                                                       cov.data_ptr(), buf.data_ptr(), nbytes, stream)
                else:
                    mean = alloc.full((bv, vn, 2), np.nan, f32)
                    code = L.pv_estimate_voting_distribution(ctypes.byref(d), ctypes.byref(prm), mean.data_ptr(),
                                                             cov.data_ptr(), buf.data_ptr(), nbytes, stream)
                out.update(mean=mean, cov=cov)
        finally:
            alloc.done()
    _lib.check(code, case.name)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    words, counts, tn, hyp = workspace_views(buf, nbytes, bv, case.H, case.W, vn, nh)
    out["words"] = words
    if evd:
        out.update(counts=counts, tn=tn, hyp=hyp)
    else:                                                       # the diag's copies are the workspace's
        np.testing.assert_array_equal(out["tn"], tn)
        np.testing.assert_array_equal(out["counts"], counts)
    return out


def check(case, got, ref):
    """The device's outputs against the oracle's, virtual image by virtual image."""
    assert got["tn"].tolist() == [r["tn"] for r in ref]
    evd = case.entry.startswith("evd")
    for i, r in enumerate(ref):
        at = f"{case.name} virtual image {i}"
        if r["tn"] > 0:
            np.testing.assert_array_equal(bits(got["hyp"][i]), bits(r["hyp"]), err_msg=at + " hyp")
            np.testing.assert_array_equal(got["counts"][i].T, r["counts"], err_msg=at + " counts")
        if evd:
            np.testing.assert_allclose(got["cov"][i], r["cov"], rtol=COV_RTOL, atol=1e-4 * np.abs(r["cov"]).max(),
                                       err_msg=at + " cov")
            if case.entry == "evd_topk":
                np.testing.assert_allclose(got["mean"][i], r["mean"], atol=1e-3, rtol=1e-5, err_msg=at + " mean")
            else:
                np.testing.assert_array_equal(bits(got["mean"][i]), bits(r["mean"]))     # the input, untouched
            continue
        if r["tn"] == 0:                                        # a skipped class: exact zeros
            assert not bits(got["kp"][i]).any(), at
            if case.entry == "v5":
                assert not bits(got["conf"][i]).any(), at
            continue
        np.testing.assert_array_equal(got["win_idx"][i], r["win_idx"], err_msg=at + " win_idx")
        np.testing.assert_allclose(got["ata"][i], r["ATA"], rtol=1e-6, atol=1e-7 * np.abs(r["ATA"]).max(), err_msg=at)
        np.testing.assert_allclose(got["atb"][i], r["ATb"], rtol=1e-6, atol=1e-7 * np.abs(r["ATb"]).max(), err_msg=at)
        np.testing.assert_allclose(got["kp"][i], r["kp"], atol=KP_TOL, rtol=0, err_msg=at + " kp")
        if case.entry == "v5":
            np.testing.assert_array_equal(bits(got["conf"][i]), bits(r["conf"]), err_msg=at + " conf")
    assert not any(np.isnan(got["hyp"][i]).any() for i, r in enumerate(ref) if r["tn"] > 0)


def ids(cases):
    return [c.name for c in cases]


# ---------------------------------------------------------------- A. label reading
@pytest.mark.parametrize("case", EC.part_a(), ids=ids(EC.part_a()))
def test_label_reading(case, device, rvg):
    """Label maps and logits of 1 to 64 classes (2 to 65 planes: every way the argmax's groups of
    four planes can end), classes in every fill state, a downsampled one by an injected keep mask."""
    got = run(case, device, rvg)
    check(case, got, EC.reference(case))
    if case.ncls == 1 and case.kind not in EC.SEG:
        # labels 2, 256, 257 ... are no foreground of the one-class call; the same map through the
        # single-object v3 (mask.byte() != 0) counts all whose low byte is set
        inp, mask, field, _ = device_inputs(case, device)
        lab = inp["label"]
        assert {2, 255} <= set(lab.reshape(-1).tolist()) and (case.kind == "u8" or {256, 257} <= set(lab.reshape(-1).tolist()))
        diag = {}
        rvg.ransac_voting_layer_v3(mask, field, case.nh, min_num=inp["min_num"], _seed=1, _diag=diag)
        single = diag["tn"].cpu().numpy()
        want = np.array([int(O.fg_mask_v3(m).sum()) for m in inp["mask"]])
        np.testing.assert_array_equal(single, want)
        own = (lab == 1).reshape(case.b, -1).sum(1)
        assert np.all(want > own) and np.all(got["tn"] <= own)
        np.testing.assert_array_equal(got["tn"][inp["fgn"] <= inp["max_num"]],
                                      np.where(own < inp["min_num"], 0, own)[inp["fgn"] <= inp["max_num"]])


# ---------------------------------------------------------------- B, C, E
@pytest.mark.parametrize("case", EC.part_b(), ids=ids(EC.part_b()))
def test_logits_into_v5_and_evd(case, device, rvg):
    """Single-object logits through the entries that have no *_from_network layer; image 1 is below
    min_num; 520 images reach the wide foreground count."""
    check(case, run(case, device, rvg), EC.reference(case))


@pytest.mark.parametrize("case", EC.part_c(), ids=ids(EC.part_c()))
def test_multi_object_v5_and_evd(case, device, rvg):
    """conf, mean and cov indexed by the virtual image, from an int32 label view and f16 logits."""
    check(case, run(case, device, rvg), EC.reference(case))


@pytest.mark.parametrize("case", EC.part_e(), ids=ids(EC.part_e()))
def test_field_inside_a_larger_allocation(case, device, rvg):
    """The class-shifted buffer descriptor of a field surrounded by NaNs, or ending with its allocation."""
    _, _, field, owner = device_inputs(case, device)
    assert bool(torch.isnan(owner).any()) and not bool(torch.isnan(field).any())
    got = run(case, device, rvg)
    check(case, got, EC.reference(case))
    voted = got["tn"] > 0
    assert voted.any() and np.isfinite(got["hyp"][voted]).all() and np.isfinite(got["kp"]).all()


# ---------------------------------------------------------------- D. routes
@pytest.mark.parametrize("case", EC.part_d_route(), ids=ids(EC.part_d_route()))
def test_hyp_gen_route_virtual_images(case, device, rvg):
    """1,537 chunks: one k_hyp_gen launch makes the hypotheses and class words of both virtual images."""
    assert _lib.load().pv_v3_kernel_launches(case.bv, case.H, case.W, case.vn, case.nh) == 5
    got = run(case, device, rvg)
    check(case, got, EC.reference(case))
    for i in range(case.bv):
        np.testing.assert_array_equal(got["words"][i], class_words(got["hyp"][i], case.nh), err_msg=f"class {i}")
    assert got["words"].any()


def test_vote_launch_cut_between_classes(device, rvg):
    """One image, 17 classes of 64 keypoints, nh = 4096: the vote runs as 15 + 2 virtual images.
    All 17 tn; virtual images 0, 14, 15 and 16 against the oracle's hypotheses and counts, whole sets
    of lattice and far hypotheses among them at other sets after the cut than before it, and their
    class words.  Virtual image 1 holds two sets of non-finite hypotheses (an f16 infinity in the
    field): virtual image 16, second of its launch, has ordinary ones there, which a launch that
    read the first launch's words would not vote."""
    S, sp = EC.SPLIT, EC.split_scene()
    ncls, vn, H, W, nh = (S[k] for k in ("ncls", "vn", "H", "W", "nh"))
    L = _lib.load()
    assert L.pv_v3_kernel_launches(ncls, H, W, vn, nh) == 2 + 0 + 2 + 1
    gen = torch.Generator(device=device).manual_seed(4096)      # the same noise off the classes' pixels in every run
    field = torch.randn((1, H, W, ncls * vn, 2), dtype=torch.float16, device=device, generator=gen)
    assert field.numel() * 2 == 285_212_672
    for c, (rows, cols, direct) in enumerate(sp["pix"]):
        field[0, cu(rows, device), cu(cols, device), c * vn:(c + 1) * vn] = cu(direct, device)
    label = cu(sp["label"], device)
    d = rvg._desc_multi(label, field, ncls)
    idxs = cu(sp["idxs"], device)
    prm = rvg._params(nh, 0.99, min_num=100, max_num=30000, seed=1, idxs=idxs)
    nbytes = L.pv_v3_workspace_size(ncls, H, W, vn, nh)
    ws = rvg.VotingWorkspace()
    buf = ws.get(device, nbytes)
    dt = dict(hyp=torch.empty((ncls, nh, vn, 2), dtype=torch.float32, device=device),
              counts=torch.empty((ncls, vn, nh), dtype=torch.int32, device=device),
              tn=torch.empty(ncls, dtype=torch.int32, device=device))
    diag = _lib.V3Diag(**{k: v.data_ptr() for k, v in dt.items()})
    kp = torch.empty((ncls, vn, 2), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        try:
            code = L.pv_ransac_voting_v3(ctypes.byref(d), ctypes.byref(prm), kp.data_ptr(), buf.data_ptr(), nbytes,
                                         ctypes.byref(diag), torch.cuda.current_stream(device).cuda_stream)
        finally:
            ws.done(device)
    _lib.check(code, "launch split")
    np.testing.assert_array_equal(dt["tn"].cpu().numpy(), sp["tn"])
    words = workspace_views(buf, nbytes, ncls, H, W, vn, nh)[0]
    for i in S["checked"]:
        r = sp["ref"][i]
        np.testing.assert_array_equal(bits(dt["hyp"][i].cpu().numpy()), bits(r["hyp"]), err_msg=f"class {i}")
        np.testing.assert_array_equal(words[i], class_words(r["hyp"], nh), err_msg=f"class {i}")
        for s_ in r["sets"]:
            assert not words[i, :, s_, 0].any() and np.all(words[i, :, s_, 1] == 0xffffffff)
        np.testing.assert_array_equal(dt["counts"][i].cpu().numpy().T, r["counts"], err_msg=f"class {i}")
    assert bool(torch.isfinite(kp[list(S["checked"])]).all())
    w1 = words[1][:, list(S["nonfinite_sets"])]                 # image 1's non-finite sets: of neither class
    assert not w1.any() and not dt["counts"][1].cpu().numpy().reshape(vn, -1, 32)[:, list(S["nonfinite_sets"])].any()


# ---------------------------------------------------------------- F. the table
TABLE_CASES = EC.table_cases()


@pytest.mark.parametrize("case", TABLE_CASES, ids=ids(TABLE_CASES))
def test_table_row(case, device, rvg):
    """One row of the pairwise table against the oracle."""
    got = run(case, device, rvg)
    if case.ds == "seed":
        # the call that draws its own pairs and keep decisions against the one handed
        # tests/front_ref.py's restatement of them over the virtual images
        seeded = run(case, device, rvg, draws="seed")
        voted = got["tn"] > 0
        assert seeded["tn"].tolist() == got["tn"].tolist()
        for k in got:
            if k in ("hyp", "counts", "win_idx", "win_ratio", "iters", "ata", "atb", "words"):
                np.testing.assert_array_equal(seeded[k][voted].view(np.uint32), got[k][voted].view(np.uint32), err_msg=k)
            elif k != "tn":
                np.testing.assert_array_equal(bits(seeded[k]), bits(got[k]), err_msg=k)
    check(case, got, EC.reference(case))


def layer_call(case, device, rvg):
    """The public layer of a combination (EC.layer_of) -> its outputs as run()'s."""
    name = EC.layer_of(case)
    fn = getattr(rvg, name)
    inp, mask, field, owner = device_inputs(case, device)
    multi, bv, vn = case.ncls > 0, case.bv, case.vn
    lead = (case.b, case.ncls) if multi else (case.b,)
    vertex = owner if name.endswith("from_network") else field   # the NCHW vertex_pred itself
    cls = (case.ncls,) if multi else ()
    kw = dict(inlier_thresh=case.thresh, min_num=inp["min_num"], max_num=inp["max_num"], _seed=case.seed,
              _idxs=cu(inp["idxs"], device).reshape(*lead, case.nh, vn, 2),
              _keep=None if inp["keep"] is None else cu(inp["keep"], device).reshape(*lead, case.H, case.W))
    if case.entry in ("v3", "v5"):
        diag = {}
        res = fn(mask, vertex, *cls, case.nh, _diag=diag, **kw)
        out = dict(kp=res[0], conf=res[1]) if case.entry == "v5" else dict(kp=res)
        out.update({k: diag[k] for k in ("hyp", "counts", "win_idx", "tn", "ata", "atb")})
    else:
        kw.update(round_hyp_num=case.rounds[0], min_hyp_num=case.nh)
        if case.entry == "evd_topk":
            m, cov = fn(mask, field, topk=case.topk, **kw)
        else:
            m, cov = fn(mask, field, cu(inp["mean"], device).reshape(*lead, vn, 2), *cls, **kw)
        out = dict(mean=m, cov=cov)
    return {k: v.cpu().numpy().reshape(bv, *v.shape[len(lead):]) for k, v in out.items()}


LAYER_CASES = [c for c in EC.all_cases() if EC.layer_of(c)]


@pytest.mark.parametrize("case", LAYER_CASES, ids=ids(LAYER_CASES))
def test_public_layer_gives_the_same_bits(case, device, rvg):
    """Where a Python layer exists for the combination, it gives what the C entry gave ``run``
    (which the case's own part compares with the oracle; part_layers' cases are compared here)."""
    got = run(case, device, rvg)
    lay = layer_call(case, device, rvg)
    voted = got["tn"] > 0
    for k, v in lay.items():
        a, g = (v[voted], got[k][voted]) if k in ("hyp", "counts", "win_idx", "ata", "atb") else (v, got[k])
        np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(g).view(np.uint32),
                                      err_msg=f"{case.name}: {k}")
    if case in EC.part_layers():
        check(case, got, EC.reference(case))
