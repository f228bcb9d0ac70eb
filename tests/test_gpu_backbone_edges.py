"""The backbone kernels (pvnet_amd/csrc/pvconv.hip) and PVNetInference at the
states tests/test_backbone.py leaves out.

A. k_conv3x3: a ragged pixel tile through the unsplit K loop, the 3-way and
   the K-forced 2-way split of the last round (uneven parts, the 1x1
   downsample step alone at a part's end), ``ldo > cout``, ``act == 0``, maps
   smaller than the dilation.  Every case derives the split the library takes
   from ``pv_conv3x3_workspace_bytes`` and the device's CU count and asserts
   that it is the state the case names before it runs.
B. The tile kernels (k_dec_conv, k_decoder_tail, k_conv64, k_stem) and the
   elementwise passes at maps of one tile, less than one tile and less than
   the decoder's 7 x 19 patch, batch 1 included.
C. PVNetInference: every route switch with the calls it implies counted,
   batches, frames down to a one-row stride-8 map, batch independence bit for
   bit, graph replay.

Kernel-level bounds are tests/fp16_bounds.py's (derived from the roundings,
any summation order); the network's are test_backbone.py's FP16_TOL and 2e-4
of the output scale, against our PVNet with the G4 weights on the CPU in f64.
"""
from __future__ import annotations

import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from pvnet_amd import _lib, network
from pvnet_amd.network import PVNet, PVNetInference
from tests import backbone_init as BI
from tests import fp16_bounds as B
from tests.golden_io import load
from tests.test_backbone import FP16_TOL

pytestmark = pytest.mark.gpu

CL = torch.channels_last
G = load("backbone_g4")


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _rnd(g, device, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(device, torch.float16)


def _mod(w: torch.Tensor, stride=1, d=1) -> torch.nn.Conv2d:
    """A bias-free Conv2d holding the fp16 weight w (3x3: padding = dilation = d)."""
    co, ci, k, _ = w.shape
    c = torch.nn.Conv2d(ci, co, k, stride, d if k == 3 else 0, d if k == 3 else 1, bias=False).to(w.device).half()
    with torch.no_grad():
        c.weight.copy_(w)
    return c


# ---------------------------------------------------------------- A. k_conv3x3 states
def _cus(device) -> int:
    return torch.cuda.get_device_properties(device).multi_processor_count


def _split_state(device, pixels: int, cout: int, ksteps: int):
    """(tiles run whole, tiles of the split last round, parts per split tile)
    as pv_conv3x3_ex_f16 takes them with a workspace: from the library's
    workspace size, bytes = 4096 + rem * S * CT * 256 * 4 (0: no split)."""
    ct = 256 if cout % 256 == 0 else 128
    ntiles = -(-pixels // 256) * (cout // ct)
    rem = ntiles % _cus(device)
    nbytes = int(_lib.load().pv_conv3x3_workspace_bytes(pixels, cout, ksteps))
    if nbytes == 0:
        return ntiles, 0, 1
    per = rem * ct * 256 * 4
    assert rem > 0 and nbytes > 4096 and (nbytes - 4096) % per == 0, (nbytes, rem, ct)
    return ntiles - rem, rem, (nbytes - 4096) // per


def _shape_for_tiles(ntiles: int):
    """(1, h, w), w odd, of exactly `ntiles` 256-pixel tiles, the last one partial."""
    for w in (37, 41):
        h = (ntiles - 1) * 256 // w + 1
        if -(-h * w // 256) == ntiles and (h * w) % 256:
            return 1, h, w
    raise AssertionError(f"no ragged shape of {ntiles} tiles")


def _conv_case(device, name, kind, n, hin, win, cin, cout, d, *, nsplit, whole=None, forced_unsplit=False, act="relu",
               res=False, rbias=False, cin2=0, s2=1, twice=False):
    """One pv_conv3x3_ex_f16 call through network.conv3x3 (kind "plain") or
    network.conv3x3_ex ("s2": stride 2; "cat": a second map's channels
    appended; "ds": a 1x1 convolution of a second map at stride s2 in the same
    accumulator) against B.conv64 with test_backbone.py's chain of bounds.
    Before the call: the split state must be `nsplit` parts (`whole`: with /
    without whole tiles beside the split round); `forced_unsplit`:
    network.CONV_SPLIT is off, so no workspace reaches the kernel.
    Returns (output, largest dev / bound)."""
    g = _gen(name)
    stride = 2 if kind == "s2" else 1
    h, w = (hin - 1) // stride + 1, (win - 1) // stride + 1
    ctot = cin + (cin2 if kind == "cat" else 0)
    k = 9 * ctot + (cin2 if kind == "ds" else 0)
    m = n * h * w
    x = _rnd(g, device, n, cin, hin, win).contiguous(memory_format=CL)
    nfull, rem, s = _split_state(device, m, cout, k // 64)
    if forced_unsplit:
        nfull, rem, s = nfull + rem, 0, 1
    print(f"{name}: {m} pixels, {nfull} whole tiles + {rem} in {s} parts of {k // 64} K-steps on {_cus(device)} CUs")
    if forced_unsplit:
        assert not network.CONV_SPLIT and network._conv_workspace(x, m, cout, k // 64) == (None, 0)
        assert m % 256, "the last pixel tile must be partial"
    else:
        assert network.CONV_SPLIT and s == nsplit, f"{name}: {s} parts, the case is about {nsplit}"
        assert whole is None or (nfull > 0) == whole, f"{name}: {nfull} whole tiles"
    wt = _rnd(g, device, cout, ctot, 3, 3, scale=1.0 / (3 * ctot ** 0.5))
    b = _rnd(g, device, cout, scale=0.5)
    r = _rnd(g, device, n, cout, h, w).contiguous(memory_format=CL) if res else None
    rb = _rnd(g, device, cout, scale=0.5) if rbias else None
    xm, x2, wd, bd = x, None, None, None
    if kind == "cat":
        x2 = _rnd(g, device, n, cin2, hin, win).contiguous(memory_format=CL)
        xm = torch.cat([x, x2], 1)
    elif kind == "ds":
        x2 = _rnd(g, device, n, cin2, s2 * (h - 1) + 1, s2 * (w - 1) + 1).contiguous(memory_format=CL)
        wd = _rnd(g, device, cout, cin2, 1, 1, scale=1.0 / cin2 ** 0.5)
        bd = _rnd(g, device, cout, scale=0.5)

    def call():
        c = _mod(wt, stride, d)
        if kind == "plain":
            return network.conv3x3(x, network.conv3x3_weight(c), b, d, act, res=r, rbias=rb)
        if kind == "s2":
            return network.conv3x3_ex(x, network.conv3x3_weight(c), b, d, stride=2, act=act)
        if kind == "cat":
            return network.conv3x3_ex(x, network.conv3x3_weight(c), b, d, act=act, x2=x2, mode2="cat")
        return network.conv3x3_ex(x, network.conv3x3_weight(c, _mod(wd, s2)), b, d, act=act, x2=x2, mode2="1x1",
                                  s2=s2, rbias=bd)

    with torch.no_grad():
        got = call()
        again = call() if twice else None
        torch.cuda.synchronize()
        assert got.shape == (n, cout, h, w) and got.is_contiguous(memory_format=CL)
        if twice:       # the parts are summed in part order, whichever arrives last
            assert torch.equal(got, again), f"{name}: two runs differ"
        conv = dict(stride=stride, padding=d, dilation=d)
        c64 = B.conv64(xm, wt, **conv)
        e = B.acc_bound(xm, wt, k, **conv)
        if kind == "ds":                                  # summed in the same accumulator, rounded once
            c64 = c64 + B.conv64(x2, wd, stride=s2)
            e = e + B.acc_bound(x2, wd, k, stride=s2)
        e = B.round_step(c64, e)                          # the convolution's fp16 output
        y64 = c64 + b.double().view(1, -1, 1, 1)
        e = B.round_step(y64, e)                          # + bias
        if kind == "ds":
            y64 = y64 + bd.double().view(1, -1, 1, 1)
            e = B.round_step(y64, e)                      # + the downsample's bias
        if res:
            r64 = r.double()
            if rbias:
                r64 = r64 + rb.double().view(1, -1, 1, 1)
                e = e + B.hulp(r64)                       # res + rbias
            y64 = y64 + r64
            e = B.round_step(y64, e)                      # + residual
        if act == "leaky":
            e = B.leaky_step(y64, e, 0.1)
            y64 = F.leaky_relu(y64, 0.1)
        elif act == "relu":
            y64 = torch.relu(y64)
    return got, B.check(got, y64, e, name)


@pytest.mark.parametrize("case", ["resb_128_128_d1", "relu_256_512_d4", "cat_256_128_d1", "ds2_64_128_d1"])
def test_conv3x3_unsplit_ragged_tile(case, device, monkeypatch):
    """(3, 13, 17) = 663 pixels, the third pixel tile with 151 rows, run whole
    through the unsplit K loop (CONV_SPLIT off): rows p >= M read as zeros and
    store nothing."""
    monkeypatch.setattr(network, "CONV_SPLIT", False)
    kind, cin, cout, d = case.split("_")[0], *[int(v) for v in case.split("_")[1:3]], int(case.split("_")[3][1:])
    kw = dict(nsplit=1, forced_unsplit=True)
    if kind == "resb":
        _conv_case(device, case, "plain", 3, 13, 17, cin, cout, d, res=True, rbias=True, **kw)
    elif kind == "relu":
        _conv_case(device, case, "plain", 3, 13, 17, cin, cout, d, **kw)
    elif kind == "cat":
        _conv_case(device, case, "cat", 3, 13, 17, cin, cout, d, act="leaky", cin2=128, **kw)
    else:
        _conv_case(device, case, "ds", 3, 13, 17, cout, cout, d, cin2=cin, s2=2, **kw)


def test_conv3x3_natural_unsplit_partial_tile(device):
    """CUs - CUs / 4 tiles: the last round is too full to split (S == 1 from
    conv_split itself), the last pixel tile partial."""
    cus = _cus(device)
    n, h, w = _shape_for_tiles(cus - cus // 4)
    assert (n * h * w) % 256
    _conv_case(device, "natural_s1", "plain", n, h, w, 128, 128, 1, nsplit=1, whole=True)


@pytest.mark.parametrize("kind", ["plain", "1x1"])
def test_conv3x3_three_way_split_beside_whole_tiles(kind, device):
    """CUs + CUs / 3 tiles of 128 couts: CUs whole tiles, then CUs / 3 tiles in
    3 parts, the last pixel tile partial.  18 K-steps split 6 / 6 / 6; with the
    1x1 downsample of 64 channels 19 K-steps split 0-6, 6-12, 12-19: uneven,
    the 1x1 step alone at the end of the last part.  Two runs are bit-equal."""
    cus = _cus(device)
    n, h, w = _shape_for_tiles(cus + cus // 3)
    if kind == "plain":
        _conv_case(device, "s3_plain", "plain", n, h, w, 128, 128, 1, nsplit=3, whole=True, twice=True)
    else:
        _conv_case(device, "s3_1x1", "ds", n, h, w, 128, 128, 1, cin2=64, nsplit=3, whole=True, twice=True)


@pytest.mark.parametrize("kind", ["s2_k9", "ds2_k10"])
def test_conv3x3_two_way_split_forced_by_k(kind, device):
    """cin 64: 9 K-steps (10 with a 1x1 of 64 channels), so conv_split's
    `while (ksteps / S < 4) --S` brings 4 parts down to 2 (0-4, 4-9: uneven;
    0-5, 5-10).  Stride 2 from an odd-sized input."""
    if kind == "s2_k9":
        _conv_case(device, kind, "s2", 2, 31, 41, 64, 128, 1, nsplit=2, whole=False, twice=True)
    else:
        _conv_case(device, kind, "ds", 2, 16, 21, 64, 128, 1, cin2=64, s2=2, nsplit=2, whole=False, twice=True)


@pytest.mark.parametrize("split", [True, False])
def test_conv3x3_ldo_wider_than_cout(split, device):
    """The entry point on an output of cout + 64 channels (ldo > cout, the
    torch.cat after fc on the fused_ds=False route): channels [:cout] within
    the bound, channels [cout:] bit-untouched (a sentinel pattern, compared as
    int16); 4-way split and unsplit."""
    n, h, w, cin, cout, d, extra = 3, 13, 17, 128, 128, 1, 64
    name = f"ldo_{'split' if split else 'unsplit'}"
    g = _gen(name)
    x = _rnd(g, device, n, cin, h, w).contiguous(memory_format=CL)
    wt = _rnd(g, device, cout, cin, 3, 3, scale=1.0 / (3 * cin ** 0.5))
    b = _rnd(g, device, cout, scale=0.5)
    wk = network.conv3x3_weight(_mod(wt, 1, d))
    nfull, rem, s = _split_state(device, n * h * w, cout, 9 * cin // 64)
    assert (nfull, rem, s) == (0, 3, 4), (nfull, rem, s)
    ws = None
    if split:
        ws = torch.zeros(int(_lib.load().pv_conv3x3_workspace_bytes(n * h * w, cout, 9 * cin // 64)), dtype=torch.uint8,
                         device=device)
    sent = torch.full((n, h, w, cout + extra), 0x5A5A, dtype=torch.int16, device=device)
    out = sent.view(torch.float16).permute(0, 3, 1, 2)            # [n, cout + extra, h, w] channels_last
    assert out.is_contiguous(memory_format=CL) and out.data_ptr() == sent.data_ptr()
    stream = torch.cuda.current_stream(device).cuda_stream
    _lib.check(_lib.load().pv_conv3x3_ex_f16(
        x.data_ptr(), h, w, 1, None, 0, 0, 0, 0, 0, wk.data_ptr(), b.data_ptr(), None, None, out.data_ptr(),
        cout + extra, n, h, w, cin, cout, d, 1, 0.1, None if ws is None else ws.data_ptr(),
        0 if ws is None else ws.numel(), stream), "pv_conv3x3_ex_f16")
    torch.cuda.synchronize()
    assert bool((sent[..., cout:] == 0x5A5A).all()), "channels past cout were written"
    with torch.no_grad():
        c64 = B.conv64(x, wt, padding=d, dilation=d)
        e = B.round_step(c64, B.acc_bound(x, wt, 9 * cin, padding=d, dilation=d))
        y64 = c64 + b.double().view(1, -1, 1, 1)
        e = B.round_step(y64, e)
    B.check(out[:, :cout], torch.relu(y64), e, name)
    if split:
        assert not ws[:4096].any(), "the arrival counters must be back at zero"


def test_conv3x3_extra_channels_bit_equal(device):
    """network.conv3x3(..., extra=64)[:, :cout] equals the extra=0 result bit for bit."""
    g = _gen("extra")
    n, h, w, cin, cout = 3, 13, 17, 128, 256
    x = _rnd(g, device, n, cin, h, w).contiguous(memory_format=CL)
    wk = network.conv3x3_weight(_mod(_rnd(g, device, cout, cin, 3, 3, scale=1.0 / (3 * cin ** 0.5)), 1, 2))
    b = _rnd(g, device, cout, scale=0.5)
    plain = network.conv3x3(x, wk, b, 2, "relu")
    wide = network.conv3x3(x, wk, b, 2, "relu", extra=64)
    torch.cuda.synchronize()
    assert wide.shape == (n, cout + 64, h, w) and wide.is_contiguous(memory_format=CL)
    assert torch.equal(wide[:, :cout], plain)


@pytest.mark.parametrize("res", [False, True])
def test_conv3x3_act_none(res, device):
    """act == 0: the sum (+ bias, + residual) stored as it is, negative values included."""
    got, _ = _conv_case(device, f"none_res{int(res)}", "plain", 3, 13, 17, 128, 128, 1, act="none", res=res, nsplit=4,
                        whole=False)
    assert bool((got < 0).any())


@pytest.mark.parametrize("case", ["2x3x5_d4_512", "1x1x1_d2_256", "2x1x9_d1_128", "2x7x1_d4_512", "ds1_2x3x5_d4",
                                  "s2_from_1x1", "s2_from_2x2"])
def test_conv3x3_degenerate_maps(case, device):
    """Maps smaller than the dilation (layer4's dilation 4 on a 3 x 5 map: all
    but the centre tap wholly or mostly out of range), one-pixel, one-row and
    one-column maps, and stride 2 down to one pixel."""
    if case == "2x3x5_d4_512":
        _conv_case(device, case, "plain", 2, 3, 5, 512, 512, 4, res=True, nsplit=4, whole=False)
    elif case == "1x1x1_d2_256":
        _conv_case(device, case, "plain", 1, 1, 1, 256, 256, 2, nsplit=4, whole=False)
    elif case == "2x1x9_d1_128":
        _conv_case(device, case, "plain", 2, 1, 9, 128, 128, 1, res=True, rbias=True, nsplit=4, whole=False)
    elif case == "2x7x1_d4_512":
        _conv_case(device, case, "plain", 2, 7, 1, 512, 512, 4, nsplit=4, whole=False)
    elif case == "ds1_2x3x5_d4":
        _conv_case(device, case, "ds", 2, 3, 5, 512, 512, 4, cin2=256, s2=1, nsplit=4, whole=False)
    elif case == "s2_from_1x1":
        _conv_case(device, case, "s2", 2, 1, 1, 64, 128, 1, nsplit=2, whole=False)
    else:
        _conv_case(device, case, "s2", 2, 2, 2, 64, 128, 1, nsplit=2, whole=False)


# ---------------------------------------------------------------- B. tile kernels at their smallest maps
# (h, w, n) of fm; the outputs are 2h x 2w: 4 x 4 (under the 7 x 19 patch and the 8 x 32 tile), 6 x 32 (one
# column tile exactly), 8 x 34 (one row tile exactly, a 2-column second tile), 10 x 4 (two row tiles, 4 columns)
SMALL_MAPS = [(2, 2, 1), (3, 16, 1), (4, 17, 3), (5, 2, 2)]


def _decoder_inputs(device, name, c1, c2, cmid, hw, wscale):
    g = _gen(name)
    h, w, n = hw
    fm = _rnd(g, device, n, c1, h, w, scale=2.0).contiguous(memory_format=CL)
    skip = _rnd(g, device, n, c2, 2 * h, 2 * w).contiguous(memory_format=CL)
    c = torch.nn.Conv2d(c1 + c2, cmid, 3, 1, 1).to(device)
    with torch.no_grad():
        c.weight.copy_(torch.randn(cmid, c1 + c2, 3, 3, generator=g) * wscale)
        c.bias.copy_(torch.randn(cmid, generator=g) * 0.5)
    return fm, skip, c.half(), g


@pytest.mark.parametrize("hw", SMALL_MAPS)
def test_decoder_conv4s_small_maps(hw, device):
    fm, skip, c, _ = _decoder_inputs(device, f"c4s{hw}", 128, 64, 64, hw, 0.04)
    with torch.no_grad():
        got = network.decoder_conv4s(fm, skip, network.decoder_conv4s_weights(c), 0.1)
    torch.cuda.synchronize()
    assert got.shape == (hw[2], 64, 2 * hw[0], 2 * hw[1]) and got.is_contiguous(memory_format=CL)
    B.check_decoder_fp64(got, fm, skip, c, 0.1, f"decoder conv4s {hw}")


@pytest.mark.parametrize("hw", SMALL_MAPS)
def test_decoder_conv2s_small_maps(hw, device):
    fm, skip, c, _ = _decoder_inputs(device, f"c2s{hw}", 64, 64, 32, hw, 0.05)
    with torch.no_grad():
        got = network.decoder_conv2s(fm, skip, network.decoder_conv2s_weights(c), 0.1)
    torch.cuda.synchronize()
    assert got.shape == (hw[2], 32, 2 * hw[0], 2 * hw[1]) and got.is_contiguous(memory_format=CL)
    B.check_decoder_fp64(got, fm, skip, c, 0.1, f"decoder conv2s {hw}")


@pytest.mark.parametrize("cout", [20, 44])
@pytest.mark.parametrize("hw", SMALL_MAPS)
def test_decoder_tail_small_maps(hw, cout, device):
    """pv_decoder_tail_f16 against the f64 reference; the split form
    (pv_decoder_tail_split_f16) bit-equal to the one-buffer form's slices."""
    fm, img, c0, g = _decoder_inputs(device, f"tail{hw}{cout}", 32, 3, 32, hw, 0.1)
    c1 = torch.nn.Conv2d(32, cout, 1).to(device)
    with torch.no_grad():
        c1.weight.copy_(torch.randn(cout, 32, 1, 1, generator=g) * 0.3)
        c1.bias.copy_(torch.randn(cout, generator=g))
    c1 = c1.half()
    wts = network.decoder_tail_weights(c0, c1)
    with torch.no_grad():
        got = network.decoder_tail(fm, img, wts, 0.1)
        seg, ver = network.decoder_tail(fm, img, wts, 0.1, split=True)
    torch.cuda.synchronize()
    h, w, n = hw
    assert got.shape == (n, cout, 2 * h, 2 * w) and got.is_contiguous(memory_format=CL)
    B.check_decoder_fp64(got, fm, img, c0, 0.1, f"decoder tail {hw} cout {cout}", head=(c1.weight, c1.bias))
    assert seg.shape == (n, 2, 2 * h, 2 * w) and ver.shape == (n, cout - 2, 2 * h, 2 * w)
    assert seg.is_contiguous(memory_format=CL) and ver.is_contiguous(memory_format=CL)
    assert torch.equal(seg, got[:, :2]) and torch.equal(ver, got[:, 2:])


@pytest.mark.parametrize("fn", ["decoder_conv4s", "decoder_conv2s", "decoder_tail"])
@pytest.mark.parametrize("hw", [(1, 5), (5, 1)])
def test_decoder_kernels_refuse_one_row_maps(fn, hw, device):
    """hin < 2 or win < 2: the decoder kernels return PV_EINVAL (no launch);
    PVNetInference.forward takes its upsample2x_cat + convolution form there."""
    c1, c2, cmid = {"decoder_conv4s": (128, 64, 64), "decoder_conv2s": (64, 64, 32), "decoder_tail": (32, 3, 32)}[fn]
    fm, skip, c, _ = _decoder_inputs(device, fn + str(hw), c1, c2, cmid, (*hw, 1), 0.05)
    with pytest.raises(_lib.PVError):
        if fn == "decoder_tail":
            c1m = torch.nn.Conv2d(32, 20, 1).to(device).half()
            network.decoder_tail(fm, skip, network.decoder_tail_weights(c, c1m), 0.1)
        else:
            getattr(network, fn)(fm, skip, getattr(network, fn + "_weights")(c), 0.1)


@pytest.mark.parametrize("case", ["1x1", "2x3", "8x32", "9x33", "8x32x3_res"])
def test_conv64_small_maps(case, device):
    """pv_conv64_f16 on one pixel, less than a tile, one 8 x 32 tile exactly and
    one row and column more (4 tiles), batch 1: fewer tiles than blocks."""
    dims = [int(v) for v in case.split("_")[0].split("x")]
    h, w, n = dims[0], dims[1], (dims[2] if len(dims) > 2 else 1)
    res = case.endswith("res")
    g = _gen("c64" + case)
    x = _rnd(g, device, n, 64, h, w).contiguous(memory_format=CL)
    r = _rnd(g, device, n, 64, h, w).contiguous(memory_format=CL) if res else None
    wt = _rnd(g, device, 64, 64, 3, 3, scale=1.0 / 24)
    b = _rnd(g, device, 64, scale=0.5)
    with torch.no_grad():
        got = network.conv64(x, network.conv64_weights(_mod(wt)), b, "relu", res=r)
        torch.cuda.synchronize()
        assert got.shape == x.shape and got.is_contiguous(memory_format=CL)
        c64 = B.conv64(x, wt, padding=1)
        e = B.round_step(c64, B.acc_bound(x, wt, 9 * 64, padding=1))
        y64 = c64 + b.double().view(1, -1, 1, 1)
        e = B.round_step(y64, e)
        if res:
            y64 = y64 + r.double()
            e = B.round_step(y64, e)
    B.check(got, torch.relu(y64), e, f"conv64 {case}")


@pytest.mark.parametrize("hw", [(2, 2), (4, 60), (4, 62), (16, 64), (18, 64)])
def test_stem_small_maps(hw, device):
    """pv_stem_conv_f16 / pv_stem_pool_f16 at x2s maps of 1 x 1, 2 x 30 (one
    pool-aligned strip exactly), 2 x 31, 8 x 32 (one row tile, two strips) and
    9 x 32, batch 1: x2s within the bound of the f64 convolution; the fused
    pass's x2s bit-equal to the conv-only pass's and its pool to max_pool2d."""
    h, w = hw
    g = _gen(f"stem{hw}")
    img = _rnd(g, device, 1, 3, h, w).contiguous(memory_format=CL)
    wt = _rnd(g, device, 64, 3, 7, 7, scale=0.1)
    b = _rnd(g, device, 64, scale=0.5)
    c = torch.nn.Conv2d(3, 64, 7, 2, 3).to(device).half()
    with torch.no_grad():
        c.weight.copy_(wt)
        c.bias.copy_(b)
        sw = network.stem_weights(c)
        x2s = network.stem_conv(img, sw)
        x2f, pool = network.stem_conv(img, sw, pool=True)
        torch.cuda.synchronize()
        assert x2s.shape == (1, 64, h // 2, w // 2) and x2s.is_contiguous(memory_format=CL)
        c64 = B.conv64(img, wt, stride=2, padding=3)
        e = B.round_step(c64, B.acc_bound(img, wt, 3 * 49, stride=2, padding=3))
        y64 = c64 + b.double().view(1, -1, 1, 1)
        e = B.round_step(y64, e)
    B.check(x2s, torch.relu(y64), e, f"stem conv {h}x{w}")
    assert torch.equal(x2f, x2s), "the fused pass's x2s"
    ref_pool = F.max_pool2d(x2s, 3, 2, 1)
    assert pool.shape == ref_pool.shape and pool.is_contiguous(memory_format=CL) and torch.equal(pool, ref_pool)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("hw", [(1, 1), (1, 2)])
def test_relu_maxpool_one_row(dtype, hw, device):
    """pv_relu_maxpool (both forms) on 1 x 1 and 1 x 2 maps: bit-equal to ATen's ops."""
    g = _gen(f"pool{hw}")
    y = (torch.randn(2, 64, *hw, generator=g) * 3).to(device, dtype).contiguous(memory_format=CL)
    b = torch.randn(64, generator=g).to(device, dtype)
    ref_x2s = torch.relu(y + b.view(1, -1, 1, 1))
    x2s, pool = network.relu_maxpool(y, b)
    only = network.maxpool(y)
    torch.cuda.synchronize()
    assert torch.equal(x2s, ref_x2s) and torch.equal(pool, F.max_pool2d(ref_x2s, 3, 2, 1))
    assert pool.shape == (2, 64, 1, 1) and torch.equal(only, F.max_pool2d(y, 3, 2, 1))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("c1,c2,cpad,h,w", [(32, 3, 40, 1, 6), (32, 3, 40, 5, 1), (128, 64, 192, 1, 5),
                                            (128, 64, 192, 5, 1), (64, 64, 128, 1, 1)])
def test_upsample2x_cat_one_row(c1, c2, cpad, h, w, dtype, device):
    """The fused upsample + cat at h = 1 and at w = 1 (align_corners scale 0
    along that axis) against ATen's, with test_upsample2x_cat_matches_torch's
    rule: fp16 one ulp, f32 a few roundings of the inputs' size; the skip and
    pad channels bit for bit."""
    g = _gen(f"up{c1}{h}{w}")
    fm = (torch.randn(2, c1, h, w, generator=g) * 4).to(device, dtype).contiguous(memory_format=CL)
    skip = (torch.randn(2, c2, 2 * h, 2 * w, generator=g) * 4).to(device, dtype).contiguous(memory_format=CL)
    out = network.upsample2x_cat(fm, skip, cpad)
    ref = torch.cat([torch.nn.UpsamplingBilinear2d(scale_factor=2)(fm), skip], 1)
    ref = torch.cat([ref, torch.zeros(2, cpad - ref.shape[1], 2 * h, 2 * w, dtype=dtype, device=device)], 1)
    assert out.shape == ref.shape and out.is_contiguous(memory_format=CL)
    d = (out.float() - ref.float()).abs()
    if dtype == torch.float16:
        ulp = torch.clamp(ref.float().abs(), min=2 ** -14) * 2 ** -10
    else:
        ulp = torch.full_like(d, 4 * 2 ** -24 * float(fm.abs().max()))
    assert bool((d <= ulp).all()), float((d / ulp).max())
    assert torch.equal(out[:, c1:], ref[:, c1:])


# ---------------------------------------------------------------- C. the inference form
@functools.lru_cache(maxsize=None)
def _pvnet(ver_dim=18, seg_dim=2) -> PVNet:
    """Our PVNet with the G4 seeded weights (f32, CPU, eval); never modified."""
    net = PVNet(ver_dim, seg_dim)
    sd = BI.seeded_state_dict(net.state_dict(), int(G["seed"]))
    if (ver_dim, seg_dim) == (18, 2):
        assert BI.weights_sha(sd) == str(G["weights_sha"]), "seeded G4 weights drifted"
    net.load_state_dict(sd, strict=True)
    return net.eval()


@functools.lru_cache(maxsize=None)
def _input(name: str) -> torch.Tensor:
    """Crops and flips of G4's 1x3x64x80 input, rounded to fp16 values: the
    fp16 and f32 forwards and the reference read the same numbers."""
    x = torch.from_numpy(G["x_small"]).half().float()
    if name == "1x64x80":
        return x
    if name in ("3x24x40", "2x24x40"):       # x8s 3 x 5: under layer4's dilation
        t = torch.cat([x[:, :, :24, :40], x[:, :, 40:, 40:].flip(3), x[:, :, 20:44, 10:50].flip(2)])
        return t if name[0] == "3" else t[:2].clone()
    if name == "2x16x16":
        return torch.cat([x[:, :, :16, :16], x[:, :, 48:, 64:].flip(2)])
    if name == "5x64x80":
        return torch.cat([x, x.flip(2), x.flip(3), x.flip(2).flip(3), torch.cat([x[..., 40:], x[..., :40]], 3)])
    if name == "1x8x40":                     # x8s 1 x 5
        return x[:, :, 28:36, 20:60].clone()
    if name == "1x40x8":                     # x8s 5 x 1
        return x[:, :, 12:52, 36:44].clone()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name: str, ver_dim=18, seg_dim=2) -> torch.Tensor:
    """cat([seg, ver], 1) of the f64 CPU forward of _pvnet on _input(name)."""
    import copy
    net = copy.deepcopy(_pvnet(ver_dim, seg_dim)).double()
    with torch.no_grad():
        seg, ver = net(_input(name).double())
    return torch.cat([seg, ver], 1)


def _inference(device, dtype, ver_dim=18, seg_dim=2) -> PVNetInference:
    return PVNetInference(_pvnet(ver_dim, seg_dim)).to(device=device, dtype=dtype).to(memory_format=CL)


def _forward(net, name, device, dtype):
    x = _input(name).to(device=device, dtype=dtype).contiguous(memory_format=CL)
    with torch.no_grad():
        seg, ver = net(x)
    torch.cuda.synchronize()
    return seg, ver


def _check_network(seg, ver, name, tol, what, ver_dim=18, seg_dim=2) -> float:
    """Every image of the batch within tol of its own reference's largest
    magnitude (an image alone is an input too, and batch independence makes
    its outputs those of the batch); returns the largest deviation of scale."""
    ref = _reference(name, ver_dim, seg_dim)
    got = torch.cat([seg, ver], 1).double().cpu()
    assert got.shape == ref.shape and seg.shape[1] == seg_dim, (got.shape, ref.shape)
    worst = 0.0
    for i in range(ref.shape[0]):
        sc = float(ref[i].abs().max())
        dev = float((got[i] - ref[i]).abs().max()) / sc
        print(f"{what} {name} image {i}: deviation {dev:.3e} of scale {sc:.2f} (tolerance {tol:.0e})")
        worst = max(worst, dev)
    assert worst <= tol, f"{what} {name}: {worst:.3e} of scale"
    return worst


COUNTED = ("conv3x3", "conv3x3_ex", "conv64", "stem_conv", "decoder_conv4s", "decoder_conv2s", "decoder_tail", "head",
           "conv_epilogue", "upsample2x_cat")


def _count_calls(monkeypatch):
    """network's kernel wrappers replaced by counting ones: name -> the keyword
    arguments of each call; "_ws": the workspaces _conv_workspace handed out."""
    calls = {n: [] for n in COUNTED}
    calls["_ws"] = []
    for n in COUNTED:
        def wrap(*a, _fn=getattr(network, n), _n=n, **k):
            calls[_n].append(k)
            return _fn(*a, **k)
        monkeypatch.setattr(network, n, wrap)

    def ws(*a, _fn=network._conv_workspace, **k):
        r = _fn(*a, **k)
        calls["_ws"].append(r)
        return r
    monkeypatch.setattr(network, "_conv_workspace", ws)
    return calls


# The calls PVNetInference.forward makes in fp16 on PVNet(18, 2), from the code.  Default route: the stem; layer1 =
# 4 conv64; layer2 = its stride-2 conv1 (conv3x3_ex, no second input), block 0's conv2 + downsample (conv3x3_ex
# "1x1"), block 1 = 2 conv3x3; layer3 and layer4 = conv1 (conv3x3), conv2 + downsample ("1x1"), 2 conv3x3 each; fc
# (conv3x3); conv8s over [xfc, x8s] (conv3x3_ex "cat"); the three decoder kernels.
DEFAULT_CALLS = dict(conv3x3=9, conv3x3_ex=5, conv64=4, stem_conv=1, decoder_conv4s=1, decoder_conv2s=1,
                     decoder_tail=1, head=0, conv_epilogue=0, upsample2x_cat=0)
ROUTES = {
    "default": dict(DEFAULT_CALLS),
    # the three downsamples as MIOpen convolutions, their sums read as residuals (conv3x3 with res + rbias); fc
    # writes into a 256 + 128 channel map (extra = 128) and conv8s is a plain conv3x3 over it: 9 + 3 + 1
    "fused_ds_off": dict(DEFAULT_CALLS, conv3x3=13, conv3x3_ex=1),
    # every convolution on MIOpen with one epilogue pass: 16 in the blocks, fc (writing the cat), conv8s, conv4s,
    # conv2s; the stem through pv_relu_maxpool; the tail kernel does not depend on fused_conv
    "fused_conv_off": dict(conv3x3=0, conv3x3_ex=0, conv64=0, stem_conv=0, decoder_conv4s=0, decoder_conv2s=0,
                           decoder_tail=1, head=0, conv_epilogue=20, upsample2x_cat=2),
    "tail_split_off": dict(DEFAULT_CALLS),
    "conv_split_off": dict(DEFAULT_CALLS),
    # PVNet(16, 3): 19 outputs, neither of pv_decoder_tail_f16's / pv_head_f16's heads: convraw's modules
    "head_16_3": dict(DEFAULT_CALLS, decoder_tail=0, upsample2x_cat=1),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_inference_route_matrix(route, device, monkeypatch):
    """Each switch of the fp16 inference form at 1x3x64x80: the outputs within
    FP16_TOL of the f64 reference, and the kernel wrappers called as that
    route's code implies -- a route that ran the default path would fail its
    counts (or, for the two module switches, the arguments they change)."""
    vd, sd = (16, 3) if route == "head_16_3" else (18, 2)
    net = _inference(device, torch.float16, vd, sd)
    if route == "fused_ds_off":
        net.fused_ds = False
    elif route == "fused_conv_off":
        net.fused_conv = False
    elif route == "tail_split_off":
        monkeypatch.setattr(network, "TAIL_SPLIT", False)
    elif route == "conv_split_off":
        monkeypatch.setattr(network, "CONV_SPLIT", False)
    calls = _count_calls(monkeypatch)
    seg, ver = _forward(net, "1x64x80", device, torch.float16)
    counts = {n: len(calls[n]) for n in COUNTED}
    print(f"route {route}: {counts}")
    assert counts == ROUTES[route]
    modes = sorted(k.get("mode2", "none") for k in calls["conv3x3_ex"])
    extras = [k["extra"] for k in calls["conv3x3"] if k.get("extra", 0) > 0]
    splits = [bool(k.get("split", False)) for k in calls["decoder_tail"]]
    if route == "fused_ds_off":
        assert modes == ["none"] and extras == [128]
        assert sum(k.get("rbias") is not None for k in calls["conv3x3"]) == 3
    elif route == "fused_conv_off":
        assert calls["_ws"] == [] and splits == [True]
    else:
        assert modes == ["1x1", "1x1", "1x1", "cat", "none"] and extras == []
    if route == "head_16_3":
        assert net.fused_tail is False and splits == []
    elif route != "fused_conv_off":
        assert splits == [route != "tail_split_off"]
    if route not in ("fused_conv_off",):
        assert len(calls["_ws"]) == counts["conv3x3"] + counts["conv3x3_ex"]
        handed = [p is not None for p, _ in calls["_ws"]]
        assert not any(handed) if route == "conv_split_off" else any(handed)
    _check_network(seg, ver, "1x64x80", FP16_TOL, f"route {route} fp16", vd, sd)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("name", ["3x24x40", "2x16x16", "5x64x80"])
def test_inference_batches_and_small_frames(name, dtype, device):
    """Batches of 2, 3 and 5 and frames whose stride-8 map is 3 x 5 (under
    layer4's dilation) and 2 x 2, default route: every image within tolerance
    of the f64 reference (fp16 FP16_TOL, f32 2e-4 of scale)."""
    net = _inference(device, dtype)
    seg, ver = _forward(net, name, device, dtype)
    _check_network(seg, ver, name, FP16_TOL if dtype == torch.float16 else 2e-4, f"inference form {dtype}")


@pytest.mark.parametrize("name", ["3x24x40", "5x64x80"])
def test_inference_batch_independence(name, device, monkeypatch):
    """With the split off, image i of a batch comes out bit-equal to image i
    run alone: unsplit k_conv3x3 sums each output pixel in one fixed K order
    wherever its pixel tile lies, and the tile kernels tile per image."""
    monkeypatch.setattr(network, "CONV_SPLIT", False)
    net = _inference(device, torch.float16)
    x = _input(name).to(device=device, dtype=torch.float16).contiguous(memory_format=CL)
    with torch.no_grad():
        seg, ver = net(x)
        for i in range(x.shape[0]):
            s1, v1 = net(x[i:i + 1].contiguous(memory_format=CL))
            torch.cuda.synchronize()
            assert torch.equal(s1[0], seg[i]) and torch.equal(v1[0], ver[i]), f"{name}: image {i} depends on its batch"


def test_inference_graph_replay_bit_equal(device):
    """The default fp16 forward at 2x3x24x40 captured on a side stream after
    one warm-up call: the replay is bit-equal to the eager result."""
    net = _inference(device, torch.float16)
    x = _input("2x24x40").to(device=device, dtype=torch.float16).contiguous(memory_format=CL)
    network.clear_conv_workspaces()
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.stream(s):
        eseg, ever = net(x)                                  # warm-up: the kernels' weight layouts are made here
        with torch.cuda.graph(graph, stream=s):
            gseg, gver = net(x)
    s.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gseg, eseg) and torch.equal(gver, ever)
    _check_network(gseg, gver, "2x24x40", FP16_TOL, "graph replay fp16")
    network.clear_conv_workspaces()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("name", ["1x8x40", "1x40x8"])
def test_inference_one_row_and_one_column_maps(name, dtype, device, monkeypatch):
    """An 8 x W / H x 8 frame: the stride-8 map has one row / column, which
    pv_decoder_conv4s_f16 refuses; forward takes upsample2x_cat + the
    convolution for that step and the fused kernels from 2 x 2 on."""
    net = _inference(device, dtype)
    calls = _count_calls(monkeypatch)
    seg, ver = _forward(net, name, device, dtype)
    if dtype == torch.float16:
        got = {n: len(calls[n]) for n in ("decoder_conv4s", "decoder_conv2s", "decoder_tail", "upsample2x_cat")}
        assert got == dict(decoder_conv4s=0, decoder_conv2s=1, decoder_tail=1, upsample2x_cat=1), got
    _check_network(seg, ver, name, FP16_TOL if dtype == torch.float16 else 2e-4, f"inference form {dtype}")
