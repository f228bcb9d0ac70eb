"""CPU-side checks of the multi-object entry (no GPU needed): the descriptor's
class count, its validation before any launch, and the argument checks of the
``_multi`` Python layers."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from pvnet_amd import build, _lib
    build.build()
    return _lib.load()


def desc(**kw):
    from pvnet_amd import _lib
    return _lib.ImageDesc(mask=1, vertex=1, b=1, H=4, W=4, vn=9, mask_kind=0, **kw)


def test_image_desc_has_ncls_last():
    from pvnet_amd import _lib
    names = [f[0] for f in _lib.ImageDesc._fields_]
    assert names[-1] == "ncls" and names[-5:-1] == ["b", "H", "W", "vn"]
    assert _lib.ImageDesc().ncls == 0          # a zero-initialised descriptor is a single-object one
    # pv_image_desc: 8 + 8 + 32 + 8 + 8 + 40 + 4 * 4 + 4, padded to the pointers' alignment
    assert ctypes.sizeof(_lib.ImageDesc) == 128 and _lib.ImageDesc.ncls.offset == 120


@pytest.mark.parametrize("ncls", [-1, 65])
def test_v3_rejects_class_count_out_of_range(lib, ncls):
    from pvnet_amd import _lib
    d = desc(ncls=ncls)
    p = _lib.VoteParams(round_hyp_num=8)
    assert lib.pv_ransac_voting_v3(ctypes.byref(d), ctypes.byref(p), 1, 1, 1 << 40, None, None) == -1


def test_v3_multi_needs_its_workspace(lib):
    from pvnet_amd import _lib
    d = desc(ncls=2)
    p = _lib.VoteParams(round_hyp_num=8)
    assert lib.pv_ransac_voting_v3(ctypes.byref(d), ctypes.byref(p), 1, None, 0, None, None) == -2
    # sized for the b * ncls virtual images: one image's workspace is too small for two classes
    one = lib.pv_v3_workspace_size(1, 4, 4, 9, 8)
    assert lib.pv_v3_workspace_size(2, 4, 4, 9, 8) > one
    assert lib.pv_ransac_voting_v3(ctypes.byref(d), ctypes.byref(p), 1, 1, one, None, None) == -2


def test_evd_rejects_class_count_out_of_range(lib):
    from pvnet_amd import _lib
    d = desc(ncls=65)
    p = _lib.VoteParams(round_hyp_num=8, min_hyp_num=8, topk=4)
    assert lib.pv_estimate_voting_distribution_with_mean(ctypes.byref(d), ctypes.byref(p), 1, 1, 1, 1 << 40,
                                                         None) == -1
    assert lib.pv_estimate_voting_distribution(ctypes.byref(d), ctypes.byref(p), 1, 1, 1, 1 << 40, None) == -1


def test_motion_voting_is_single_object_only(lib):
    d = desc(ncls=1)
    assert lib.pv_ransac_motion_voting(ctypes.byref(d), 1, None) == -1


def test_multi_layers_are_exported():
    from pvnet_amd import ransac_voting_gpu as rvg
    for name in ("ransac_voting_layer_v3_multi", "ransac_voting_layer_v3_multi_from_network",
                 "estimate_voting_distribution_with_mean_multi"):
        assert name in rvg.__all__ and callable(getattr(rvg, name))


def test_multi_layers_reject_host_tensors():
    from pvnet_amd import ransac_voting_gpu as rvg
    label = torch.zeros(1, 4, 4, dtype=torch.int64)
    vertex = torch.zeros(1, 4, 4, 6, 2)
    with pytest.raises(RuntimeError, match="CUDA"):
        rvg.ransac_voting_layer_v3_multi(label, vertex, 3, 8)
    with pytest.raises(RuntimeError, match="CUDA"):
        rvg.estimate_voting_distribution_with_mean_multi(label, vertex, torch.zeros(1, 3, 2, 2), 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        rvg.ransac_voting_layer_v3_multi_from_network(torch.zeros(1, 4, 4, 4), torch.zeros(1, 12, 4, 4), 3, 8)


def test_multi_layers_reject_bad_shapes_before_any_device_call():
    from pvnet_amd import ransac_voting_gpu as rvg
    label = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="divisible"):
        rvg.ransac_voting_layer_v3_multi(label, torch.zeros(1, 4, 4, 7, 2), 3, 8)
    with pytest.raises(RuntimeError, match="divisible"):
        rvg.estimate_voting_distribution_with_mean_multi(label, torch.zeros(1, 4, 4, 7, 2), torch.zeros(1, 3, 2, 2), 3)
    # seg_pred needs class_num + 1 channels
    with pytest.raises(RuntimeError, match=r"class_num\+1"):
        rvg.ransac_voting_layer_v3_multi_from_network(torch.zeros(1, 3, 4, 4), torch.zeros(1, 12, 4, 4), 3, 8)
    with pytest.raises(RuntimeError, match="divisible"):
        rvg.ransac_voting_layer_v3_multi_from_network(torch.zeros(1, 4, 4, 4), torch.zeros(1, 14, 4, 4), 3, 8)
    with pytest.raises(RuntimeError, match="dtype"):
        rvg.ransac_voting_layer_v3_multi(label.to(torch.float32), torch.zeros(1, 4, 4, 6, 2), 3, 8)
    with pytest.raises(RuntimeError, match="class_num"):
        rvg.ransac_voting_layer_v3_multi(label, torch.zeros(1, 4, 4, 6, 2), 0, 8)
    with pytest.raises(RuntimeError, match=r"\[b,h,w\]"):
        rvg.ransac_voting_layer_v3_multi(torch.zeros(1, 4, 5, dtype=torch.int64), torch.zeros(1, 4, 4, 6, 2), 3, 8)
