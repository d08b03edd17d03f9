"""MC-CNN's stereo method on the device (sm_mcsgm.hpp: k_mcs_vert, k_mcs_horz and the image-sized
stages) against the CPU twin, value for value and NaN for NaN: the aggregation over every strip,
tile and plane-count path, the right view, batches, strides, a reused context, every stage of the
disparity step, and McCnnStereo.compute end to end."""
import numpy as np
import pytest

import mccnn_cases as M
import mcsgm_cases as C
import stereo_match_amd as sm

pytestmark = pytest.mark.gpu


def cuda(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()


@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_aggregation_matches_twin(shape):
    H, W, D, m = shape
    left, right, vl, _ = C.scene(*shape)
    want = C.twin_aggregates(*shape)[0]
    got = sm.mc_aggregate(vl, left, right, m, C.DEFAULT)  # the host-pointer entry point
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert C.same_bits(got, want), f"{int((got != want).sum() - np.isnan(want).sum())} of {want.size} values differ"
    dev = sm.mc_aggregate(cuda(vl), cuda(left), cuda(right), m, C.DEFAULT)  # the device entry point
    assert dev.is_cuda and C.same_bits(dev.cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(33, 65, 65, 3), (40, 131, 37, -4)], ids=str)
def test_right_view(shape):
    H, W, D, m = shape
    left, right, _, vr = C.scene(*shape)
    got = sm.mc_aggregate(vr, right, left, C.right_m(D, m), C.DEFAULT)
    assert C.same_bits(got, C.twin_aggregates(*shape)[1])


def test_two_iterations():
    shape = (33, 65, 65, 3)
    left, right, vl, _ = C.scene(*shape)
    p = sm.McCnnStereoParams(sgm_i=2)
    assert C.same_bits(sm.mc_aggregate(vl, left, right, shape[3], p), sm.mc_aggregate(vl, left, right, shape[3], p, host=True))


def batch_of_two():
    shape = (33, 65, 65, 3)
    one, two = C.scene(*shape), C.scene(*shape, seed=8)
    vol = np.stack([one[2], two[2]])
    lefts, rights = np.stack([one[0], two[0]]), np.stack([one[1], two[1]])
    want = np.stack([C.twin_aggregates(*shape)[0], sm.mc_aggregate(two[2], two[0], two[1], shape[3], host=True)])
    return shape, vol, lefts, rights, want


def test_batch_of_two_equals_two_calls():
    shape, vol, lefts, rights, want = batch_of_two()
    got = sm.mc_aggregate(vol, lefts, rights, shape[3])
    assert C.same_bits(got, want)
    for i in range(2):
        assert C.same_bits(sm.mc_aggregate(vol[i], lefts[i], rights[i], shape[3]), got[i])
    dev = sm.mc_aggregate(cuda(vol), cuda(lefts), cuda(rights), shape[3])
    assert C.same_bits(dev.cpu().numpy(), want)
    # the disparity step on the batch
    al, ar = got, np.stack([sm.mc_aggregate(np.ascontiguousarray(vol[i]), rights[i], lefts[i], C.right_m(shape[2], shape[3]))
                            for i in range(2)])  # any second volume will do: device and twin see the same one
    want_d = sm.mc_disparity(al, ar, lefts, shape[3], C.SMALL_BLUR, host=True)
    assert C.same_bits(sm.mc_disparity(al, ar, lefts, shape[3], C.SMALL_BLUR), want_d)
    assert C.same_bits(sm.mc_disparity(cuda(al), cuda(ar), cuda(lefts), shape[3], C.SMALL_BLUR).cpu().numpy(), want_d)


def test_strided_cuda_images_equal_packed():
    import torch

    shape, vol, lefts, rights, want = batch_of_two()
    n, H, W = lefts.shape
    wide = torch.zeros((2, n, H + 3, W + 29), dtype=torch.uint8).cuda()
    va, vb = wide[0, :, 1:H + 1, 7:7 + W], wide[1, :, 1:H + 1, 7:7 + W]
    va.copy_(cuda(lefts))
    vb.copy_(cuda(rights))
    assert not va.is_contiguous() and va.stride(1) > W
    got = sm.mc_aggregate(cuda(vol), va, vb, shape[3])
    assert C.same_bits(got.cpu().numpy(), want)
    want_d = sm.mc_disparity(want, want, lefts, shape[3], C.SMALL_BLUR, host=True)
    assert C.same_bits(sm.mc_disparity(got, got, va, shape[3], C.SMALL_BLUR).cpu().numpy(), want_d)
    # a strided volume is packed first
    big = torch.zeros((n, shape[2], H, W + 5), dtype=torch.float32).cuda()
    big[..., :W] = cuda(vol)
    assert C.same_bits(sm.mc_aggregate(big[..., :W], va, vb, shape[3]).cpu().numpy(), want)


def test_context_reused_at_a_larger_and_a_smaller_shape():
    for shape in [(5, 3, 20, 0), (20, 200, 228, 0), (1, 70, 5, 0), (33, 65, 65, 3)]:
        left, right, vl, _ = C.scene(*shape)
        assert C.same_bits(sm.mc_aggregate(vl, left, right, shape[3]), C.twin_aggregates(*shape)[0]), shape
        al, ar = C.stage_inputs(*shape)
        assert C.same_bits(sm.mc_disparity(al, ar, left, shape[3], C.SMALL_BLUR), C.twin_disparity(*shape)[0]), shape


@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_every_stage_matches_twin(shape):
    H, W, D, m = shape
    al, ar = C.stage_inputs(*shape)
    left = C.scene(*shape)[0]
    want, want_maps = C.twin_disparity(*shape)
    got, maps = sm.mc_disparity(al, ar, left, m, C.SMALL_BLUR, stages=True)
    for k in sm.mcstereo.STAGES:
        assert maps[k].dtype == want_maps[k].dtype and C.same_bits(maps[k], want_maps[k]), k
    assert got.dtype == np.float32 and C.same_bits(got, want)
    dev, dev_maps = sm.mc_disparity(cuda(al), cuda(ar), cuda(left), m, C.SMALL_BLUR, stages=True)
    for k in sm.mcstereo.STAGES:
        assert C.same_bits(dev_maps[k].cpu().numpy(), want_maps[k]), k
    assert C.same_bits(dev.cpu().numpy(), want)
    assert C.same_bits(sm.mc_disparity(cuda(al), cuda(ar), cuda(left), m, C.SMALL_BLUR).cpu().numpy(), want)


def test_default_bilateral_window():
    shape = (9, 130, 256, -100)
    al, ar = C.stage_inputs(*shape)
    left = C.scene(*shape)[0]
    want = sm.mc_disparity(al, ar, left, shape[3], C.DEFAULT, host=True)
    assert C.same_bits(sm.mc_disparity(al, ar, left, shape[3], C.DEFAULT), want)
    # another sigma on the same context replaces the cached weights
    assert C.same_bits(sm.mc_disparity(al, ar, left, shape[3], C.SMALL_BLUR), C.twin_disparity(*shape)[0])


def test_overlapping_output_is_refused():
    import torch

    from stereo_match_amd import _lib

    left, right, vl, _ = C.scene(5, 3, 20, 0)
    v, a, b = cuda(vl), cuda(left), cuda(right)
    eng = _lib.engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ValueError, match="overlaps"):
        eng.mcsgm_aggregate_device(v.data_ptr(), a.data_ptr(), b.data_ptr(), 1, 15, 5, 3, 3, 20, 0, C.DEFAULT.c_struct(),
                                   v.data_ptr() + 4)
    assert C.same_bits(v.cpu().numpy(), vl)


def test_compute_end_to_end():
    """McCnnStereo.compute on CUDA tensors and on numpy images equals the composition of the twins."""
    net = M.model(4)
    left = M.image("ragged", 0)
    right = np.roll(left, -5, axis=1)
    stereo = sm.McCnnStereo(net, sm.McCnnStereoParams(blur_sigma=2.0, blur_t=0.5))
    want, want_r = stereo.compute(left, right, 24, -3, host=True)
    assert want.shape == left.shape and want.dtype == np.float32 and want_r.dtype == np.float32
    assert (want != want[0, 0]).any()
    got, got_r = stereo.compute(cuda(left), cuda(right), 24, -3)
    assert got.is_cuda and got_r.is_cuda
    assert C.same_bits(got.cpu().numpy(), want) and C.same_bits(got_r.cpu().numpy(), want_r)
    got, got_r = stereo.compute(left, right, 24, -3)
    assert C.same_bits(got, want) and C.same_bits(got_r, want_r)
