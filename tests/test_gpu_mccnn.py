"""The MC-CNN matching cost on the device (sm_mccnn.hpp: k_mc_sums, k_mc_layer0, k_mc_conv on the
f32 matrix instruction, k_mc_unit, k_mc_join) against the CPU twin, bit for bit: features and
volumes over tile edges, layer counts and an asymmetric integer net; batches, strides and context
reuse; and the volume straight into computeFromCost."""
import numpy as np
import pytest

import mccnn_cases as C
import stereo_match_amd as sm

pytestmark = pytest.mark.gpu


def device_features(m, img):
    import torch

    return m.features(torch.from_numpy(np.array(img)).cuda())


@pytest.mark.parametrize("name", ["tiny", "ragged", "tiles"])
@pytest.mark.parametrize("layers", [1, 2, 4, 5])
def test_features_match_twin(name, layers):
    """Fewer pixels than one 8 x 32 tile, ragged tile edges in both directions, several tiles."""
    m = C.model(layers)
    want = C.twin_features(name, layers, 0)
    got = m.features(C.image(name, 0))  # the host-pointer entry point
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} values differ"
    dev = device_features(m, C.image(name, 0))  # the device entry point
    assert np.array_equal(dev.cpu().numpy(), want)
    norm = np.sqrt((got.astype(np.float64) ** 2).sum(-1))
    assert np.abs(norm - 1).max() < 1e-6


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_integer_net(layers):
    """One or two nonzero integer weights per output map, at a different input map and tap for each:
    a transposed operand, a swapped tap or a wrong accumulator row gives other values."""
    m = C.integer_model(layers)
    for name in ("ragged", "tiles"):
        want = C.twin_features(name, layers, 0, integer=True)
        assert np.abs(want).max() > 0
        got = m.features(C.image(name, 0))
        assert np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("name,D,m0", [("tiny", 20, 0), ("ragged", 12, -4), ("tiles", 70, 3), ("tiny", 256, -100),
                                       ("tiles", 131, 0)])
def test_volume_matches_twin(name, D, m0):
    """One chunk of planes and several, a partial last chunk, negative and positive offsets, more
    planes than columns."""
    m = C.model(4)
    a, b = C.image(name, 0), C.image(name, 1)
    want = m.join(C.twin_features(name, 4, 0), C.twin_features(name, 4, 1), D, m0, host=True)
    got = m.cost_volume(a, b, D, m0)
    assert got.shape == (1, D) + a.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert C.same_bits(got, want)


def test_batch_of_three():
    import torch

    m = C.model(4)
    batch = C.image("tiles", 5, batch=3)
    want = C.twin_features("tiles", 4, 5, batch=3)
    got = m.features(batch)
    assert np.array_equal(got, want)
    for i in range(3):  # batch equals single
        assert np.array_equal(m.features(batch[i]), got[i])
    t = torch.from_numpy(np.array(batch)).cuda()
    ft = m.features(t)
    assert np.array_equal(ft.cpu().numpy(), want)
    vol = m.join(ft, ft.flip(0), 40, -3)
    wantv = m.join(want, want[::-1], 40, -3, host=True)
    assert vol.shape == (3, 40, 70, 131) and C.same_bits(vol.cpu().numpy(), wantv)


def test_strided_input_and_reuse():
    """row_stride > W and images further apart than H rows equal the packed images; a second call
    on the same context gives the same bytes."""
    import torch

    m = C.model(4)
    batch = C.image("ragged", 2, batch=2)
    want = C.twin_features("ragged", 4, 2, batch=2)
    H, W = batch.shape[1:]
    wide = torch.zeros((2, H + 3, W + 29), dtype=torch.uint8).cuda()
    view = wide[:, 1:H + 1, 7:7 + W]
    view.copy_(torch.from_numpy(np.array(batch)))
    assert not view.is_contiguous()
    first = m.features(view).cpu().numpy()
    assert np.array_equal(first, want)
    other = C.model(2).features(C.image("tiny", 0))  # another net and shape through the same context
    assert np.array_equal(other, C.twin_features("tiny", 2, 0))
    assert np.array_equal(m.features(view).cpu().numpy(), first)
    assert np.array_equal(m.features(batch), first)


def test_constant_image_is_an_error_on_the_device():
    m = C.model(2)
    imgs = np.array(C.image("tiny", 0, batch=2))
    imgs[1] = 77
    with pytest.raises(ValueError, match="image 1 is constant"):
        m.features(imgs)
    assert np.array_equal(m.features(imgs[0]), m.features(imgs[0], host=True))  # the context still works


@pytest.mark.parametrize("mode", ["sgbm", "hh"])
def test_end_to_end_into_compute_from_cost(mode):
    """computeFromCost of the device volume (CUDA tensors, no copy through the host) equals
    computeFromCost of the twin's numpy volume; the right matcher through cost_volumes."""
    import torch

    m = C.model(4)
    left = C.image("tiles", 0)
    right = np.roll(left, -6, axis=1)
    matcher = sm.StereoSGBM_create(minDisparity=0, numDisparities=32, P1=40, P2=160, uniquenessRatio=5,
                                   mode=sm.STEREO_SGBM_MODE_HH if mode == "hh" else sm.STEREO_SGBM_MODE_SGBM)
    t_l, t_r = torch.from_numpy(np.array(left)).cuda(), torch.from_numpy(right).cuda()
    vol = m.cost_volume(t_l, t_r, 32)
    assert vol.is_cuda and tuple(vol.shape) == (1, 32) + left.shape
    twin = m.cost_volume(left, right, 32, host=True)
    assert C.same_bits(vol.cpu().numpy(), twin)
    got = matcher.computeFromCost(vol, 1.0, 2047.5)
    want = matcher.computeFromCost(twin, 1.0, 2047.5)
    assert np.array_equal(got.cpu().numpy(), want)
    vl, vr = m.cost_volumes(t_l, t_r, matcher)
    tl, tr = m.cost_volumes(left, right, matcher, host=True)
    assert C.same_bits(vl.cpu().numpy(), tl) and C.same_bits(vr.cpu().numpy(), tr)
    rmatcher = sm.createRightMatcher(matcher)
    assert np.array_equal(rmatcher.computeFromCost(vr, 1.0, 2047.5).cpu().numpy(), rmatcher.computeFromCost(tr, 1.0, 2047.5))


def test_fused_volume_entry_points():
    """sm_mccnn_volume (host pointers) and sm_mccnn_volume_device through their Engine wrappers: a
    batch, a strided input (row_stride > W, images further apart than H rows), two calls on one
    context, against the twin bit for bit."""
    import torch

    m = C.model(4)
    a, b = C.image("ragged", 2, batch=2), C.image("ragged", 4, batch=2)
    D, m0 = 70, -3  # two chunks of planes, the second partial
    want = m.join(C.twin_features("ragged", 4, 2, batch=2), C.twin_features("ragged", 4, 4, batch=2), D, m0, host=True)
    eng = m._engine()
    for _ in range(2):
        got = eng.mccnn_volume(np.array(a), np.array(b), D, m0)
        assert got.shape == want.shape and C.same_bits(got, want)
    n, H, W = a.shape
    wide = torch.zeros((2, n, H + 3, W + 29), dtype=torch.uint8).cuda()
    va, vb = wide[0, :, 1:H + 1, 7:7 + W], wide[1, :, 1:H + 1, 7:7 + W]
    va.copy_(torch.from_numpy(np.array(a)))
    vb.copy_(torch.from_numpy(np.array(b)))
    assert va.stride() == vb.stride() and va.stride(1) > W and va.stride(0) > H * va.stride(1)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        vol = torch.empty((n, D, H, W), dtype=torch.float32, device="cuda")
        eng.mccnn_volume_device(va.data_ptr(), vb.data_ptr(), n, va.stride(0), H, W, va.stride(1), D, m0, vol.data_ptr())
        assert C.same_bits(vol.cpu().numpy(), want)
    # the public method takes the same road
    assert C.same_bits(m.cost_volume(va, vb, D, m0).cpu().numpy(), want)
    assert C.same_bits(m.cost_volume(a, b, D, m0), want)
    with pytest.raises(ValueError, match="16-byte aligned"):  # feature maps are read 16 bytes at a time
        f = torch.zeros(H * W * 64 + 1, dtype=torch.float32, device="cuda")
        eng.mccnn_features_device(va.data_ptr(), 1, va.stride(0), H, W, va.stride(1), f.data_ptr() + 4)
