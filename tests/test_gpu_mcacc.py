"""The accurate MC-CNN matching cost on the device (sm_mcacc.hpp: k_ac_sums, k_ac_layer0, k_ac_conv
and k_ac_dense on the f32 matrix instruction, k_ac_h1, k_ac_final) against the CPU twin, bit for
bit: features over tile edges and layer counts, volumes over unit and layer counts, both roles and
chunked cells, integer nets against int64 numpy; batches, strides and context reuse beside the fast
net; the volume into computeFromCost and McCnnStereo."""
import numpy as np
import pytest

import mcacc_cases as C
import mccnn_cases as FAST
import stereo_match_amd as sm

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("name", ["tiny", "ragged", "tiles"])
@pytest.mark.parametrize("layers", [1, 2, 4, 5])
def test_features_match_twin(name, layers):
    """Fewer pixels than one 2 x 32 tile row, ragged tile edges in both directions, several tiles."""
    m = C.model(layers)
    want = C.twin_features(name, layers, 0)
    got = m.features(C.image(name, 0))  # the host-pointer entry point
    assert got.dtype == np.float32 and got.shape == want.shape == C.SHAPES[name] + (112,)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} values differ"
    dev = m.features(cuda(C.image(name, 0)))  # the device entry point
    assert np.array_equal(dev.cpu().numpy(), want)
    assert got.min() >= 0 and got.max() > 0


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_integer_conv_net(layers):
    """One or two nonzero integer weights per output map, at a different input map and tap for each:
    a transposed operand, a swapped tap or a wrong accumulator row gives other values."""
    m = C.integer_model(layers)
    for name in ("ragged", "tiles"):
        want = C.twin_features(name, layers, 0, integer=True)
        assert np.abs(want).max() > 0
        got = m.features(C.image(name, 0))
        assert np.array_equal(got, want), (name, int((got != want).sum()))


CASES = [("tiny", 1, 0), ("tiny", 20, 0), ("ragged", 12, -4), ("tiles", 70, 3), ("tiny", 60, -30)]
VOLUMES = ([(c, 1, 32, True) for c in CASES] + [(c, 2, 96, True) for c in CASES]
           + [(CASES[1], 1, 32, False), (CASES[2], 2, 96, False), (CASES[4], 2, 96, False)]
           + [(CASES[0], 4, 384, True), (CASES[1], 4, 384, True), (CASES[1], 4, 384, False), (CASES[2], 2, 384, True)])


@pytest.mark.parametrize("case,F,U,left", VOLUMES)
def test_volume_matches_twin(case, F, U, left):
    """One plane, several, negative and positive offsets, more planes than columns; one, three and
    twelve 32-blocks of units; no U x U layer, one, three; both roles."""
    name, D, m0 = case
    m = C.model(2, F, U)
    a, b = C.image(name, 0), C.image(name, 1)
    want = C.twin_volume(name, D, m0, F, U, left)
    got = m.cost_volume(a, b, D, m0, a_is_left=left)
    assert got.shape == (1, D) + a.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert C.same_bits(got, want), int((got != want).sum())
    assert np.nanmin(got) >= -1 and np.nanmax(got) <= 0
    # the two steps on CUDA tensors are the fused call
    fa, fb = m.features(cuda(a)), m.features(cuda(b))
    assert C.same_bits(m.join(fa, fb, D, m0, a_is_left=left).cpu().numpy(), want)


@pytest.mark.parametrize("F,U", [(1, 32), (2, 32), (3, 96)])
def test_raw_integer_scorer(F, U):
    """raw=True on integer features and an asymmetric integer scorer: the int64 numpy values of the
    network's definition, in both roles; and the twin's sigmoid of them."""
    m = C.integer_model(2, F, U)
    fa, fb = C.integer_features("ragged", 0), C.integer_features("ragged", 1)
    D, m0 = 12, -4
    for left in (True, False):
        want, peak = C.int_volume(m, fa, fb, D, m0, left)
        assert 0 < peak < 2**24
        got = m.join(fa, fb, D, m0, a_is_left=left, raw=True)
        assert C.same_bits(got[0], want), (left, int((got[0] != want).sum()))
        assert C.same_bits(m.join(fa, fb, D, m0, a_is_left=left), m.join(fa, fb, D, m0, a_is_left=left, host=True))


def test_chunked_cells():
    """31080 cells in passes of 12000: three chunks, the last one ragged and none a multiple of the
    128-row tile, against the one-pass result and the twin."""
    m = C.model(2, 2, 96)
    a, b = C.image("ragged", 0), C.image("ragged", 1)
    want = C.twin_volume("ragged", 12, -4, 2, 96)
    eng = m._engine()
    one = m.cost_volume(a, b, 12, -4)
    try:
        eng.set_tuning(eng.TUNE_MCACC_CHUNK, 12000)
        three = m.cost_volume(a, b, 12, -4)
        eng.set_tuning(eng.TUNE_MCACC_CHUNK, 129)
        many = m.cost_volume(a, b, 12, -4)
    finally:
        eng.set_tuning(eng.TUNE_MCACC_CHUNK, 0)
    assert C.same_bits(one, want) and C.same_bits(three, one) and C.same_bits(many, one)
    with pytest.raises(ValueError):
        eng.set_tuning(eng.TUNE_MCACC_CHUNK, -1)


def test_cost_volumes():
    """cost_volumes is two cost_volume calls, and the right volume holds the left one's values at the
    cells that pair the same two columns."""
    m = C.model(2, 2, 96)
    left, right = C.image("ragged", 0), C.image("ragged", 1)
    matcher = sm.StereoSGBM_create(minDisparity=-4, numDisparities=16)
    rm = sm.createRightMatcher(matcher)
    vl, vr = m.cost_volumes(cuda(left), cuda(right), matcher)
    vl, vr = vl.cpu().numpy(), vr.cpu().numpy()
    assert C.same_bits(vl, m.cost_volume(left, right, 16, -4))
    assert C.same_bits(vr, m.cost_volume(right, left, rm.numDisparities, rm.minDisparity, a_is_left=False))
    tl, tr = m.cost_volumes(left, right, matcher, host=True)
    assert C.same_bits(vl, tl) and C.same_bits(vr, tr)
    W = left.shape[1]
    x = np.arange(W)
    for d in (0, 3, 4, 9, 15):
        s = -4 + d
        dr = -s - rm.minDisparity
        ok = (x - s >= 0) & (x - s < W)
        assert np.array_equal(vr[0, dr][:, x[ok] - s], vl[0, d][:, ok])


def test_batch_strides_and_reuse():
    """A batch of 3, row_stride > W with images further apart than H rows, a second call on the same
    context and another net in between."""
    import torch

    m = C.model(2, 2, 96)
    batch = C.image("ragged", 2, batch=3)
    want = C.twin_features("ragged", 2, 2, batch=3)
    got = m.features(batch)
    assert np.array_equal(got, want)
    n, H, W = batch.shape
    wide = torch.zeros((n, H + 3, W + 29), dtype=torch.uint8).cuda()
    view = wide[:, 1:H + 1, 7:7 + W]
    view.copy_(torch.from_numpy(np.array(batch)))
    assert not view.is_contiguous()
    first = m.features(view)
    assert np.array_equal(first.cpu().numpy(), want)
    wantv = m.join(want, want[::-1], 9, -2, host=True)
    vol = m.join(first, first.flip(0), 9, -2)
    assert vol.shape == (3, 9, H, W) and C.same_bits(vol.cpu().numpy(), wantv)
    assert C.same_bits(m.cost_volume(view, view.flip(0), 9, -2).cpu().numpy(), wantv)
    other = C.model(1, 1, 32)
    assert C.same_bits(other.cost_volume(C.image("tiny", 0), C.image("tiny", 1), 20, 0), C.twin_volume("tiny", 20, 0, 1, 32, conv_layers=1))
    assert np.array_equal(m.features(view).cpu().numpy(), want)
    assert C.same_bits(m.join(got, got[::-1], 9, -2), wantv)  # host pointers
    with pytest.raises(ValueError, match="16-byte aligned"):
        f = torch.zeros(H * W * 112 + 1, dtype=torch.float32, device="cuda")
        m._engine().mcacc_features_device(view.data_ptr(), 1, view.stride(0), H, W, view.stride(1), f.data_ptr() + 4)
    imgs = np.array(batch)
    imgs[1] = 77
    with pytest.raises(ValueError, match="image 1 is constant"):
        m.features(imgs)
    assert np.array_equal(m.features(batch[0]), want[0])  # the context still works


def test_fast_and_accurate_on_one_engine():
    """The two nets keep their own weights in the context: used alternately, each equals its twin."""
    acc, fast = C.model(2, 2, 96), FAST.model(2)
    a, b = C.image("tiny", 0), C.image("tiny", 1)
    assert acc._engine() is fast._engine()
    want_acc = C.twin_volume("tiny", 20, 0, 2, 96)
    want_fast = fast.cost_volume(a, b, 20, 0, host=True)
    for _ in range(2):
        assert C.same_bits(acc.cost_volume(a, b, 20, 0), want_acc)
        assert C.same_bits(fast.cost_volume(a, b, 20, 0), want_fast)
    assert np.array_equal(fast.features(a), FAST.twin_features("tiny", 2, 0))
    assert np.array_equal(acc.features(a), C.twin_features("tiny", 2, 0))


def test_end_to_end_into_compute_from_cost():
    """computeFromCost of the device volume (CUDA tensors) equals computeFromCost of the twin's numpy
    volume, in the fixed window of costs in [-1, 0]."""
    m = C.model(2, 2, 96)
    left = C.image("ragged", 0)
    right = np.roll(left, -4, axis=1)
    matcher = sm.StereoSGBM_create(minDisparity=0, numDisparities=16, P1=40, P2=160, uniquenessRatio=5)
    vol = m.cost_volume(cuda(left), cuda(right), 16)
    assert vol.is_cuda and tuple(vol.shape) == (1, 16) + left.shape
    twin = m.cost_volume(left, right, 16, host=True)
    assert C.same_bits(vol.cpu().numpy(), twin)
    got = matcher.computeFromCost(vol, 1.0, 4095.0)
    want = matcher.computeFromCost(twin, 1.0, 4095.0)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_stereo_end_to_end(name):
    """McCnnStereo with the accurate net on the device equals the composition of the twins; the
    cross-based aggregation rides along on one shape."""
    net = C.model(2, 2, 96)
    left = C.image(name, 0)
    right = np.roll(left, -3, axis=1)
    cross = sm.McCnnCrossParams(i1=1) if name == "tiny" else None
    stereo = sm.McCnnStereo(net, sm.McCnnStereoParams(blur_sigma=2.0, blur_t=0.5), cross)
    want, want_r = stereo.compute(left, right, 12, -2, host=True)
    assert want.shape == left.shape and want.dtype == np.float32
    got, got_r = stereo.compute(cuda(left), cuda(right), 12, -2)
    assert got.is_cuda and C.same_bits(got.cpu().numpy(), want) and C.same_bits(got_r.cpu().numpy(), want_r)
    got, got_r = stereo.compute(left, right, 12, -2)
    assert C.same_bits(got, want) and C.same_bits(got_r, want_r)
