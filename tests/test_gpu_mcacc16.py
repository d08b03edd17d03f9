"""McCnnAccurate's precision="bf16" on the device (sm_mcacc.hpp: k_ac_fused16, the whole scorer of a
tile of cells in one kernel on the bf16 matrix instruction) -- DESIGN.md §4.21.  Dense integer nets:
device == twin == exact numpy, bit for bit, over the tile's edges.  Random float nets: within E_q,
the distance between the two CPU twins, of the bf16 twin.  Determinism, both views, batches, strides,
reuse, two precisions alternately on one engine, and McCnnStereo on a bf16 net."""
import numpy as np
import pytest

import mcacc16_cases as Q
import stereo_match_amd as sm
from stereo_match_amd.mcstereo import mc_aggregate, mc_disparity, right_min_disparity

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


NETS = [(1, 32), (2, 32), (3, 96), (3, 352), (4, 384), (2, 384)]
# a wave takes 32 columns of one plane, a workgroup 4 planes: several tiles each way; ragged in x;
# planes that are NaN throughout (offsets 45 .. 59 of 45 columns); fewer columns than a tile; ragged
# in x (37 = 32 + 5) and in d (6 = 4 + 2)
GEOS = [("tiny", 20, 0), ("ragged", 12, -3), ("tiny", 30, 30), ("narrow", 7, -2), ("odd", 6, 1)]


@pytest.mark.parametrize("geo,D,m0", GEOS)
@pytest.mark.parametrize("F,U", NETS)
def test_integer_nets_bit_for_bit(F, U, geo, D, m0):
    """Every sum stays below 2^24 in magnitude (asserted by the evaluation), so the order of the
    matrix instruction's additions cannot show: the device equals the twin and the exact numpy
    values, raw and through the sigmoid, in both roles, on numpy and on CUDA tensors.  A wrong
    lane map, k permutation or weight packing gives other integers."""
    m = Q.dense_model(F, U)
    fa, fb = Q.int_features(geo, 0), Q.int_features(geo, 1)
    for left in (True, False):
        want, info = Q.int_volume16(F, U, geo, D, m0, left)
        assert 0 < info["peak"] < 2**24
        if geo == "tiny" and m0 == 30:
            assert np.isnan(want[15:]).all() and not np.isnan(want[0]).all()
        twin = m.join(fa, fb, D, m0, a_is_left=left, raw=True, host=True)
        assert Q.same_bits(twin[0], want)
        got = m.join(fa, fb, D, m0, a_is_left=left, raw=True)
        assert got.shape == (1, D) + fa.shape[:2] and got.dtype == np.float32
        assert np.array_equal(np.isnan(got[0]), np.isnan(want))
        assert Q.same_bits(got[0], want), (left, int((got[0] != want).sum()))
        dev = m.join(cuda(fa), cuda(fb), D, m0, a_is_left=left, raw=True)
        assert dev.is_cuda and Q.same_bits(dev.cpu().numpy()[0], want)
        squashed = m.join(cuda(fa), cuda(fb), D, m0, a_is_left=left).cpu().numpy()
        assert Q.same_bits(squashed, m.join(fa, fb, D, m0, a_is_left=left, host=True))
        assert Q.same_bits(m.join(fa, fb, D, m0, a_is_left=left), squashed)


@pytest.mark.parametrize("F,U", [(2, 32), (4, 384)])
def test_cost_volume_is_features_and_join(F, U):
    """The fused entry point in bf16 mode gives the bits of features + join, from numpy images and
    from CUDA tensors."""
    m = Q.dense_model(F, U)
    a, b = Q.image("tiny", 0), Q.image("tiny", 1)
    for left in (True, False):
        want = m.join(m.features(a), m.features(b), 20, -3, a_is_left=left)
        assert np.isfinite(want).any()
        assert Q.same_bits(m.cost_volume(a, b, 20, -3, a_is_left=left), want)
        assert Q.same_bits(m.cost_volume(cuda(a), cuda(b), 20, -3, a_is_left=left).cpu().numpy(), want)


def test_more_tiles_than_resident_workgroups():
    """64 x 256 x 32 = 524288 cells, 4096 workgroups of 128 cells: several rounds of resident
    workgroups on every compute unit.  (2, 32), bit for bit against the twin and numpy."""
    m = Q.dense_model(2, 32)
    fa, fb = Q.int_features("wide", 0), Q.int_features("wide", 1)
    want, info = Q.int_volume16(2, 32, "wide", 32, -5)
    assert 0 < info["peak"] < 2**24
    assert Q.same_bits(m.join(fa, fb, 32, -5, raw=True, host=True)[0], want)
    assert Q.same_bits(m.join(fa, fb, 32, -5, raw=True)[0], want)


FLOAT_CASES = [("tiny", 20, 0), ("ragged", 12, -3)]


@pytest.mark.parametrize("name,D,m0", FLOAT_CASES)
@pytest.mark.parametrize("F,U", [(2, 96), (3, 384), (4, 384)])
def test_random_float_nets_within_e_q(name, D, m0, F, U):
    """max |device - twin_bf16| <= E_q on the raw volume, E_q = max |twin_bf16 - twin_f32| of the
    same case from the two CPU twins.  The device differs from the twin by the order of the float32
    additions (O(K 2^-24) relative) and by rare one-unit flips of a rounded operand; E_q sums about
    sqrt(K) operand roundings of 2^-9 per layer.  A wrong lane map errs at the size of the values.
    Measured ratios: DESIGN.md §4.21."""
    m = Q.float_net(F, U)
    fa, fb = Q.twin_features(name, 2, 0), Q.twin_features(name, 2, 1)
    for left in (True, False):
        twin = Q.twin_raw(name, D, m0, F, U, "bf16", left)
        eq = Q.e_q(name, D, m0, F, U, left)
        assert eq > 0
        got = m.join(fa, fb, D, m0, a_is_left=left, raw=True)
        assert np.array_equal(np.isnan(got), np.isnan(twin))
        err = float(np.nanmax(np.abs(got.astype(np.float64) - twin)))
        print(f"bf16 device vs twin {name} D={D} m={m0} F={F} U={U} left={left}: max {err:.3e}, E_q {eq:.3e}, "
              f"ratio {err / eq:.3e}, bit-equal {Q.same_bits(got, twin)}")
        assert err <= eq
        s = m.join(cuda(fa), cuda(fb), D, m0, a_is_left=left).cpu().numpy()
        assert np.array_equal(np.isnan(s), np.isnan(twin)) and np.nanmin(s) >= -1 and np.nanmax(s) <= 0


def test_deterministic():
    m = Q.float_net(4, 384)
    a, b = Q.image("ragged", 0), Q.image("ragged", 1)
    first = m.cost_volume(a, b, 12, -3)
    assert np.array_equal(first.view(np.uint32), m.cost_volume(a, b, 12, -3).view(np.uint32))
    ta, tb = cuda(a), cuda(b)
    assert np.array_equal(m.cost_volume(ta, tb, 12, -3).cpu().numpy().view(np.uint32), first.view(np.uint32))


def test_cost_volumes_views_agree():
    """The right view's volume pairs the same columns through the same projections: its cells agree
    with the left view's within E_q (whether they are in fact identical: DESIGN.md §4.21)."""
    m = Q.float_net(3, 384)
    left, right = Q.image("ragged", 0), Q.image("ragged", 1)
    matcher = sm.StereoSGBM_create(minDisparity=-3, numDisparities=12)
    rm = sm.createRightMatcher(matcher)
    vl, vr = m.cost_volumes(cuda(left), cuda(right), matcher)
    vl, vr = vl.cpu().numpy(), vr.cpu().numpy()
    assert Q.same_bits(vl, m.cost_volume(left, right, 12, -3))
    assert Q.same_bits(vr, m.cost_volume(right, left, rm.numDisparities, rm.minDisparity, a_is_left=False))
    eq = Q.e_q("ragged", 12, -3, 3, 384)
    W = left.shape[1]
    x = np.arange(W)
    worst, same = 0.0, True
    for d in range(12):
        s = -3 + d
        dr = -s - rm.minDisparity
        ok = (x - s >= 0) & (x - s < W)
        p, q = vr[0, dr][:, x[ok] - s], vl[0, d][:, ok]
        worst = max(worst, float(np.abs(p.astype(np.float64) - q).max()))
        same = same and np.array_equal(p, q)
    print(f"cost_volumes: largest difference between the views {worst:.3e}, E_q {eq:.3e}, identical {same}")
    assert worst <= eq  # of the similarity, whose slope is at most 1/4 of the raw value's


def test_batch_strides_and_reuse():
    """A batch of 3, row_stride > W with images further apart than H rows, a second call on the same
    context with another net in between."""
    import torch

    m = Q.dense_model(3, 96)
    batch = Q.image("ragged", 2, batch=3)
    n, H, W = batch.shape
    feat = m.features(batch)
    want = m.join(feat, feat[::-1], 9, -2)
    assert want.shape == (3, 9, H, W)
    for i in range(3):
        assert Q.same_bits(m.join(feat[i], feat[2 - i], 9, -2)[0], want[i])
    wide = torch.zeros((n, H + 3, W + 29), dtype=torch.uint8).cuda()
    view = wide[:, 1:H + 1, 7:7 + W]
    view.copy_(torch.from_numpy(np.array(batch)))
    assert not view.is_contiguous()
    assert Q.same_bits(m.cost_volume(view, view.flip(0), 9, -2).cpu().numpy(), want)
    other = Q.dense_model(2, 32)
    fa, fb = Q.int_features("tiny", 0), Q.int_features("tiny", 1)
    assert Q.same_bits(other.join(fa, fb, 20, 0, raw=True)[0], Q.int_volume16(2, 32, "tiny", 20, 0)[0])
    assert Q.same_bits(m.cost_volume(view, view.flip(0), 9, -2).cpu().numpy(), want)
    assert Q.same_bits(m.cost_volume(batch, batch[::-1], 9, -2), want)


def test_two_precisions_on_one_engine():
    """An f32 net and a bf16 net of the same arrays, alternately: the f32 results stay the bits of
    the f32 twin (today's arithmetic), the bf16 ones stay their own."""
    f32 = Q.model(2, 3, 96)
    b16 = f32.with_precision("bf16")
    assert f32._engine() is b16._engine()
    a, b = Q.image("tiny", 0), Q.image("tiny", 1)
    want32 = f32.cost_volume(a, b, 20, 0, host=True)
    first16 = b16.cost_volume(a, b, 20, 0)
    assert not Q.same_bits(first16, want32)
    for _ in range(2):
        assert Q.same_bits(f32.cost_volume(a, b, 20, 0), want32)
        assert Q.same_bits(b16.cost_volume(a, b, 20, 0), first16)
        assert Q.same_bits(f32.cost_volume(cuda(a), cuda(b), 20, 0).cpu().numpy(), want32)
    # the chunked f32 path is untouched by the mode having been used
    eng = f32._engine()
    try:
        eng.set_tuning(eng.TUNE_MCACC_CHUNK, 129)
        assert Q.same_bits(b16.cost_volume(a, b, 20, 0), first16)  # ignored in bf16 mode
        assert Q.same_bits(f32.cost_volume(a, b, 20, 0), want32)
    finally:
        eng.set_tuning(eng.TUNE_MCACC_CHUNK, 0)
    with pytest.raises(ValueError, match="precision"):
        eng.mcacc_set_precision("fp8")
    assert eng._lib.sm_mcacc_set_precision(eng.ctx, 7) == sm._lib.SM_E_ARG
    assert Q.same_bits(f32.cost_volume(a, b, 20, 0), want32)


def test_stereo_on_a_bf16_net():
    """McCnnStereo takes the bf16 net as it is: compute equals mc_disparity on the bf16 volumes."""
    net = Q.float_net(2, 96)
    left = Q.image("ragged", 0)
    right = np.roll(left, -3, axis=1)
    stereo = sm.McCnnStereo(net, sm.McCnnStereoParams(blur_sigma=2.0, blur_t=0.5))
    got, got_r = stereo.compute(left, right, 12, -2)
    assert got.shape == left.shape and got.dtype == np.float32
    fl, fr = net.features(left), net.features(right)
    m_r = right_min_disparity(12, -2)
    vl = mc_aggregate(net.join(fl, fr, 12, -2, a_is_left=True), left, right, -2, stereo.params)
    vr = mc_aggregate(net.join(fr, fl, 12, m_r, a_is_left=False), right, left, m_r, stereo.params)
    want, maps = mc_disparity(vl, vr, left, -2, stereo.params, stages=True)
    assert Q.same_bits(got, want[0]) and Q.same_bits(got_r, maps["wta_right"][0].astype(np.float32))
    # and it is the bf16 volume that went in: the bf16 twin's volume is within E_q of it, the f32 one is another
    assert not Q.same_bits(net.join(fl, fr, 12, -2), net.with_precision("f32").join(fl, fr, 12, -2))
    f32, _ = sm.McCnnStereo(net.with_precision("f32"), stereo.params).compute(left, right, 12, -2)
    print(f"McCnnStereo bf16 vs f32 on 37 x 70: {int((f32 != got).sum())} of {got.size} disparities differ")
