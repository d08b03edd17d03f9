"""MC-CNN's stereo method on the CPU: the plain C++ twin (sm_mcsgm_*_host) against
the numpy restatement tests/mcsgm_np.py, value for value and NaN for NaN; a hand-derived answer;
the properties the definition implies; and the conditions under which those comparisons mean
something, asserted so that none passes vacuously."""
import ctypes
import dataclasses

import numpy as np
import pytest

import mcsgm_cases as C
import mcsgm_np as N
import stereo_match_amd as sm
from stereo_match_amd import _lib

P = sm.McCnnStereoParams


@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_twin_aggregation_equals_numpy(shape):
    H, W, D, m = shape
    left, right, vl, _ = C.scene(*shape)
    want = N.aggregate(vl, left, right, m, C.DEFAULT)
    got = C.twin_aggregates(*shape)[0]
    assert got.shape == vl.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(vl))
    assert C.same_bits(got, want), f"{int((got != want).sum() - np.isnan(want).sum())} of {want.size} values differ"


@pytest.mark.parametrize("shape", [(33, 65, 65, 3), (40, 131, 37, -4)], ids=str)
def test_right_view(shape):
    """The right view: the images swapped and m_R = -(m + D) + 1."""
    H, W, D, m = shape
    left, right, _, vr = C.scene(*shape)
    want = N.aggregate(vr, right, left, C.right_m(D, m), C.DEFAULT)
    assert C.same_bits(C.twin_aggregates(*shape)[1], want)


def test_known_answer():
    """H = 1, W = 3, D = 3, m = 0; pi1 = 1, pi2 = 4, Q1 = 2, Q2 = 4, sgm_D = 0.5.  a = (0, 0, 255): no step
    between x = 0 and 1, a large one between 1 and 2; b = (0, 255, 255): the other way round.  One row,
    so r2 and r3 return V.
    r0: x = 0: (1, -, -).  x = 1: M = 1; d = 0 is mixed (P1 .5, P2 2): e = min(3, 1) = 1, L = (2 - 1) + 1
    = 2; d = 1 has b's second column outside, both steps small (P1 1, P2 4): e = min(5, 1 + 1) = 2,
    L = (5 - 1) + 2 = 6.  x = 2: M = 2; d = 0 mixed: e = min(4, 2, 6.5) = 2, L = 3; d = 1 both large
    (P1 .25, P2 1): e = min(3, 6, 2.25) = 2.25, L = (1 - 2) + 2.25 = 1.25; d = 2 mixed: e = min(4, 6.5)
    = 4, L = 4.
    r1: x = 2: (3, 1, 2).  x = 1: M = 1; d = 0 mixed: e = min(3, 3, 1.5) = 1.5, L = 2.5; d = 1 both
    large: e = min(2, 1, 3.25, 2.25) = 1, L = 5.  x = 0: M = 2.5; d = 0 mixed: e = min(4.5, 2.5, 5.5)
    = 2.5, L = (1 - 2.5) + 2.5 = 1.
    A = ((L0 + L1) + (V + V)) / 4."""
    nan = np.nan
    V = np.array([[[1, 2, 3]], [[nan, 5, 1]], [[nan, nan, 2]]], np.float32)
    a = np.array([[0, 0, 255]], np.uint8)
    b = np.array([[0, 255, 255]], np.uint8)
    p = P(pi1=1, pi2=4, sgm_q1=2, sgm_q2=4, sgm_v=2, sgm_d=0.5)
    want = np.array([[[1, 2.125, 3]], [[nan, 5.25, 1.0625]], [[nan, nan, 2.5]]], np.float32)
    assert C.same_bits(sm.mc_aggregate(V, a, b, 0, p, host=True), want)
    assert C.same_bits(N.aggregate(V, a, b, 0, p), want)


def dyadic_volume(shape, seed):
    """Costs on the grid k / 8, k < 256: every V - M, (V - M) + M and 4 V is exact in float32."""
    H, W, D, m = shape
    rng = np.random.default_rng(seed)
    V = (rng.integers(0, 256, (D, H, W)) / 8).astype(np.float32)
    V[np.isnan(C.scene(*shape)[2])] = np.nan
    return V


def test_zero_penalties_return_the_volume():
    """pi1 = pi2 = 0: e = M on every path, (V - M) + M = V and the average of four equal values is V.
    That identity holds in float32 where V - M is exact, so the costs lie on a dyadic grid."""
    shape = (33, 65, 65, 3)
    left, right = C.scene(*shape)[:2]
    V = dyadic_volume(shape, 1)
    got = sm.mc_aggregate(V, left, right, shape[3], P(pi1=0, pi2=0), host=True)
    assert C.same_bits(got, V)


def test_vertical_flip():
    """Flipping V, a and b along y flips A: r2 and r3 change places and L2 + L3 commutes."""
    shape = (33, 65, 65, 3)
    left, right, vl, _ = C.scene(*shape)
    flipped = sm.mc_aggregate(np.ascontiguousarray(vl[:, ::-1]), left[::-1], right[::-1], shape[3], C.DEFAULT, host=True)
    assert C.same_bits(flipped[:, ::-1], C.twin_aggregates(*shape)[0])
    assert not C.same_bits(flipped, C.twin_aggregates(*shape)[0])


def test_two_iterations_are_two_calls():
    shape = (33, 65, 65, 3)
    left, right, vl, _ = C.scene(*shape)
    once = C.twin_aggregates(*shape)[0]
    twice = sm.mc_aggregate(once, left, right, shape[3], C.DEFAULT, host=True)
    assert C.same_bits(sm.mc_aggregate(vl, left, right, shape[3], P(sgm_i=2), host=True), twice)
    assert C.same_bits(N.aggregate(vl, left, right, shape[3], P(sgm_i=2)), twice)
    assert not C.same_bits(once, twice)


def test_all_penalty_classes_occur():
    left, right, vl, _ = C.scene(*C.SCENE)
    classes = [0, 0, 0]
    N.aggregate(vl, left, right, C.SCENE[3], C.DEFAULT, classes)
    assert min(classes) > 0.02 * sum(classes), classes
    p1h, p1v, _ = N.penalties(C.DEFAULT)
    assert np.all(p1h != p1v)
    # and the vertical constant matters: another sgm_V gives another volume
    other = sm.mc_aggregate(vl, left, right, C.SCENE[3], P(sgm_v=1.0), host=True)
    assert not C.same_bits(other, C.twin_aggregates(*C.SCENE)[0])


@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_twin_stages_equal_numpy(shape):
    H, W, D, m = shape
    al, ar = C.stage_inputs(*shape)
    want = N.disparity(al, ar, C.scene(*shape)[0], m, C.SMALL_BLUR)
    disp, maps = C.twin_disparity(*shape)
    assert set(maps) == set(sm.mcstereo.STAGES)
    for k in sm.mcstereo.STAGES:
        assert maps[k].dtype == want[k].dtype and C.same_bits(maps[k], want[k]), k
    assert disp.dtype == np.float32 and C.same_bits(disp, want["out"])
    assert C.same_bits(disp == np.float32(m - 1), want["filled"] == m - 1)  # invalid stays invalid, valid stays valid
    assert C.same_bits(sm.mc_disparity(al, ar, C.scene(*shape)[0], m, C.SMALL_BLUR, host=True), disp)


def test_default_bilateral_window():
    """The default sigma 7.74: a 49 x 49 window, larger than the image in one direction."""
    shape = (9, 130, 256, -100)
    al, ar = C.stage_inputs(*shape)
    want = N.disparity(al, ar, C.scene(*shape)[0], shape[3], C.DEFAULT)
    got = sm.mc_disparity(al, ar, C.scene(*shape)[0], shape[3], C.DEFAULT, host=True)
    assert C.same_bits(got, want["out"])
    assert not C.same_bits(got, want["median"])


def test_scene_conditions():
    """The scene exercises every branch of the interpolation and every guard of the sub-pixel step."""
    H, W, D, m = C.SCENE
    al, ar = C.stage_inputs(*C.SCENE)
    r = N.disparity(al, ar, C.scene(*C.SCENE)[0], m, C.SMALL_BLUR)
    st = r["status"]
    for code in (N.CORRECT, N.MISMATCH, N.OCCLUDED):
        assert (st == code).mean() >= 0.01, (code, float((st == code).mean()))
    supported = (st == N.CORRECT).any(axis=1)[:, None]  # rows with a correct pixel
    lonely = r["none_left"] & (st == N.OCCLUDED)
    assert (lonely & supported).any()   # nothing to the left: the nearest one to the right
    assert (lonely & ~supported).any()  # nothing in the row: the pixel's own value
    invalid = r["out"] == np.float32(m - 1)
    assert invalid.any() and (r["wta_left"] == m - 1).sum() > invalid.sum()  # one stays invalid, one is filled
    assert ((r["hits"] >= 0) & (r["hits"] < 16)).any()
    assert (r["filled"] != r["wta_left"]).any()
    for name, hit in r["guards"].items():
        assert hit.any(), name
    assert (r["subpixel"] != r["filled"].astype(np.float32)).any()
    assert (r["median"] != r["subpixel"]).any() and (r["out"] != r["median"]).any()
    # the bilateral threshold rejects some taps and keeps others
    ta = N.normalise(C.scene(*C.SCENE)[0])
    step = np.abs(ta[:, 1:] - ta[:, :-1])
    assert (step < C.SMALL_BLUR.blur_t).any() and (step >= C.SMALL_BLUR.blur_t).any()


def test_batch_and_strides_on_the_twin():
    shape = (33, 65, 65, 3)
    H, W, D, m = shape
    left, right, vl, _ = C.scene(*shape)
    other = C.scene(33, 65, 65, 3, seed=8)
    vol = np.stack([vl, other[2]])
    wide = np.zeros((2, 2, H + 2, W + 9), np.uint8)
    wide[0, :, 1:H + 1, 4:4 + W] = np.stack([left, other[0]])
    wide[1, :, 1:H + 1, 4:4 + W] = np.stack([right, other[1]])
    va, vb = wide[0, :, 1:H + 1, 4:4 + W], wide[1, :, 1:H + 1, 4:4 + W]
    got = _lib.mcsgm_aggregate_host(vol, va, vb, va.strides[0], va.strides[1], m, C.DEFAULT.c_struct())
    assert C.same_bits(got[0], C.twin_aggregates(*shape)[0])
    assert C.same_bits(got[1], sm.mc_aggregate(other[2], other[0], other[1], m, C.DEFAULT, host=True))
    assert C.same_bits(sm.mc_aggregate(vol, np.stack([left, other[0]]), np.stack([right, other[1]]), m, host=True), got)


def test_arguments():
    for bad in (dict(pi1=-1), dict(pi2=float("nan")), dict(sgm_q1=0), dict(sgm_q2=float("inf")), dict(sgm_v=-2),
                dict(sgm_d=0), dict(sgm_i=0), dict(sgm_i=1.5), dict(blur_sigma=0), dict(blur_t=0), dict(blur_sigma=17),
                dict(blur_t=1e39)):
        with pytest.raises(ValueError):
            P(**bad)
    assert dataclasses.asdict(P()) == dict(pi1=4.0, pi2=55.72, sgm_q1=3.0, sgm_q2=2.5, sgm_v=1.5, sgm_d=0.02, sgm_i=1,
                                           blur_sigma=7.74, blur_t=5.0)
    d = _lib.SmMcsgmParams()
    assert _lib.load().sm_mcsgm_default_params(ctypes.byref(d)) == 0
    assert all(getattr(d, k) == getattr(P().c_struct(), k) for k, _ in d._fields_)
    left, right, vl, _ = C.scene(5, 3, 20, 0)
    with pytest.raises(ValueError, match="float32"):
        sm.mc_aggregate(vl.astype(np.float64), left, right, 0, host=True)
    with pytest.raises(ValueError, match="shape"):
        sm.mc_aggregate(vl, left[:, :2], right, 0, host=True)
    with pytest.raises(ValueError, match="uint8"):
        sm.mc_aggregate(vl, left.astype(np.int32), right, 0, host=True)
    with pytest.raises(ValueError, match="McCnnStereoParams"):
        sm.mc_aggregate(vl, left, right, 0, dict(pi1=1), host=True)
    with pytest.raises(ValueError, match="2\\^23"):
        sm.mc_disparity(vl, vl, left, 2**23, host=True)
    with pytest.raises(ValueError, match="planes"):
        sm.mc_aggregate(np.zeros((257, 2, 2), np.float32), left[:2, :2], right[:2, :2], 0, host=True)
    # an output that overlaps the input is refused
    buf = np.array(vl)
    prm = P().c_struct()
    rc = _lib.load().sm_mcsgm_aggregate_host(buf.ctypes.data, left.ctypes.data, right.ctypes.data, 1, 15, 5, 3, 3, 20, 0,
                                             ctypes.byref(prm), buf.ctypes.data)
    assert rc == _lib.SM_E_ARG and b"overlaps" in _lib.load().sm_last_error(None)
    assert C.same_bits(buf, vl)
