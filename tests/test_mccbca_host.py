"""Cross-based cost aggregation on the CPU: the plain C++ twin (sm_mccbca_*_host)
against the numpy restatement tests/mccbca_np.py, bit for bit; a hand-derived answer; the properties
the definition implies; and the conditions under which those comparisons mean something, asserted
so that none passes vacuously."""
import ctypes
import dataclasses

import numpy as np
import pytest

import mccbca_cases as C
import mccbca_np as N
import mccnn_cases as M
import stereo_match_amd as sm
from stereo_match_amd import _lib

P = sm.McCnnCrossParams
FMAX = float(np.finfo(np.float32).max)


@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_twin_arms_equal_numpy(shape):
    left = C.scene(*shape)[0]
    got = C.twin_arms(shape)
    assert got.dtype == np.uint8 and got.shape == (4,) + left.shape
    assert C.same_bits(got, N.arms(left, 5, C.TAU1))


def test_arm_conditions():
    """In each direction each of the three reasons to stop (the cap L1, the border, tau1) ends at
    least 1 % of the arms."""
    reasons = []
    N.arms(C.scene(*C.SCENE)[0], 5, C.TAU1, reasons)
    assert len(reasons) == 4
    for s, why in enumerate(reasons):
        for reason in (N.CAP, N.BORDER, N.TAU):
            share = float((why == reason).mean())
            assert share >= 0.01, (s, reason, share)


@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_twin_aggregation_equals_numpy(shape):
    H, W, D, m = shape
    left, right, vl, _ = C.scene(*shape)
    got = C.twin_cross(shape)
    assert got.shape == vl.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(vl))
    want = N.aggregate(vl, left, right, m, 5, C.TAU1)
    assert C.same_bits(got, want), f"{int((got != want).sum() - np.isnan(want).sum())} of {want.size} values differ"


@pytest.mark.parametrize("l1", C.L1S)
def test_every_arm_length(l1):
    H, W, D, m = C.SCENE
    left, right, vl, _ = C.scene(*C.SCENE)
    assert C.same_bits(C.twin_arms(C.SCENE, l1), N.arms(left, l1, C.TAU1))
    assert C.same_bits(C.twin_cross(C.SCENE, l1), N.aggregate(vl, left, right, m, l1, C.TAU1))


def test_aggregation_conditions():
    """Both images shorten arms, and some regions are a single cell."""
    H, W, D, m = C.SCENE
    left, right, vl, _ = C.scene(*C.SCENE)
    st = {}
    N.cross(vl, left, right, m, 5, C.TAU1, st)
    ex = st["exists"]
    a, b = st["arm_a"][:, ex], st["arm_b"][:, ex]  # [side, cell]
    assert (a < b).mean() >= 0.05, float((a < b).mean())
    assert (b < a).mean() >= 0.05, float((b < a).mean())
    single = (np.minimum(a, b).sum(axis=0) == 0).mean()
    assert single >= 0.01, float(single)
    assert not C.same_bits(C.twin_cross(C.SCENE), vl)


@pytest.mark.parametrize("shape", [(33, 65, 65, 3), (40, 131, 37, -4)], ids=str)
def test_right_view(shape):
    H, W, D, m = shape
    left, right, _, vr = C.scene(*shape)
    want = N.aggregate(vr, right, left, C.right_m(D, m), 5, C.TAU1)
    assert C.same_bits(C.twin_cross(shape, view=1), want)


def test_three_iterations_are_three_calls():
    H, W, D, m = shape = (33, 65, 65, 3)
    left, right, vl, _ = C.scene(*shape)
    v = vl
    for _ in range(3):
        v = sm.mc_cross_aggregate(v, left, right, m, C.params(), host=True)
    assert C.same_bits(C.twin_cross(shape, iterations=3), v)
    assert C.same_bits(N.aggregate(vl, left, right, m, 5, C.TAU1, 3), v)
    assert not C.same_bits(C.twin_cross(shape), v)


def test_l1_of_one_returns_the_input():
    assert C.same_bits(C.twin_cross(C.SCENE, 1), C.scene(*C.SCENE)[2])
    assert not C.twin_arms(C.SCENE, 1).any()


def border_arms(H, W, l1):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.minimum(np.stack([xs, W - 1 - xs, ys, H - 1 - ys]), l1 - 1).astype(np.uint8)


@pytest.mark.parametrize("constant", [False, True], ids=["tau1_max", "constant_image"])
def test_unbounded_arms(constant):
    """tau1 = FLOAT32_MAX, or a constant image (the table 0) at any tau1: the arms are min(l1 - 1,
    distance to the border), and a volume that is 0.375 wherever a cell exists stays 0.375 there
    (0.375 k is exact for k <= 63^2, and so is the division)."""
    H, W, D, m = shape = (33, 65, 65, 3)
    left, right, vl, _ = C.scene(*shape)
    if constant:
        left = right = np.full((H, W), 77, np.uint8)
    p = P(l1=14, tau1=C.TAU1 if constant else FMAX)
    assert C.same_bits(sm.mc_cross_arms(left, p, host=True), border_arms(H, W, 14))
    V = np.where(np.isnan(vl), np.float32(np.nan), np.float32(0.375)).astype(np.float32)
    assert C.same_bits(sm.mc_cross_aggregate(V, left, right, m, p, 2, host=True), V)


def test_known_answer():
    """D = 1, H = 3, W = 3, m = 0, l1 = 2 (arms of 0 or 1), tau1 = 0.5; grey levels 0 / 255 and 5 / 200
    are far more than tau1 apart after the table, equal ones are 0 apart.
    a = (0 0 255 / 0 0 255 / 255 255 255), b = (5 5 5 / 5 5 5 / 200 200 200).
    Arms (l r u d) of a:  (0,0) 0101  (0,1) 1001  (0,2) 0001 / (1,0) 0110  (1,1) 1010  (1,2) 0011 /
    (2,0) 0100  (2,1) 1100  (2,2) 1010.  b's rows are constant, so its horizontal arms only meet the
    border; vertically row 2 is cut off: u = 0 in row 2 and d = 0 in row 1.  The minimum changes a's
    arms in two places: (1,2) d 1 -> 0 and (2,2) u 1 -> 0.
    C = (1 2 4 / 8 16 32 / 64 128 256).  S, n_h:  3,2  3,2  4,1 / 24,2  24,2  32,1 / 192,2  448,3  384,2.
    T / N:  (0,0) (3 + 24) / 4;  (0,1) the same;  (0,2) (4 + 32) / 2;  (1,0), (1,1) u = 1, d = 0: 27 / 4;
    (1,2) u = 1, d = 0: 36 / 2;  row 2 has u = d = 0: 192 / 2, 448 / 3, 384 / 2."""
    a = np.array([[0, 0, 255], [0, 0, 255], [255, 255, 255]], np.uint8)
    b = np.array([[5, 5, 5], [5, 5, 5], [200, 200, 200]], np.uint8)
    V = np.array([[[1, 2, 4], [8, 16, 32], [64, 128, 256]]], np.float32)
    p = P(l1=2, tau1=0.5)
    want = np.array([[[6.75, 6.75, 18], [6.75, 6.75, 18], [96, np.float32(448) / np.float32(3), 192]]], np.float32)
    assert C.same_bits(sm.mc_cross_aggregate(V, a, b, 0, p, host=True), want)
    assert C.same_bits(N.aggregate(V, a, b, 0, 2, 0.5), want)
    arms_a = np.array([[[0, 1, 0], [0, 1, 0], [0, 1, 1]], [[1, 0, 0], [1, 0, 0], [1, 1, 0]],
                       [[0, 0, 0], [1, 1, 1], [0, 0, 1]], [[1, 1, 1], [0, 0, 1], [0, 0, 0]]], np.uint8)
    assert C.same_bits(sm.mc_cross_arms(a, p, host=True), arms_a)


def test_vertical_flip():
    """The flip swaps up and down.  It reverses the order of the vertical adds, so the aggregation
    commutes with it where those sums are exact: costs on the grid k / 8, k < 256."""
    H, W, D, m = shape = (33, 65, 65, 3)
    left, right, vl, _ = C.scene(*shape)
    arms = C.twin_arms(shape)
    assert C.same_bits(sm.mc_cross_arms(left[::-1], C.params(), host=True), arms[[0, 1, 3, 2]][:, ::-1])
    assert (arms[2] != arms[3]).any()
    rng = np.random.default_rng(3)
    V = (rng.integers(0, 256, vl.shape) / 8).astype(np.float32)
    V[np.isnan(vl)] = np.nan
    straight = sm.mc_cross_aggregate(V, left, right, m, C.params(), host=True)
    flipped = sm.mc_cross_aggregate(np.ascontiguousarray(V[:, ::-1]), left[::-1], right[::-1], m, C.params(), host=True)
    assert C.same_bits(flipped[:, ::-1], straight)
    assert not C.same_bits(flipped, straight)


def test_cells_that_do_not_exist_keep_their_bits():
    H, W, D, m = C.SCENE
    left, right, vl, _ = C.scene(*C.SCENE)
    rng = np.random.default_rng(5)
    gone = np.isnan(vl)
    bits = vl.view(np.uint32).copy()
    bits[gone] = rng.integers(0, 2**32, int(gone.sum()), dtype=np.uint64).astype(np.uint32)  # NaNs and infinities among them
    V = bits.view(np.float32)
    got = sm.mc_cross_aggregate(V, left, right, m, C.params(), host=True)
    assert np.array_equal(got.view(np.uint32)[gone], bits[gone])
    assert np.array_equal(got.view(np.uint32)[~gone], C.twin_cross(C.SCENE).view(np.uint32)[~gone])


def test_a_nan_reaches_the_cells_whose_region_holds_it():
    H, W, D, m = C.SCENE
    left, right, vl, _ = C.scene(*C.SCENE)
    st = {}
    N.cross(vl, left, right, m, 5, C.TAU1, st)
    lo = np.minimum(st["arm_a"], st["arm_b"])  # [side, D, H, W]
    d0 = 11
    y0, x0 = np.unravel_index(np.argmax(np.where(st["exists"][d0], lo[:, d0].sum(axis=0), -1)), (H, W))  # the widest region
    assert st["exists"][d0, y0, x0]
    ys, xs = np.mgrid[0:H, 0:W]
    in_row = st["exists"][d0, y0] & (xs[0] - lo[0, d0, y0] <= x0) & (x0 <= xs[0] + lo[1, d0, y0])  # S(x, y0, d0) holds it
    want = np.zeros(vl.shape, bool)
    want[d0] = in_row[None, :] & (ys - lo[2, d0] <= y0) & (y0 <= ys + lo[3, d0])
    assert want.sum() > 4 and want[d0, y0, x0]
    V = vl.copy()
    V[d0, y0, x0] = np.nan
    got = sm.mc_cross_aggregate(V, left, right, m, C.params(), host=True)
    assert np.array_equal(np.isnan(got) & ~np.isnan(vl), want)
    keep = ~want
    assert C.same_bits(got[keep], C.twin_cross(C.SCENE)[keep])
    assert C.same_bits(got, N.aggregate(V, left, right, m, 5, C.TAU1))


def test_batch_and_strides_on_the_twin():
    H, W, D, m = shape = (33, 65, 65, 3)
    one, two = C.scene(*shape), C.scene(*shape, seed=8)
    vol = np.stack([one[2], two[2]])
    wide = np.zeros((2, 2, H + 2, W + 9), np.uint8)
    wide[0, :, 1:H + 1, 4:4 + W] = np.stack([one[0], two[0]])
    wide[1, :, 1:H + 1, 4:4 + W] = np.stack([one[1], two[1]])
    va, vb = wide[0, :, 1:H + 1, 4:4 + W], wide[1, :, 1:H + 1, 4:4 + W]
    prm = C.params().c_struct()
    got = _lib.mccbca_aggregate_host(vol, va, vb, va.strides[0], va.strides[1], m, prm, 1)
    assert C.same_bits(got[0], C.twin_cross(shape))
    assert C.same_bits(got[1], sm.mc_cross_aggregate(two[2], two[0], two[1], m, C.params(), host=True))
    arms = _lib.mccbca_arms_host(va, va.strides[0], va.strides[1], prm)
    assert C.same_bits(arms[0], C.twin_arms(shape)) and C.same_bits(arms[1], N.arms(two[0], 5, C.TAU1))


def test_stereo_without_and_with_cross():
    """cross=None is the method without the step; with it, compute is the hand-composed chain."""
    net = M.model(4)
    left = M.image("tiny", 0)
    right = np.roll(left, -3, axis=1)
    D, m = 12, -2
    m_r = sm.mcstereo.right_min_disparity(D, m)
    prm = sm.McCnnStereoParams(blur_sigma=2.0, blur_t=0.5)
    vl, vr = net.cost_volume(left, right, D, m, host=True), net.cost_volume(right, left, D, m_r, host=True)

    def chain(cross):
        vols = []
        for v, a, b, mm in ((vl, left, right, m), (vr, right, left, m_r)):
            if cross:
                v = sm.mc_cross_aggregate(v, a, b, mm, cross, cross.i1, host=True)
            v = sm.mc_aggregate(v, a, b, mm, prm, host=True)
            if cross:
                v = sm.mc_cross_aggregate(v, a, b, mm, cross, cross.i2, host=True)
            vols.append(v)
        disp, maps = sm.mc_disparity(vols[0], vols[1], left, m, prm, host=True, stages=True)
        return disp.reshape(left.shape), maps["wta_right"].astype(np.float32).reshape(left.shape)  # one image: no batch axis

    plain = sm.McCnnStereo(net, prm).compute(left, right, D, m, host=True)
    none = sm.McCnnStereo(net, prm, cross=None).compute(left, right, D, m, host=True)
    want = chain(None)
    for got in (plain, none):
        assert C.same_bits(got[0], want[0]) and C.same_bits(got[1], want[1])
    cross = P(l1=5, tau1=0.3, i1=1, i2=1)
    got = sm.McCnnStereo(net, prm, cross).compute(left, right, D, m, host=True)
    want_c = chain(cross)
    assert C.same_bits(got[0], want_c[0]) and C.same_bits(got[1], want_c[1])
    assert not C.same_bits(want_c[0], want[0])


def test_arguments():
    for bad in (dict(l1=0), dict(l1=33), dict(l1=2.5), dict(tau1=0), dict(tau1=float("nan")), dict(tau1=float("inf")),
                dict(tau1=-1), dict(tau1=1e39), dict(i1=17), dict(i1=-1), dict(i2=17), dict(i2=True)):
        with pytest.raises(ValueError):
            P(**bad)
    assert dataclasses.asdict(P()) == dict(l1=5, tau1=0.13, i1=2, i2=0)
    d = _lib.SmMccbcaParams()
    lib = _lib.load()
    assert lib.sm_mccbca_default_params(ctypes.byref(d)) == 0
    assert all(getattr(d, k) == getattr(P().c_struct(), k) for k, _ in d._fields_)
    left, right, vl, _ = C.scene(5, 3, 20, 0)
    with pytest.raises(ValueError, match="float32"):
        sm.mc_cross_aggregate(vl.astype(np.float64), left, right, 0, host=True)
    with pytest.raises(ValueError, match="shape"):
        sm.mc_cross_aggregate(vl, left[:, :2], right, 0, host=True)
    with pytest.raises(ValueError, match="uint8"):
        sm.mc_cross_aggregate(vl, left.astype(np.int32), right, 0, host=True)
    with pytest.raises(ValueError, match="uint8"):
        sm.mc_cross_arms(left.astype(np.float32), host=True)
    with pytest.raises(ValueError, match="uint8"):
        sm.mc_cross_arms(left[0], host=True)
    with pytest.raises(ValueError, match="McCnnCrossParams"):
        sm.mc_cross_aggregate(vl, left, right, 0, sm.McCnnStereoParams(), host=True)
    with pytest.raises(ValueError, match="McCnnCrossParams"):
        sm.McCnnStereo(M.model(4), cross=dict(l1=3))
    with pytest.raises(ValueError, match="planes"):
        sm.mc_cross_aggregate(np.zeros((257, 2, 2), np.float32), left[:2, :2], right[:2, :2], 0, host=True)
    for it in (0, 17, 1.5):
        with pytest.raises(ValueError, match="iterations"):
            sm.mc_cross_aggregate(vl, left, right, 0, iterations=it, host=True)
    # the raw ABI refuses the same values, and an output that overlaps the input
    buf, out = np.array(vl), np.empty_like(vl)
    arms = np.empty((4, 5, 3), np.uint8)

    def raw(prm, iterations=1, dst=out):
        return lib.sm_mccbca_aggregate_host(buf.ctypes.data, left.ctypes.data, right.ctypes.data, 1, 15, 5, 3, 3, 20, 0,
                                            ctypes.byref(prm), iterations, dst.ctypes.data)

    S = _lib.SmMccbcaParams
    assert raw(S(5, 0.13, 2, 0)) == 0
    for prm in (S(0, 0.13, 2, 0), S(33, 0.13, 2, 0), S(5, 0.0, 2, 0), S(5, float("nan"), 2, 0), S(5, float("inf"), 2, 0),
                S(5, 0.13, 17, 0), S(5, 0.13, 0, -1)):
        assert raw(prm) == _lib.SM_E_ARG
        assert lib.sm_mccbca_arms_host(left.ctypes.data, 1, 15, 5, 3, 3, ctypes.byref(prm), arms.ctypes.data) == _lib.SM_E_ARG
    assert raw(S(5, 0.13, 2, 0), iterations=0) == _lib.SM_E_ARG
    assert raw(S(5, 0.13, 2, 0), dst=buf) == _lib.SM_E_ARG and b"overlaps" in lib.sm_last_error(None)
    assert C.same_bits(buf, vl)
