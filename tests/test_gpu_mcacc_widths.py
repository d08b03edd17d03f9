"""McCnnAccurate on the device at every hidden width, in both precisions, and at the row limits
(DESIGN.md §4.20, §4.21).  The width U is the one shape parameter that selects other compiled code:
U / 32 picks one of twelve k_ac_fused16 instantiations (each with its own unrolling and, for even
U / 32, the two-tile accumulator path), and in f32 it decides how k_ac_dense's 128-column tiles
fall: one partial tile, full tiles, or a partial tile behind full ones.  Everything here is bit for
bit -- dense integer scorers whose sums stay below 2^24 against exact numpy, the f32 device against
its twin's fmaf chains -- except the float nets in bf16, which keep the suite's E_q bound.  Then the
rows: the fused kernel's second trip through its row loop (more rows than a grid has workgroup
rows), and every declared row limit at the limit and one past it."""
import numpy as np
import pytest

import mcacc16_cases as Q
import mcacc_cases as C
import mccnn_cases as FAST
from stereo_match_amd import _lib

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


# ---- a. bf16: every instantiation of k_ac_fused16, on 11 x 37 with 6 planes from offset 1 (ragged in
# x, 32 + 5, and in d, 4 + 2; 2442 cells)
ODD = ("odd", 6, 1)
SWEEP16 = [(F, U) for U in Q.UNITS_INTERLEAVED for F in (2, 3, 4)]
_first16 = {}


def device_raw16(F, U, left):
    m = Q.dense_model(F, U)
    return m.join(Q.int_features("odd", 0), Q.int_features("odd", 1), ODD[1], ODD[2], a_is_left=left, raw=True)


@pytest.mark.parametrize("F,U", SWEEP16)
def test_bf16_every_width_bit_for_bit(F, U):
    """device == exact numpy == twin in both roles; the squashed volume on CUDA tensors equals the
    twin's.  The widths come from the ends inwards, so the engine repacks its bf16 weights from
    larger to smaller U and back."""
    geo, D, m0 = ODD
    m = Q.dense_model(F, U)
    fa, fb = Q.int_features(geo, 0), Q.int_features(geo, 1)
    for left in (True, False):
        want, info = Q.int_volume16(F, U, geo, D, m0, left)
        assert 0 < info["peak"] < 2**24
        if F >= 3:
            assert max(info["changed"]) > 0 and info["ties"] > 0
        got = device_raw16(F, U, left)
        assert got.shape == (1, D) + fa.shape[:2] and got.dtype == np.float32
        assert Q.same_bits(got[0], want), (left, int((got[0] != want).sum()))
        assert Q.same_bits(got, m.join(fa, fb, D, m0, a_is_left=left, raw=True, host=True))
        _first16.setdefault((F, U, left), got)
    squashed = m.join(cuda(fa), cuda(fb), D, m0).cpu().numpy()
    assert Q.same_bits(squashed, m.join(fa, fb, D, m0, host=True))


def test_bf16_first_width_again_after_the_sweep():
    """The first case once more, after every other width has been through the engine: the bits of
    the first run (when the sweep ran in this process) and of the exact values."""
    F, U = SWEEP16[0]
    for left in (True, False):
        got = device_raw16(F, U, left)
        assert Q.same_bits(got[0], Q.int_volume16(F, U, *ODD, left)[0])
        if (F, U, left) in _first16:
            assert np.array_equal(got.view(np.uint32), _first16[F, U, left].view(np.uint32))


# ---- b. bf16, float nets at tile parities no other float net runs (U / 32 = 2, 5, 8)
@pytest.mark.parametrize("U", [64, 160, 256])
def test_bf16_float_nets_within_e_q(U):
    """test_gpu_mcacc16.test_random_float_nets_within_e_q's bound and NaN-mask check.  The bound is
    loose; it is here so that a float net, not only integers, runs on even and odd U / 32 below 11.
    Measured ratios: DESIGN.md §4.21."""
    name, D, m0, F = "tiny", 20, 0, 3
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


# ---- c. f32: every width.  13 x 45 with 6 planes from offset -2: 3510 cells = 27 x 128 + 54 (a ragged
# row tile of the hidden layers), 585 pixels = 4 x 128 + 73 (of the projections)
SWEEP32 = [(F, U) for U in C.UNITS_INTERLEAVED for F in ((2, 3, 4) if U in (160, 256, 352) else (3,))]


@pytest.mark.parametrize("F,U", SWEEP32)
def test_f32_every_width_matches_twin(F, U):
    """cost_volume on numpy images and features + join on CUDA tensors equal the twin in both roles.
    At 352 units (two full column tiles and a partial one) also in passes of 129 cells."""
    name, D, m0 = "tiny", 6, -2
    m = C.model(2, F, U)
    a, b = C.image(name, 0), C.image(name, 1)
    fa, fb = m.features(cuda(a)), m.features(cuda(b))
    for left in (True, False):
        want = C.twin_volume(name, D, m0, F, U, left)
        got = m.cost_volume(a, b, D, m0, a_is_left=left)
        assert got.shape == (1, D) + a.shape and got.dtype == np.float32
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any() and not np.isnan(want).all()
        assert C.same_bits(got, want), (left, int((got != want).sum()))
        dev = m.join(fa, fb, D, m0, a_is_left=left).cpu().numpy()
        assert np.array_equal(np.isnan(dev), np.isnan(want)) and C.same_bits(dev, want)
        if U == 352:
            eng = m._engine()
            try:
                eng.set_tuning(eng.TUNE_MCACC_CHUNK, 129)
                many = m.cost_volume(a, b, D, m0, a_is_left=left)
            finally:
                eng.set_tuning(eng.TUNE_MCACC_CHUNK, 0)
            assert C.same_bits(many, got)


# ---- d. rows
def test_tall_second_trip_of_the_row_loop():
    """65538 rows: k_ac_fused16 runs 65535 workgroup rows and walks y += 65535, so rows 65535 .. are
    the second trip of its loop.  Exact values from numpy features and from CUDA tensors; and, so
    that a wrong reference could not hide it, those rows hold finite values that are not the first
    trip's (rows 0 ..) over again."""
    F, U, geo, D, m0 = 2, 32, "tall", 2, 0
    H = Q.GEOMETRY[geo][0]
    assert H > 65535
    m = Q.dense_model(F, U)
    fa, fb = Q.int_features(geo, 0), Q.int_features(geo, 1)
    want, info = Q.int_volume16(F, U, geo, D, m0)
    assert 0 < info["peak"] < 2**24
    got = m.join(fa, fb, D, m0, raw=True)
    dev = m.join(cuda(fa), cuda(fb), D, m0, raw=True).cpu().numpy()
    for v in (got, dev):
        assert v.shape == (1, D, H, 2)
        assert Q.same_bits(v[0], want), int((v[0] != want).sum())
        assert np.isfinite(v[0, 0, 65535:]).all() and np.isfinite(v[0, 1, 65535:, 1]).all()
        for y in range(65535, H):
            assert not np.array_equal(v[0, 0, y], v[0, 0, 0]) and not np.array_equal(v[0, 0, y], v[0, 0, y - 65535])
    assert Q.same_bits(m.join(fa, fb, D, m0, raw=True, host=True)[0], want)


def test_tall_f32_matches_twin():
    m = Q.dense_model(2, 32, "f32")
    fa, fb = Q.int_features("tall", 0), Q.int_features("tall", 1)
    want = m.join(fa, fb, 2, 0, raw=True, host=True)
    assert Q.same_bits(m.join(fa, fb, 2, 0, raw=True), want)
    assert Q.same_bits(m.join(cuda(fa), cuda(fb), 2, 0, raw=True).cpu().numpy(), want)


def column(H, seed):
    """An image of one column."""
    return np.random.default_rng(1200 + seed).integers(0, 256, (H, 1)).astype(np.uint8)


def test_accurate_features_row_limit():
    """sm_mcacc_features_device: 131070 rows (of one column, one convolution) equal the twin, one
    more is refused by name, and the context goes on working."""
    m = C.model(1, 1, 32)
    img = column(131070, 0)
    want = m.features(img, host=True)
    assert want.max() > 0
    assert np.array_equal(m.features(img), want)
    assert np.array_equal(m.features(cuda(img)).cpu().numpy(), want)
    over = column(131071, 1)
    for arg in (over, cuda(over)):
        with pytest.raises(_lib.SmError, match="at most 131070") as e:
            m.features(arg)
        assert e.value.code == _lib.SM_E_UNSUPPORTED
    assert np.array_equal(m.features(C.image("tiny", 0)), C.twin_features("tiny", 1, 0))


def test_fast_join_row_limit():
    """sm_mccnn_join_device: 65535 rows equal the twin, 65536 are refused by name."""
    m = FAST.model(1)
    rng = np.random.default_rng(77)
    fa, fb = (rng.standard_normal((65536, 1, 64)).astype(np.float32) for _ in range(2))
    want = m.join(fa[:65535], fb[:65535], 1, 0, host=True)
    assert np.isfinite(want).all()
    assert FAST.same_bits(m.join(fa[:65535], fb[:65535], 1, 0), want)
    assert FAST.same_bits(m.join(cuda(fa[:65535]), cuda(fb[:65535]), 1, 0).cpu().numpy(), want)
    for a, b in ((fa, fb), (cuda(fa), cuda(fb))):
        with pytest.raises(_lib.SmError, match="at most 65535") as e:
            m.join(a, b, 1, 0)
        assert e.value.code == _lib.SM_E_UNSUPPORTED
    fa, fb = FAST.twin_features("tiny", 1, 0), FAST.twin_features("tiny", 1, 1)
    assert FAST.same_bits(m.join(fa, fb, 5, -1), m.join(fa, fb, 5, -1, host=True))


def test_fast_features_row_limit():
    """sm_mccnn_features_device: its convolutions take a workgroup row per 8 image rows, so 524280
    rows are the most a grid holds.  That many equal the twin; one more is refused by name before
    anything is launched, and the context goes on working."""
    m = FAST.model(1)
    img = column(524280, 2)
    want = m.features(img, host=True)
    assert np.array_equal(m.features(img), want)
    assert np.array_equal(m.features(cuda(img)).cpu().numpy(), want)
    over = column(524281, 3)
    for arg in (over, cuda(over)):
        with pytest.raises(_lib.SmError, match="rows .at most 524280.") as e:
            m.features(arg)
        assert e.value.code == _lib.SM_E_UNSUPPORTED
    assert np.array_equal(m.features(FAST.image("tiny", 0)), FAST.twin_features("tiny", 1, 0))
