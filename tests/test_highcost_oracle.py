"""The inputs of test_gpu_highcost.py are what they claim (CPU only): the two oracles agree bit for
bit on every parameter set at the top of the u16 range, and the `mixed` pairs and `high_volume`
volumes really put cells at and above 65535, between 32767 and 65535, and whole pixels at the
WTA's clamp, while leaving enough pixels valid that a wrong sum shows in the map."""
import numpy as np
import pytest

import highcost as hc
from oracle import ref_c, sgm_np

_CASES = []
for _i, (_name, _mode, _D, _minD) in enumerate((n, m, D, md) for n in hc.FAST_SETS for m in (5, 8)
                                                for D in (16, 64, 128) for md in (0, -5)):
    # both variants and all three inputs under every parameter set and mode
    _CASES.append((_name, _mode, _D, _minD, ("open", "strict")[(_i + _i // 6) % 2], hc.INPUTS[_i % 3]))


@pytest.mark.parametrize("name,mode,D,minD,variant,inp", _CASES,
                         ids=["%s-p%d-D%d-m%d-%s-%s" % c for c in _CASES])
def test_oracles_agree(name, mode, D, minD, variant, inp):
    left, right = hc.pair(inp, 23, 3 * D + 257, D)
    p = hc.params(name, D, mode, minD, variant)
    assert hc.path_max(name) <= 16383
    assert np.array_equal(sgm_np.compute(left, right, p), ref_c.compute(left, right, p))


def test_case_list_covers_variants_and_inputs():
    for name in hc.FAST_SETS:
        for mode in (5, 8):
            mine = [c for c in _CASES if c[0] == name and c[1] == mode]
            assert {c[4] for c in mine} == set(hc.VARIANTS) and {c[5] for c in mine} == set(hc.INPUTS)
            assert {(c[2], c[3]) for c in mine} == {(D, md) for D in (16, 64, 128) for md in (0, -5)}


@pytest.mark.parametrize("mode", [5, 8])
def test_wide_bottom_is_outside_the_numpy_oracle(mode):
    """path_max 16384: sgm_np refuses, the C oracle (OpenCV's saturating int16 arithmetic) computes."""
    D = 64
    left, right = hc.pair("mixed40", 23, 3 * D + 257, D)
    p = hc.params("WIDE_BOTTOM", D, mode)
    assert hc.path_max("WIDE_BOTTOM") == 16384
    with pytest.raises(ValueError, match="outside the int16-exact range"):
        sgm_np.compute(left, right, p)
    out = ref_c.compute(left, right, p)
    assert out.shape == left.shape and (out >= 0).any()


def test_parameter_table():
    for name, (bs, P1, P2, pm) in hc.SETS.items():
        assert hc.path_max(name) == pm and P1 < P2
    # 13107 / 13108: the last value whose five-path sum cannot reach 65536, and the first that can
    assert 5 * hc.path_max("ATOM_TOP") == 65535 and 5 * hc.path_max("SAT_BOTTOM") > 65535
    assert hc.path_max("FAST_TOP") == hc.path_max("FLAT_TOP") == hc.path_max("BS9") == 16383


@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("stripe,H,W,D,seed", hc.FLOOR_INPUTS, ids=["s%d-%dx%d-D%d-seed%d" % c for c in hc.FLOOR_INPUTS])
def test_mixed_floors(stripe, H, W, D, seed, mode):
    cs, vo = hc.assert_floors(stripe, H, W, D, seed, mode)
    print({k: round(v, 4) for k, v in cs.items()}, "open valid", round(vo, 4))


@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("name", ["P12288_100", "P12288_flat"])
@pytest.mark.parametrize("lo", hc.VOLUME_LO)
@pytest.mark.parametrize("D", [32, 37])
def test_volume_floors(D, lo, name, mode):
    c = hc.volume_coverage(hc.high_volume(D, 24, 150, lo), hc.volume_params(name, D, mode))
    print({k: round(v, 4) for k, v in c.items()})
    assert c["max_L"] == 16383, c
    assert c["sat_full"] >= hc.FLOOR_VOLUME_SAT, c


@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("name", list(hc.VOLUME_SETS))
@pytest.mark.parametrize("lo", hc.VOLUME_LO)
@pytest.mark.parametrize("D", [32, 37])
def test_volume_oracles_agree(D, lo, name, mode):
    vol = hc.high_volume(D, 24, 150, lo)
    p = hc.volume_params(name, D, mode)
    assert vol.min() >= 0 and vol.max() <= 4095 and np.array_equal(vol, np.rint(vol))  # nothing to clamp
    assert np.array_equal(sgm_np.compute_volume(vol, p, 0.0, 1.0), ref_c.compute_volume(vol, p, 0.0, 1.0))


def test_cost_volumes_of_the_two_oracles():
    """ref_c.cost_volume is OpenCV's row buffer, which carries the P2 seed; sgm_np's is C itself."""
    left, right = hc.pair("mixed40", 40, 200, 32)
    for mode in (5, 8):
        p = hc.params("FAST_TOP", 32, mode)
        prm = sgm_np.normalize_params(p)
        C = sgm_np.cost_volume(left, right, prm)
        assert np.array_equal(ref_c.cost_volume(left, right, p).astype(np.int64) - prm["P2"], C)
        assert C.max() >= 7500  # of the 49 * 189 = 9261 a 7 x 7 block can cost: above any parity_params path


def test_saw_bands_is_saturated_and_flat():
    """The pair of the open-carry test: columns constant down the rows over 200-column bands, costs
    at the top."""
    left, right = hc.pair("saw_bands", 23, 641, 128)
    for band in (slice(0, 200), slice(400, 600)):
        assert (left[:, band] == left[0, band]).all() and (right[:, band] == right[0, band]).all()
    assert not (left[:, 200:400] == left[0, 200:400]).all()
    for name in ("FAST_TOP", "BS9", "BS3"):
        for mode in (5, 8):
            p = hc.params(name, 128, mode)
            assert np.array_equal(sgm_np.compute(left, right, p), ref_c.compute(left, right, p))
    prm = sgm_np.normalize_params(hc.params("FAST_TOP", 128, 5))
    c = hc.coverage(sgm_np.cost_volume(left, right, prm), prm["P1"], prm["P2"], 5)
    print(c)
    assert c["sat5"] >= hc.FLOOR_SAT5 and c["max_L"] >= hc.FLOOR_MAX_L
