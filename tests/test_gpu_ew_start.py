"""The cost-derived start state of the in-sweep E/W strip segments (SM_TUNE_EW_START, DESIGN.md
§4.4): every start state and warmup is bit-exact against the C oracle (the patch pass repairs
what started wrong), and the cost-derived state at 9 warmup columns leaves the patch pass no
more to repair than the zero state at 18."""
import functools

import numpy as np
import pytest

from oracle import ref_c
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

SWEEP8 = 16384  # sm_api.hip DBG_SWEEP8: the fused sweeps at any pair count
GUESS, ZERO = 1, -1  # SM_TUNE_EW_START


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _params(cost, D, mode, minD=0, bs=5, **kw):
    if cost:
        return dict(synthetic.headline_params(D), minDisparity=minD, mode=mode, **kw)
    return dict(dict(synthetic.parity_params(D), minDisparity=minD, mode=mode, blockSize=bs, P1=8 * bs * bs,
                     P2=32 * bs * bs), **kw)


def _run(eng, left, right, p, **tune):
    eng.set_debug_flags(SWEEP8)
    for k, v in tune.items():
        eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), v)
    try:
        return eng.compute(left, right, synthetic.to_sm_params(p))
    finally:
        eng.set_debug_flags(0)
        for k in tune:
            eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), 0)


@functools.lru_cache(maxsize=None)
def _pair(H, W, D, seed):
    left, right, _ = synthetic.random_dot_pair(H, W, D, seed=seed)
    return left, right


@functools.lru_cache(maxsize=None)
def _expected(H, W, D, seed, pkey):
    left, right = _pair(H, W, D, seed)
    return ref_c.compute(left, right, dict(pkey))


def _check_random(eng, H, W, D, p, seed, **tune):
    left, right = _pair(H, W, D, seed)
    exp = _expected(H, W, D, seed, tuple(sorted(p.items())))
    c0 = eng.counters()
    out = _run(eng, left, right, p, **tune)
    assert np.array_equal(out, exp), f"{np.sum(out != exp)} px differ"
    assert eng.counters()["line_groups"] > c0["line_groups"], "the in-sweep lines ran"


# strip widths of the wide MODE 3 instances: 9 own waves x 64 / VL columns (16-lane lines at
# D = 128, 8-lane lines at D = 32)
CW = {128: 36, 32: 72}
CONFIGS = [(1, 8, 128), (1, 8, 32), (0, 5, 128), (0, 8, 128)]  # (cost, paths, D)


@pytest.mark.parametrize("cost,mode,D", CONFIGS)
@pytest.mark.parametrize("wide", [True, False], ids=["strips4", "strip1"])
@pytest.mark.parametrize("warm", [1, 9, 0])
@pytest.mark.parametrize("start", [GUESS, ZERO], ids=["guess", "zero"])
def test_start_states_and_warmups(eng, cost, mode, D, wide, warm, start):
    """Three strips plus a ragged fourth, and one strip without an interior boundary; the
    shortest warmup, one 9-column chunk and the default."""
    H, W = 24, D + (3 * CW[D] + 5 if wide else 20)
    _check_random(eng, H, W, D, _params(cost, D, mode), 100 + D + mode, ew_start=start, ew_warmup=warm)


@pytest.mark.parametrize("warm", [1, 9])
def test_guess_columns_left_of_the_domain(eng, warm):
    """minDisparity -5: the first strips' guess columns fall outside the cost volume's columns."""
    D = 128
    _check_random(eng, 24, D + 3 * CW[D] + 5, D, _params(1, D, 8, minD=-5), 77, ew_start=GUESS, ew_warmup=warm)


def _bands(H, W, period=40, seed=0):
    """Textureless vertical bands alternating with random texture."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    flat = (np.arange(W) // period) % 2 == 0
    img[:, flat] = 90
    return img


ADV = [
    ("const", lambda H, W: (np.full((H, W), 77, np.uint8), np.full((H, W), 77, np.uint8))),
    ("const_lr_differ", lambda H, W: (np.full((H, W), 40, np.uint8), np.full((H, W), 200, np.uint8))),
    ("bands", lambda H, W: (_bands(H, W, 40, 1), np.roll(_bands(H, W, 40, 1), -7, axis=1))),
    ("wide_bands", lambda H, W: (_bands(H, W, 150, 2), np.roll(_bands(H, W, 150, 2), -3, axis=1))),
    ("hgradient", lambda H, W: (np.tile(np.arange(W, dtype=np.int64) % 256, (H, 1)).astype(np.uint8),
                                np.tile((np.arange(W, dtype=np.int64) + 5) % 256, (H, 1)).astype(np.uint8))),
    ("noise_lr_indep", lambda H, W: (np.random.default_rng(3).integers(0, 256, (H, W)).astype(np.uint8),
                                     np.random.default_rng(4).integers(0, 256, (H, W)).astype(np.uint8))),
]


@pytest.mark.parametrize("name,make", ADV, ids=[a[0] for a in ADV])
@pytest.mark.parametrize("cost,mode,D,P1,P2", [(1, 8, 128, 60, 61), (1, 8, 128, 1, 193), (1, 8, 32, 192, 193),
                                               (0, 5, 128, 200, 201)])
def test_guess_adversarial(eng, name, make, cost, mode, D, P1, P2):
    """Inputs chosen against the speculation (flat images: A - min A = 0, the zero state; flat
    bands; smooth gradients; uncorrelated noise) with the cost-derived start at the smallest P2
    the matcher keeps and at the census form's largest."""
    H, W = 23, 3 * D + 257
    left, right = make(H, W)
    p = _params(cost, D, mode, P1=P1, P2=P2)
    out = _run(eng, left, right, p, ew_start=GUESS)
    exp = ref_c.compute(left, right, p)
    assert np.array_equal(out, exp), f"{np.sum(out != exp)} px differ"


def test_repair_counts(eng):
    """24 KITTI-wide census rows of the seed-1003 pair the CPU model studies (rows 150-173 of
    the 375-row pair: a pair generated at H = 24 squeezes the whole disparity ramp into 24 rows,
    nothing matches inside a census window and every start state is repaired nearly everywhere,
    6014 / 6512 / 7372 walks): the cost-derived start at 9 warmup columns is repaired about as
    rarely as the zero state at 18 and far more rarely than the zero state at 9 (the CPU model,
    tools/ew_start_study.py: 0.033-0.034 / 0.033-0.035 / 0.77 of the segments)."""
    (KH, W, D), H = synthetic.CONFIGS["kitti"], 24
    left, right = (np.ascontiguousarray(a[150:150 + H]) for a in _pair(KH, W, D, 1003))
    p = _params(1, D, 8)
    exp = ref_c.compute(left, right, p)
    rep = {}
    for key, start, warm in (("guess9", GUESS, 9), ("zero18", ZERO, 18), ("zero9", ZERO, 9)):
        c0 = eng.counters()
        out = _run(eng, left, right, p, ew_start=start, ew_warmup=warm)
        assert np.array_equal(out, exp), f"{key}: {np.sum(out != exp)} px differ"
        assert eng.counters()["line_groups"] > c0["line_groups"], "the in-sweep lines ran"
        rep[key] = eng.counters()["ew_repairs"] - c0["ew_repairs"]
    print("ew_repairs", rep)
    assert rep["guess9"] <= 1.5 * rep["zero18"] + 8
    assert rep["guess9"] <= 0.25 * rep["zero9"]


def test_start_tuning_arguments(eng):
    for bad in (-2, 5):
        with pytest.raises(ValueError):
            eng.set_tuning(eng.TUNE_EW_START, bad)
    for ok in (-1, 1, 2, 3, 4, 0):
        eng.set_tuning(eng.TUNE_EW_START, ok)
