"""StereoBM on the device at every configuration of k_bm_sad (csrc/sm_bm.hpp), bit-exact against
oracle/bm_np.py: the four strip widths run_bm (csrc/sm_api.hip) picks and the pairs it refuses,
rofs > 0, the sub-pixel end mirrors, SADs above 2^22 in the WTA key, a batch past one launch
group, and validateDisparity on rows whose LDS passes 64 KiB.  The tables are tests/bm_cases.py;
test_bm_cases_oracle.py shows on the CPU that none of them is vacuous."""
import numpy as np
import pytest

import bm_cases as C
import strided as S
from stereo_match_amd import _lib

pytestmark = pytest.mark.gpu

RUN_IDS = [C.case_id(c) for c in C.RUNNING]


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def differ(got, exp) -> str:
    bad = np.argwhere(got != exp)
    return f"{len(bad)} px differ, first at {tuple(bad[0]) if len(bad) else None}"


def compute(eng, left, right, p):
    return eng.bm_compute(left, right, S.bm_params(p))


def device_batch(eng, images, p, extra, gap, offsets, fill):
    """sm_bm_compute_batch_device on pairs embedded with rows `extra` bytes longer than W and
    `gap` bytes between the pairs, into a guarded output: the [n, H, W] maps."""
    import torch

    n = len(images)
    H, W = images[0][0].shape
    st = W + extra
    ps = H * st + gap
    L, pl = S.embed([a for a, _ in images], st, ps, offsets[0], fill)
    R, pr = S.embed([b for _, b in images], st, ps, offsets[1], fill)
    out = S.guarded(n, H, W)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.bm_compute_batch_device(pl, pr, n, ps, H, W, st, S.bm_params(p), out[1])
        eng.synchronize()
    finally:
        eng.set_stream(None)
    assert S.unchanged(L) and S.unchanged(R), "the call wrote into its input"
    return S.maps_of(out, n, H, W)


# ---- the strip widths
@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("c", C.RUNNING, ids=RUN_IDS)
def test_strip_rows(eng, c, which):
    left, right, p = C.strip_inputs(c, which)
    got = compute(eng, left, right, p)
    exp = C.expected_strip(c, which)
    assert np.array_equal(got, exp), f"SWs {c.sws}, set {which}: {differ(got, exp)}"


# one row per strip width (D = 16 .. 256, the two-band row among them)
DEVICE_ROWS = [next(c for c in C.RUNNING if (c.D, c.bs, c.H) == k)
               for k in ((112, 15, 30), (160, 15, 30), (256, 5, 72), (256, 33, 60))]


@pytest.mark.parametrize("c", DEVICE_ROWS, ids=[f"SWs{c.sws}" for c in DEVICE_ROWS])
def test_strip_rows_strided_device_batch(eng, c):
    """sm_bm_compute_batch_device on a batch of the row's pair and its swap, once with set B's
    parameters and once with the right matcher's: rows 13 bytes longer than W, 77 bytes between
    the pairs, left and right misaligned to each other, guards around the output."""
    assert {r.sws for r in DEVICE_ROWS} == {64, 32, 16, 8}
    left, right, pb = C.strip_inputs(c, "B")
    _, _, pc = C.strip_inputs(c, "C")
    images = [(left, right), (right, left)]
    for p, fill in ((pb, 0x00), (pc, 0xFF)):
        got = device_batch(eng, images, p, 13, 77, (1, 0), fill)
        for i, (a, b) in enumerate(images):
            exp = C.oracle(a, b, p)
            assert np.array_equal(got[i], exp), f"SWs {c.sws} pair {i}: {differ(got[i], exp)}"


# ---- refusals
@pytest.mark.parametrize("c", C.REFUSED, ids=[C.case_id(c) for c in C.REFUSED])
def test_refused_rows(eng, c):
    left, right, p = C.strip_inputs(c, "A")
    with pytest.raises(_lib.SmError) as ei:
        compute(eng, left, right, p)
    assert ei.value.code == _lib.SM_E_UNSUPPORTED
    msg = str(ei.value)
    assert f"blockSize {c.bs}" in msg and f"numDisparities {c.D}" in msg
    n = C.running_neighbour(c)
    left, right, p = C.strip_inputs(n, "B")
    got = compute(eng, left, right, p)
    assert np.array_equal(got, C.expected_strip(n, "B")), differ(got, C.expected_strip(n, "B"))


def test_refusal_needs_a_region(eng):
    """Where nothing would be launched nothing is refused: FILTERED everywhere, as the oracle."""
    c = C.REFUSED[0]
    left, right = C.pair(c.bs + 1, c.D + c.bs - 2, c.D)
    p = C.base_params(c)
    got = compute(eng, left, right, p)
    assert np.array_equal(got, C.oracle(left, right, p)) and (got == -16).all()


# ---- rofs > 0, and frames without a region
@pytest.mark.parametrize("c", C.RANGE_CASES, ids=[f"{C.case_id(c)}_{i}" for i, c in enumerate(C.RANGE_CASES)])
def test_range_cases(eng, c):
    left, right, p = C.range_inputs(c)
    got = compute(eng, left, right, p)
    exp = C.oracle(left, right, p)
    assert np.array_equal(got, exp), differ(got, exp)


# ---- the sub-pixel end mirrors
@pytest.mark.parametrize("c", C.SHIFT_CASES, ids=[f"bs{c.bs}_minD{c.minD}_mind{c.mind}" for c in C.SHIFT_CASES])
def test_shift_cases(eng, c):
    left, right, p = C.shift_inputs(c)
    got = compute(eng, left, right, p)
    exp = C.oracle(left, right, p)
    assert np.array_equal(got, exp), f"winner at index {c.mind}: {differ(got, exp)}"


# ---- 23 bits of SAD in the WTA key
@pytest.mark.parametrize("uniq", C.HIGH_SAD_UNIQ)
def test_high_sad(eng, uniq):
    left, right, p = C.high_sad_inputs(uniq)
    got = compute(eng, left, right, p)
    exp = C.oracle(left, right, p)
    assert np.array_equal(got, exp), differ(got, exp)


# ---- more pairs than one launch group
def test_batch_of_17(eng):
    images = C.batch_pairs()
    got = device_batch(eng, images, C.BATCH_PARAMS, 3, 50, (0, 1), 0xFF)
    for i, (a, b) in enumerate(images):
        exp = C.oracle(a, b, C.BATCH_PARAMS)
        assert np.array_equal(got[i], exp), f"pair {i}: {differ(got[i], exp)}"


# ---- validateDisparity on wide rows
def test_validate_row_above_64k(eng):
    left, right, p = C.wide_inputs(C.WIDE_OK, 1)
    got = compute(eng, left, right, p)
    exp = C.oracle(left, right, p)
    assert np.array_equal(got, exp), differ(got, exp)


def test_validate_row_above_the_cu_is_refused(eng):
    left, right, p = C.wide_inputs(C.WIDE_REFUSED, 1)
    with pytest.raises(_lib.SmError) as ei:
        compute(eng, left, right, p)
    assert ei.value.code == _lib.SM_E_UNSUPPORTED
    assert str(C.WIDEST_VALIDATE) in str(ei.value) and "disp12MaxDiff" in str(ei.value)
    left, right, p = C.wide_inputs(C.WIDE_REFUSED, -1)
    got = compute(eng, left, right, p)
    exp = C.oracle(left, right, p)
    assert np.array_equal(got, exp), differ(got, exp)
    # and the engine validates an ordinary row afterwards
    c = C.RUNNING[0]
    got = compute(eng, *C.strip_inputs(c, "B"))
    assert np.array_equal(got, C.expected_strip(c, "B"))
