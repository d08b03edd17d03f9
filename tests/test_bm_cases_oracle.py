"""CPU: the case tables of tests/bm_cases.py are not vacuous.  test_gpu_bm_configs.py compares the
device with oracle/bm_np.py bit for bit, which proves nothing where the oracle's own map is all
FILTERED, holds a handful of values, or never reaches the configuration the row is there for.  So
the conditions on the inputs are checked here, against the oracle alone."""
import numpy as np
import pytest

import bm_cases as C
from oracle import bm_np

RUN_IDS = [C.case_id(c) for c in C.RUNNING]


def test_strip_width_table():
    assert {C.strip_width(c.D, c.bs) for c in C.STRIP_CASES} == {64, 32, 16, 8, 0}
    for c in C.STRIP_CASES:
        assert C.strip_width(c.D, c.bs) == c.sws, c
    for sws in (64, 32, 16, 8):
        assert sum(c.sws == sws for c in C.STRIP_CASES) >= 3
    assert {112, 128, 144, 160, 224, 240, 256} <= {c.D for c in C.RUNNING}
    # both sides of each boundary, at one numDisparities and adjacent block sizes
    sides = {(c.D, c.bs): c.sws for c in C.STRIP_CASES}
    for D, bs, hi, lo in ((112, 15, 64, 32), (224, 9, 32, 16), (256, 31, 16, 8), (256, 47, 8, 0),
                          (160, 85, 8, 0), (128, 109, 8, 0)):
        assert (sides[D, bs], sides[D, bs + 2]) == (hi, lo)
    for c in C.REFUSED:
        n = C.running_neighbour(c)
        assert (n.D, n.bs, n.sws) == (c.D, c.bs - 2, 8)


def test_strip_width_sweep():
    """The (numDisparities, blockSize) table of DESIGN.md: where each strip width begins."""
    first = {}
    for D in range(16, 257, 16):
        prev = 64
        for bs in range(5, 256, 2):
            s = C.strip_width(D, bs)
            assert s <= prev  # never wider again under a larger block
            if s != prev:
                first[D, s] = bs
            prev = s
    assert [first.get((112, s)) for s in (32, 16, 8, 0)] == [17, 81, 113, 129]
    assert [first.get((128, s)) for s in (16, 8, 0)] == [63, 95, 111]
    assert [first.get((160, s)) for s in (16, 8, 0)] == [39, 71, 87]
    assert [first.get((224, s)) for s in (16, 8, 0)] == [11, 43, 59]
    assert [first.get((256, s)) for s in (8, 0)] == [33, 49]
    assert first[64, 0] == 233 and (16, 32) not in first and C.strip_width(16, 255) == 64
    assert C.strip_width(128, 5) == 32 and C.strip_width(240, 5) == 16 and C.strip_width(256, 5) == 16


@pytest.mark.parametrize("c", C.STRIP_CASES, ids=[C.case_id(c) for c in C.STRIP_CASES])
def test_row_geometry(c):
    """An ROI of two rows at least; wider than one strip and no multiple of it, so that the last
    strip is partial (but for the one `narrow` row, whose ROI is 16 columns, and which has a
    sibling that is not); a refused row has a region too, since run_bm refuses only where it
    would launch."""
    _, _, p = C.strip_inputs(c, "A")
    x, y, w, h = bm_np.valid_roi(c.H, c.W, bm_np.normalize_bm(p))
    assert h >= 2 and w >= 1
    assert c.H <= 262 and c.W <= 345
    if c.narrow:
        assert w < c.sws and any(s.D == c.D and s.bs == c.bs and not s.narrow for s in C.RUNNING)
    elif c.sws:
        assert w > c.sws and w % c.sws != 0
    if c.sws:  # the right matcher's computed columns [blockSize // 2, W - D + 1) as well
        wc = c.W - c.D + 1 - c.bs // 2
        assert c.narrow or (wc > c.sws and wc % c.sws != 0)


@pytest.mark.parametrize("c", C.RUNNING, ids=RUN_IDS)
def test_set_a_keeps_every_pixel_and_many_values(c):
    left, right, p = C.strip_inputs(c, "A")
    roi, filtered = C.roi_of(C.oracle(left, right, p), p)
    distinct = len(np.unique(roi))
    print(f"{C.case_id(c)}: ROI {roi.shape}, {distinct} distinct values")
    assert (roi != filtered).all()
    assert distinct >= (C.MIN_DISTINCT_WIDE if c.bs >= 129 else C.MIN_DISTINCT)


@pytest.mark.parametrize("c", C.RUNNING, ids=RUN_IDS)
def test_set_b_is_mixed(c):
    left, right, p = C.strip_inputs(c, "B")
    roi, filtered = C.roi_of(C.oracle(left, right, p), p)
    kept = float(np.mean(roi != filtered))
    print(f"{C.case_id(c)}: uniquenessRatio {c.uniq_b} keeps {kept:.3f}")
    assert C.MIN_MIXED <= kept <= 1 - C.MIN_MIXED


@pytest.mark.parametrize("c", C.RUNNING, ids=RUN_IDS)
def test_set_c_keeps_the_columns_it_computes(c):
    """The right matcher (minDisparity = 1 - D) computes columns [0, W - D + 1) only, so over the
    whole valid ROI [blockSize // 2, W - blockSize // 2) it cannot keep more than
    (W - D + 1 - r) / (W - 2r), r = blockSize // 2: under a half at every row whose W < 2D.  The
    share is therefore taken over the ROI's computed columns."""
    left, right, p = C.strip_inputs(c, "C")
    out = C.oracle(left, right, p)
    roi, filtered = C.roi_of(out, p)
    computed = roi[:, :c.W - c.D + 1 - c.bs // 2]
    kept = float(np.mean(computed != filtered))
    print(f"{C.case_id(c)}: computed {computed.shape} of ROI {roi.shape}, kept {kept:.3f}, "
          f"{len(np.unique(computed))} distinct values")
    assert computed.shape[1] >= 1 and kept >= C.MIN_KEPT_C
    assert (roi[:, computed.shape[1]:] == filtered).all()


@pytest.mark.parametrize("c", C.RANGE_CASES, ids=[f"{C.case_id(c)}_{i}" for i, c in enumerate(C.RANGE_CASES)])
def test_range_cases(c):
    left, right, p = C.range_inputs(c)
    q = bm_np.normalize_bm(p)
    out = C.oracle(left, right, p)
    filtered = (c.minD - 1) * 16
    rofs = -min(c.D - 1 + c.minD, 0)
    if c.W - c.bs + 1 < c.D + rofs:
        assert (out == filtered).all() and q["speckleWindowSize"] > 0
    else:
        assert rofs > 0
        kept = float(np.mean(C.roi_of(out, p)[0] != filtered))
        print(f"{C.case_id(c)}: rofs {rofs}, kept {kept:.3f}")
        assert kept >= 0.1
    assert any(r.W - r.bs + 1 < r.D for r in C.RANGE_CASES)
    assert {(r.D, r.minD) for r in C.RANGE_CASES} >= {(16, -19), (32, -40), (256, -260)}


@pytest.mark.parametrize("c", C.SHIFT_CASES, ids=[f"bs{c.bs}_minD{c.minD}_mind{c.mind}" for c in C.SHIFT_CASES])
def test_shift_cases_win_at_the_ends(c):
    assert C.strip_width(c.D, c.bs) == c.sws
    assert c.shift == (c.minD + c.D - 1 if c.mind == 0 else c.minD)
    left, right, p = C.shift_inputs(c)
    roi, _ = C.roi_of(C.oracle(left, right, p), p)
    hit = float(np.mean((roi + 8) >> 4 == c.shift))
    print(f"shift {c.shift}: {hit:.4f} of ROI {roi.shape}")
    assert roi.size and hit >= C.MIN_SHIFT_HIT


def test_shift_cases_cover_the_table():
    assert {(c.bs, c.sws, c.minD, c.mind) for c in C.SHIFT_CASES} == \
        {(bs, sws, m, e) for bs, sws in ((5, 16), (33, 8)) for m in (0, 3) for e in (0, 255)}


def test_high_sad_fills_the_key():
    left, right, p = C.high_sad_inputs(0)
    out, cost = C.oracle(left, right, p, return_cost=True)
    roi, filtered = C.roi_of(out, p)
    croi, _ = C.roi_of(cost, p)
    print(f"ROI {roi.shape}, minimum SAD {croi.min()} .. {croi.max()}")
    assert roi.shape == (8, 31) and (roi != filtered).all()
    assert croi.min() > 1 << 22 and croi.max() < 1 << 23
    assert int(croi.max()) * max(C.HIGH_SAD_UNIQ) < 1 << 31
    left, right, p = C.high_sad_inputs(100)
    assert (C.oracle(left, right, p) == filtered).all()


def test_batch_is_past_one_launch_group():
    pairs = C.batch_pairs()
    assert len(pairs) == C.BATCH["n"] == 17
    outs = [C.oracle(a, b, C.BATCH_PARAMS) for a, b in pairs]
    assert len({o.tobytes() for o in outs}) == len(outs)
    for o in outs:
        roi, filtered = C.roi_of(o, C.BATCH_PARAMS)
        assert np.mean(roi != filtered) >= 0.2


def test_wide_validate_shapes():
    per = C.VALIDATE_LDS_PER_COLUMN
    assert 65536 < C.WIDE_OK["W"] * per <= 163840 < C.WIDE_REFUSED["W"] * per
    assert C.WIDEST_VALIDATE == 12603
    # validateDisparity removes pixels on both sides of column 5041, where its LDS passes 64 KiB
    with_check = C.oracle(*C.wide_inputs(C.WIDE_OK, 1))
    without = C.oracle(*C.wide_inputs(C.WIDE_OK, -1))
    columns = np.argwhere(with_check != without)[:, 1]
    assert (columns < 2500).sum() >= 100 and (columns > 5041).sum() >= 10
