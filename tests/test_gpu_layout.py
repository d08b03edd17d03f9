"""Which disparity wins, for every position a disparity can take inside a lane's packed words.

The fused sweeps keep a lane's disparities of u8-cost instances in the interleaved layout
(sm_pk.hpp pk_disp: word k = (d_k, d_k+NP)).  random_dot_pair's ground truth visits a few dozen
disparities per image, so a slip in the layout's bookkeeping (a word's halves exchanged, the
wrap between word NP - 1 and word 0, a lane edge, a converted store) could pass the other
suites.  A disparity ladder makes every such position the winner of some rows: rows of constant
shift d for d = 0 .. 2 DPL, D/2 - 1, D/2 and D - DPL - 1 .. D - 1 (DPL = D / 16 disparities per
lane of a 16-lane line).  Every case is bit-exact against the C oracle (oracle/sgm_ref.c), and
the oracle's own output is first checked to contain every target disparity."""
import numpy as np
import pytest

from oracle import ref_c
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

PERDIR = 4096   # sm_api.hip DBG_LEGACY: per-direction engine
SWEEP8 = 16384  # sm_api.hip DBG_SWEEP8: the fused sweeps at any pair count

ROWS = 4  # rows per target disparity (2 leave a few targets with fewer than 8 pixels)
SEED = 7


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def ladder_targets(D):
    dpl = max(D // 16, 1)
    t = set(range(0, 2 * dpl + 1)) | {D // 2 - 1, D // 2} | set(range(D - dpl - 1, D))
    return sorted(d for d in t if 0 <= d < D)


def ladder_pair(D, rows=ROWS, seed=SEED):
    """left[y] = base[y, :W], right[y] = base[y, d:d + W] with d = the target of row y (rows
    rows per target), base = smoothed seeded noise of shape (H, W + D); W = D + 80."""
    targets = ladder_targets(D)
    H, W = rows * len(targets), D + 80
    rng = np.random.default_rng(seed)
    base = np.clip(synthetic._smooth3(rng.integers(0, 256, (H, W + D)).astype(np.float64)), 0, 255).astype(np.uint8)
    left = np.ascontiguousarray(base[:, :W])
    right = np.empty_like(left)
    for y in range(H):
        d = targets[y // rows]
        right[y] = base[y, d:d + W]
    return left, right, targets


def assert_targets_win(disp, targets, rows, what):
    """Precondition on the oracle's map alone: every target disparity is the integer disparity
    (floor or ceil of value / 16) of at least 8 valid pixels in its own rows."""
    for i, d in enumerate(targets):
        v = disp[i * rows:(i + 1) * rows].astype(np.int64)
        hit = (v >= 0) & (((v >> 4) == d) | (((v + 15) >> 4) == d))
        assert int(hit.sum()) >= 8, f"{what}: target {d} wins only {int(hit.sum())} px of its rows"


MODES = {"census8": (1, 8), "census5": (1, 5), "sgbm5": (0, 5), "sgbm8": (0, 8)}


def _params(mode, D):
    cost, paths = MODES[mode]
    return dict(synthetic.headline_params(D) if cost else synthetic.parity_params(D), mode=paths)


_cache = {}


def _ladder(D, mode):
    """The pair and the oracle's map of (D, mode), computed once and checked once."""
    key = (D, mode)
    if key not in _cache:
        left, right, targets = ladder_pair(D)
        p = _params(mode, D)
        exp = ref_c.compute(left, right, p)
        exp.setflags(write=False)
        assert_targets_win(exp, targets, ROWS, f"D={D} {mode}")
        _cache[key] = (left, right, p, exp)
    return _cache[key]


def _run(eng, left, right, p, flags=SWEEP8, **tune):
    eng.set_debug_flags(flags)
    for k, v in tune.items():
        eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), v)
    try:
        return eng.compute(left, right, synthetic.to_sm_params(p))
    finally:
        eng.set_debug_flags(0)
        for k in tune:
            eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), 0)


ENGINES = {
    "lines": dict(flags=SWEEP8),                    # MODE 3 line waves -> patch -> MODE 4 / k_wta
    "ewvol": dict(flags=SWEEP8, sweep_lines=-1),    # E/W volumes: MODE 0 -> MODE 2, MODE 1
    "perdir": dict(flags=PERDIR),                   # per-direction engine
}

# (D, mode) whose wide MODE 3 instance is built (sm_sweep.hpp wide_ncw, LineGeo::BUILT: u8 costs
# up to D = 192, u16 costs except D = 64, 192 and 256): the lines engine must run there.  The
# other sizes take the E/W volumes, which the "ewvol" leg covers for every size
LINES_RUN = ({(D, m) for D in (16, 32, 48, 64, 96, 128, 160, 192) for m in ("census8", "census5")} |
             {(D, m) for D in (16, 32, 48, 96, 128, 160) for m in ("sgbm5", "sgbm8")})


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("D", [128, 160, 64, 16, 32, 48, 96, 192, 256])
def test_disparity_ladder(eng, D, mode, engine):
    left, right, p, exp = _ladder(D, mode)
    c0 = eng.counters()
    out = _run(eng, left, right, p, **ENGINES[engine])
    c1 = eng.counters()
    bad = out != exp
    assert not bad.any(), f"{int(bad.sum())} px differ, first rows {np.unique(np.nonzero(bad)[0])[:8]}"
    assert c1["sweep_fallbacks"] == c0["sweep_fallbacks"]
    if engine == "lines" and (D, mode) in LINES_RUN:
        assert c1["line_groups"] > c0["line_groups"], "the in-sweep lines ran"
    if engine != "lines":
        assert c1["line_groups"] == c0["line_groups"]


def test_padded_planes_ladder(eng):
    """A volume of 37 planes (Dv < D = 48: the pad planes' mask) whose winners include Dv - 1 and
    Dv - 2, through the lines and the E/W-volume engines."""
    Dv = 37
    left, right, targets = ladder_pair(Dv)
    assert Dv - 1 in targets and Dv - 2 in targets
    vol = synthetic.absdiff_volume(left, right, Dv)
    p = synthetic.cost_volume_params(Dv)
    exp = ref_c.compute_volume(vol[0], p, 0.0, synthetic.VOLUME_SCALE)
    assert_targets_win(exp, targets, ROWS, "volume Dv=37")
    for tune in (dict(), dict(sweep_lines=-1)):
        eng.set_debug_flags(SWEEP8)
        for k, v in tune.items():
            eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), v)
        try:
            out = eng.aggregate_cost_f32(vol, synthetic.to_sm_params(p), 0.0, synthetic.VOLUME_SCALE)
        finally:
            eng.set_debug_flags(0)
            for k in tune:
                eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), 0)
        assert np.array_equal(out, exp), f"{tune}: {int(np.sum(out != exp))} px differ"


def test_ew_repairs_on_the_ladder(eng):
    """The shortest warmup and a wrong start state: every E/W segment is repaired, each walk
    adding its deltas into the partial the sweeps wrote."""
    left, right, p, exp = _ladder(128, "census8")
    c0 = eng.counters()
    out = _run(eng, left, right, p, ew_warmup=1, ew_guess=1)
    c1 = eng.counters()
    assert np.array_equal(out, exp), f"{int(np.sum(out != exp))} px differ"
    assert c1["line_groups"] > c0["line_groups"]
    assert c1["ew_repairs"] > c0["ew_repairs"]


def test_band_repairs_on_the_ladder(eng):
    """Three row bands of the 5-path lines engine with a wrong entering state: the band patch
    walks add their deltas into the partial."""
    left, right, p, exp = _ladder(128, "census5")
    c0 = eng.counters()
    out = _run(eng, left, right, p, bands=3, band_guess=1)
    c1 = eng.counters()
    assert np.array_equal(out, exp), f"{int(np.sum(out != exp))} px differ"
    assert c1["band_groups"] > c0["band_groups"]
    assert c1["band_repairs"] > c0["band_repairs"]


def test_wta_out_kitti_width(eng):
    """The full wta_out record of a KITTI-width, 24-row pair through the fused sweeps: the
    records kept their public format (OpenCV's bestDisp, -1 where rejected)."""
    H, W, D = 24, synthetic.CONFIGS["kitti"][1], 128
    left, right, _ = synthetic.random_dot_pair(H, W, D, seed=77)
    p = synthetic.headline_params(D)
    eng.set_debug_flags(SWEEP8)
    try:
        disp, wta = eng.compute_wta(left, right, synthetic.to_sm_params(p))
    finally:
        eng.set_debug_flags(0)
    rdisp, rwta = ref_c.compute_wta(left, right, p)
    assert np.array_equal(wta, rwta), f"{int(np.sum(wta != rwta))} indices differ"
    assert np.array_equal(disp, rdisp)
    assert (wta >= 0).mean() > 0.3
