"""The SGM engines where u16 path sums saturate and S clamps at 32767.

Every other engine test runs `synthetic.parity_params`, whose paths stay below about 7100 and
whose five-path sums stay below 36000.  Here `path_max` (sm_api.hip) runs from 13107 to 16384 on
inputs (tests/highcost.py) that put cells at and above 65535, between 32767 and 65535 and whole
pixels at the WTA's clamp: the MODE 3 partial saturates, the eight-path sum chains saturating adds,
every WTA clamps at 32767 and rejects a clamped minimum, the E/W patch takes its ordered form with
the "a cell at 0xFFFF stays there" repair, the row bands switch off, and the volume mode's pad
planes (S = 0xFFFF) stand beside clamped real planes.  Everything is bit-exact against the C oracle;
test_highcost_oracle.py holds the inputs to their coverage floors on the CPU."""
import functools

import numpy as np
import pytest

import highcost as hc
import strided
from conftest import skip_unless_ablation
from oracle import ref_c, sgm_np, wls_np
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

PERDIR, SWEEP8, NARROW, WIDE, HYBRID = 4096, 16384, 1 << 19, 1 << 21, 32768
# the engine flags of test_gpu_parity.py test_random_shapes_vs_c_oracle
FLAGS = [0, PERDIR, SWEEP8, SWEEP8 | NARROW, SWEEP8 | WIDE, HYBRID]
FLAG_IDS = {0: "default", PERDIR: "perdir", SWEEP8: "sweep8", SWEEP8 | NARROW: "sweep8narrow",
            SWEEP8 | WIDE: "sweep8wide", HYBRID: "hybrid"}


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


class Tuned:
    """Debug flags and SM_TUNE_* knobs for the block, all back at 0 afterwards; `grew` holds the
    counters' growth over the block."""

    def __init__(self, eng, flags=0, **tune):
        self.eng, self.flags, self.tune, self.grew = eng, flags, tune, {}

    def __enter__(self):
        try:
            self.eng.set_debug_flags(self.flags)
            for k, v in self.tune.items():
                self.eng.set_tuning(getattr(self.eng, "TUNE_" + k.upper()), v)
        except BaseException:
            self._restore()
            raise
        self.c0 = self.eng.counters()
        return self

    def _restore(self):
        self.eng.set_debug_flags(0)
        for k in self.tune:
            self.eng.set_tuning(getattr(self.eng, "TUNE_" + k.upper()), 0)

    def __exit__(self, *exc):
        try:
            c1 = self.eng.counters()
            self.grew = {k: c1[k] - self.c0[k] for k in c1}
        finally:
            self._restore()
        return False


def _same(got, exp, what=""):
    assert np.array_equal(got, exp), f"{what}: {int(np.sum(got != exp))} px differ"


@functools.lru_cache(maxsize=None)
def _expected(inp, H, W, D, seed, pkey):
    """(map, WTA index) of the C oracle, computed once per input and parameter set."""
    out = ref_c.compute_wta(*hc.pair(inp, H, W, D, seed), dict(pkey))
    for a in out:
        a.setflags(write=False)
    return out


def _wta_device(eng, left, right, p):
    """sm_compute_wta_batch_device on one pair, as tests/test_gpu_wta.py calls it."""
    import torch

    H, W = left.shape
    L = torch.tensor(np.ascontiguousarray(left)[None], device="cuda")
    R = torch.tensor(np.ascontiguousarray(right)[None], device="cuda")
    out = torch.full((1, H, W), 7777, dtype=torch.int16, device="cuda")
    wta = torch.full((1, H, W), 7777, dtype=torch.int16, device="cuda")
    eng.compute_wta_batch_device(L.data_ptr(), R.data_ptr(), 1, H * W, H, W, W, synthetic.to_sm_params(p),
                                 out.data_ptr(), wta.data_ptr())
    eng.synchronize()
    return out.cpu().numpy()[0], wta.cpu().numpy()[0]


def _batch(eng, pairs, p):
    """sm_compute_batch_device over the pairs: int16 [n, H, W]."""
    import torch

    n = len(pairs)
    H, W = pairs[0][0].shape
    L = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
    R = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
    out = torch.full((n, H, W), strided.SENTINEL, dtype=torch.int16, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.compute_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, synthetic.to_sm_params(p),
                                 out.data_ptr())
        eng.synchronize()  # raises if a sweep strip hand-off timed out
    finally:
        eng.set_stream(None)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _batch_pairs(inp, H, W, D, n):
    return tuple(hc.pair(inp, H, W, D, seed) for seed in range(1, n + 1))


@functools.lru_cache(maxsize=None)
def _batch_expected(inp, H, W, D, n, pkey):
    out = ref_c.compute_many(list(_batch_pairs(inp, H, W, D, n)), dict(pkey))
    for o in out:
        o.setflags(write=False)
    return tuple(out)


# ---------------------------------------------------------------- a. every engine, outputs
def _engine_cases():
    """About 140 of the cross product (3 inputs x 7 sets x 2 variants x 2 modes x 4 D x 2 minD x
    6 flags): every set, flag and mode with mixed40 at D = 64, the other inputs and D = 16 / 128
    under every flag with the sets, modes, variants and minDisparity taken in turn, and one
    D = 256 case per flag."""
    names, variants = list(hc.SETS), list(hc.VARIANTS)
    out = []

    def add(inp, name, mode, D, flags):
        i = len(out)
        k = i + i // 6 + i // 12
        H, W = (23, 600) if D == 256 else (23, 3 * D + 257)
        out.append((inp, name, variants[k % 2], mode, H, W, D, (0, -5)[(k // 2 + i // 24) % 2], flags))

    for name in names:
        for mode in (5, 8):
            for flags in FLAGS:
                add("mixed40", name, mode, 64, flags)
    turn = 0
    for inp, Ds in (("saw", (16, 64, 128)), ("mixed150", (16, 64, 128)), ("mixed40", (16, 128))):
        for D in Ds:
            for flags in FLAGS:
                add(inp, names[turn % 7], (5, 8)[(turn // 7 + turn) % 2], D, flags)
                turn += 1
    for j, flags in enumerate(FLAGS):
        add("mixed40", "FAST_TOP", (5, 8)[j % 2], 256, flags)
    return out


ENGINE_CASES = _engine_cases()


def _case_id(c):
    inp, name, variant, mode, H, W, D, minD, flags = c
    return f"{inp}-{name}-{variant}-p{mode}-D{D}-m{minD}-{FLAG_IDS[flags]}"


def test_engine_case_list():
    """The thinned cross product keeps what the thinning must not lose."""
    core = [c for c in ENGINE_CASES if c[0] == "mixed40" and c[6] == 64]
    assert {(c[1], c[3], c[8]) for c in core} == {(n, m, f) for n in hc.SETS for m in (5, 8) for f in FLAGS}
    assert {(c[1], c[2]) for c in ENGINE_CASES} == {(n, v) for n in hc.SETS for v in hc.VARIANTS}
    for inp in hc.INPUTS:
        assert {(c[6], c[8]) for c in ENGINE_CASES if c[0] == inp} >= {(D, f) for D in (16, 64, 128) for f in FLAGS}
    assert {c[7] for c in ENGINE_CASES} == {0, -5} and any(c[6] == 256 for c in ENGINE_CASES)
    assert 130 <= len(ENGINE_CASES) <= 160 and len(set(ENGINE_CASES)) == len(ENGINE_CASES)


@pytest.mark.parametrize("c", ENGINE_CASES, ids=_case_id)
def test_engines_map_and_wta_index(eng, c):
    """The int16 map of sm_compute and the map and integer WTA index of
    sm_compute_wta_batch_device.  The index does not pass through the LR check, so it shows a wrong
    S even where the final map is -1."""
    inp, name, variant, mode, H, W, D, minD, flags = c
    skip_unless_ablation(flags)
    left, right = hc.pair(inp, H, W, D)
    p = hc.params(name, D, mode, minD, variant)
    exp, exp_wta = _expected(inp, H, W, D, 1, strided.key(p))
    with Tuned(eng, flags):
        out = eng.compute(left, right, synthetic.to_sm_params(p))
        out2, wta = _wta_device(eng, left, right, p)
    _same(wta, exp_wta, "WTA index")
    _same(out, exp, "sm_compute")
    _same(out2, exp, "sm_compute_wta_batch_device")


# ---------------------------------------------------------------- b. intermediate volumes
def test_cost_and_path_volumes_at_the_top(eng):
    """The per-direction engine's cost volume and its eight path volumes at FAST_TOP: u16 cells
    up to 15000 and more, each direction against the numpy recurrence."""
    H, W, D = 40, 200, 32
    left, right = hc.pair("mixed40", H, W, D)
    p = hc.params("FAST_TOP", D, 8)
    with Tuned(eng, PERDIR):
        out = eng.compute(left, right, synthetic.to_sm_params(p))
        cost = eng.debug_fetch(0)
        paths = eng.debug_fetch(1)
    prm = sgm_np.normalize_params(p)
    Cref = ref_c.cost_volume(left, right, p).astype(np.int64) - prm["P2"]  # OpenCV's rows carry the P2 seed
    C = np.frombuffer(cost, np.uint16).reshape(Cref.shape).astype(np.int64)
    _same(C, Cref, "cost volume")
    vols = np.frombuffer(paths, np.uint16).reshape((8,) + Cref.shape).astype(np.int64)
    for k, d in enumerate(hc.ENGINE_DIRS):  # E, W, SE, S, SW, NE, N, NW
        _same(vols[k], sgm_np.aggregate_path(Cref, d, prm["P1"], prm["P2"]), f"direction {d}")
    assert vols.max() >= 15000, int(vols.max())
    _same(out, ref_c.compute(left, right, p), "map")


# ---------------------------------------------------------------- c. the 13107 / 13108 boundary
# D = 64 is the size the boundary was first asked about, but u16 costs have no wide MODE 3 instance
# there (sm_sweep.hpp wide_ncw: 16, 32, 48, 96, 128, 160), so neither the in-sweep lines nor the row
# bands can run at D = 64: that size is held to the oracle, and the counters are asserted at
# D = 128, where the instance is built.  Two bands of 25 rows at one pair.
BAND_SHAPES = {64: (50, 449, 64), 128: (50, 641, 128)}
LINES_BUILT = {64: False, 128: True}


@pytest.mark.parametrize("D", list(BAND_SHAPES))
@pytest.mark.parametrize("variant", list(hc.VARIANTS))
def test_band_boundary_one_pair(eng, variant, D):
    """One pair, 5 paths: at path_max 13107 the row bands run (5 x 13107 = 65535: no partial cell
    can saturate), at 13108 they do not, not even when SM_TUNE_BANDS asks for them."""
    H, W, D = BAND_SHAPES[D]
    left, right = hc.pair("mixed150", H, W, D)
    for name, banded in (("ATOM_TOP", LINES_BUILT[D]), ("SAT_BOTTOM", False)):
        p = hc.params(name, D, 5, 0, variant)
        exp, _ = _expected("mixed150", H, W, D, 1, strided.key(p))
        with Tuned(eng) as t:
            out = eng.compute(left, right, synthetic.to_sm_params(p))
        _same(out, exp, name)
        assert (t.grew["band_groups"] > 0) == banded, (name, t.grew)
        with Tuned(eng, bands=2, band_guess=1) as t:
            out = eng.compute(left, right, synthetic.to_sm_params(p))
        _same(out, exp, name + " bands 2, wrong entering state")
        assert (t.grew["band_groups"] > 0) == banded, (name, t.grew)
        assert (t.grew["band_repairs"] > 0) == banded, (name, t.grew)
        assert t.grew["sweep_fallbacks"] == 0


@pytest.mark.parametrize("D", list(BAND_SHAPES))
@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("name", ["ATOM_TOP", "SAT_BOTTOM"])
def test_band_boundary_batch(eng, name, mode, D):
    """Four pairs per call: the default sweeps with in-sweep E/W lines; the atomic E/W patch at
    13107 and the ordered read-modify-write patch at 13108, with a wrong start state so that
    nearly every segment is patched."""
    H, W, D = BAND_SHAPES[D]
    pairs = _batch_pairs("mixed150", H, W, D, 4)
    p = hc.params(name, D, mode, 0, "strict")
    exp = _batch_expected("mixed150", H, W, D, 4, strided.key(p))
    for tune in ({}, dict(ew_guess=1, ew_warmup=1)):
        with Tuned(eng, **tune) as t:
            got = _batch(eng, pairs, p)
        for i in range(4):
            _same(got[i], exp[i], f"{name} pair {i} {tune}")
        # (13107 at 5 paths: the launch group may take row bands too, where its strips leave CUs idle)
        assert t.grew["band_groups"] == 0 or (name == "ATOM_TOP" and mode == 5), t.grew
        assert t.grew["sweep_fallbacks"] == 0, t.grew
        assert (t.grew["line_groups"] > 0) == LINES_BUILT[D], t.grew
        if tune and LINES_BUILT[D]:
            assert t.grew["ew_repairs"] > 0, t.grew


# ---------------------------------------------------------------- d. repairs among saturated cells
# sizes with a wide MODE 3 u16 instance: 16-lane lines in 36-column strips (D = 128) and 8-lane
# lines in 88-column strips (D = 32), both narrower than the 150- and 200-column stripes
REPAIR_SHAPES = {128: (23, 641, 128), 32: (23, 353, 32)}


def _repair_case(eng, inp, name, mode, flags, D=128, **tune):
    H, W, D = REPAIR_SHAPES[D]
    pairs = _batch_pairs(inp, H, W, D, 4)
    p = hc.params(name, D, mode, 0, "strict")
    exp = _batch_expected(inp, H, W, D, 4, strided.key(p))
    with Tuned(eng, flags, **tune) as t:
        got = _batch(eng, pairs, p)
    for i in range(4):
        _same(got[i], exp[i], f"{inp} {name} pair {i}")
    assert t.grew["line_groups"] > 0 and t.grew["sweep_fallbacks"] == 0, t.grew
    return t.grew


@pytest.mark.parametrize("flags", [0, SWEEP8], ids=["default", "sweep8"])
@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("name,D", [("FAST_TOP", 128), ("BS9", 128), ("BS3", 128), ("FAST_TOP", 32)])
@pytest.mark.parametrize("inp", ["mixed150", "saw_bands"])
def test_repairs_among_saturated_cells(eng, inp, name, D, mode, flags):
    """A wrong start state and the shortest warmup: the ordered E/W patch repairs nearly every
    strip segment of partials that hold cells at 0xFFFF, and in stripes of saturated cells wider
    than a strip the repaired walks stay open and are carried on."""
    grew = _repair_case(eng, inp, name, mode, flags, D, ew_guess=1, ew_warmup=1)
    print(inp, name, D, mode, flags, grew)
    assert grew["ew_repairs"] > 0, grew
    assert grew["ew_open"] > 0, grew


@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("tune", [dict(ew_patch=1), dict(ew_patch=-1), dict(ew_start=1), dict(ew_start=-1),
                                  dict(ew_start=1, ew_warmup=9), dict(ew_start=-1, ew_warmup=1),
                                  dict(ew_patch=1, ew_guess=1, ew_warmup=1),
                                  dict(ew_patch=-1, ew_start=1, ew_guess=1, ew_warmup=1)],
                         ids=lambda t: "-".join(f"{k}{v}" for k, v in t.items()))
def test_patch_place_and_start_state_at_the_top(eng, tune, mode):
    """SM_TUNE_EW_PATCH and SM_TUNE_EW_START over the values of test_gpu_patch_in_sweep.py and
    test_gpu_ew_start.py, on saturated data."""
    _repair_case(eng, "mixed150", "FAST_TOP", mode, SWEEP8, **tune)


# ---------------------------------------------------------------- e. the 16383 / 16384 boundary
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mode", [5, 8])
def test_fast_top_and_wide_bottom(eng, mode, D):
    """P2 7122 runs the packed u16 kernels, P2 7123 OpenCV's int16 arithmetic (sm_wide.hpp): the
    same pairs, four per call and one at a time, both equal to the oracle."""
    H, W = 23, 3 * D + 257
    pairs = _batch_pairs("mixed150", H, W, D, 4)
    for name in ("FAST_TOP", "WIDE_BOTTOM"):
        p = hc.params(name, D, mode, 0, "strict")
        exp = _batch_expected("mixed150", H, W, D, 4, strided.key(p))
        got = _batch(eng, pairs, p)
        for i in range(4):
            _same(got[i], exp[i], f"{name} pair {i} of the batch")
        for inp in hc.INPUTS:
            q = hc.params(name, D, mode, 0, "open")
            _same(eng.compute(*hc.pair(inp, H, W, D), synthetic.to_sm_params(q)),
                  _expected(inp, H, W, D, 1, strided.key(q))[0], f"{name} {inp}")


# ---------------------------------------------------------------- f. volume mode
VOL_HW = (24, 150)


@functools.lru_cache(maxsize=None)
def _volume_expected(D, lo, seed, pkey):
    out = ref_c.compute_volume(hc.high_volume(D, *VOL_HW, lo, seed), dict(pkey), 0.0, 1.0)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("flags", [0, PERDIR, SWEEP8], ids=["default", "perdir", "sweep8"])
@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("name", list(hc.VOLUME_SETS))
@pytest.mark.parametrize("lo", hc.VOLUME_LO)
@pytest.mark.parametrize("D", [32, 37])
def test_volume_at_the_top(eng, D, lo, name, mode, flags):
    """External volumes near VOL_CMAX with P2 up to 12288 (L = 16383 exactly).  D = 37 runs on 48
    planes whose pad planes hold S = 0xFFFF; they must never win against real planes clamped to
    32767.  The window is offset 0, scale 1: nothing is clamped, nothing is NaN."""
    vol = hc.high_volume(D, *VOL_HW, lo)
    p = hc.volume_params(name, D, mode)
    with Tuned(eng, flags) as t:
        out = eng.aggregate_cost_f32(vol, synthetic.to_sm_params(p), 0.0, 1.0)
    _same(out, _volume_expected(D, lo, 1, strided.key(p)))
    assert t.grew["volume_clamped"] == 0 and t.grew["volume_nan"] == 0, t.grew


@pytest.mark.parametrize("mode", [5, 8])
@pytest.mark.parametrize("D", [32, 37])
def test_volume_batch_device_with_gaps(eng, D, mode):
    """Three volumes per call with a gap of huge values between them, the maps between sentinel
    guards: a cell read from the gap would count as clamped."""
    import torch

    H, W = VOL_HW
    n, gap = 3, 1000
    p = hc.volume_params("P12288_100", D, mode)
    stride = D * H * W + gap
    host = np.full(n * stride, 3.0e38, np.float32)
    for i in range(n):
        host[i * stride:i * stride + D * H * W] = hc.high_volume(D, H, W, hc.VOLUME_LO[i % 2], 1 + i).ravel()
    V = torch.from_numpy(host).cuda()
    out = strided.guarded(n, H, W)
    with Tuned(eng) as t:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.aggregate_cost_f32_device(V.data_ptr(), n, stride, D, H, W, synthetic.to_sm_params(p), 0.0, 1.0,
                                          out[1])
            eng.synchronize()
        finally:
            eng.set_stream(None)
    got = strided.maps_of(out, n, H, W)
    for i in range(n):
        _same(got[i], _volume_expected(D, hc.VOLUME_LO[i % 2], 1 + i, strided.key(p)), f"volume {i}")
    assert t.grew["volume_clamped"] == 0 and t.grew["volume_nan"] == 0, t.grew
    assert np.array_equal(V.cpu().numpy(), host), "the input was written"


# ---------------------------------------------------------------- g. one chain
CHAIN_SHAPE = (50, 320, 64)


def _chain_expected(left, right, p, lmbda, sigma):
    """(displ, filtered) of the oracles, built as test_compute_disparity_left_matcher_semantics and
    test_compute_disparity_end_to_end build them: the left matcher with the WLS factory's mutation,
    the right matcher of the unmutated parameters on the swapped pair."""
    D, minD = p["numDisparities"], p["minDisparity"]
    exp_l = ref_c.compute(left, right, dict(p, uniquenessRatio=0, disp12MaxDiff=1000000))
    exp_r = ref_c.compute(right, left, sgm_np.right_matcher_params(p))
    wp = dict(lmbda=float(lmbda), sigma=float(sigma), radius=-(-p["blockSize"] // 2), min_disp=minD,
              left_offset=max(0, minD + D), right_offset=max(0, -minD))
    return exp_l, exp_r, wp, wls_np.wls_filter(exp_l, left, exp_r, wp)


def test_chain_at_fast_top():
    """Left matcher, right matcher and WLS filter at FAST_TOP (P1 100, P2 7122) on a mixed40 pair:
    the three calls compute_disparity makes, and sm_compute_disparity in one call.  (No settings
    dict gives FAST_TOP exactly: compute_disparity derives P2 = 96 window_size^2.)"""
    import stereo_match_amd as sm
    from stereo_match_amd import wls

    H, W, D = CHAIN_SHAPE
    left, right = hc.pair("mixed40", H, W, D)
    p = hc.params("FAST_TOP", D, 5, 0, "strict")
    exp_l, exp_r, wp, exp_f = _chain_expected(left, right, p, 8000.0, 1.5)
    lm = sm.StereoSGBM_create(minDisparity=0, numDisparities=D, blockSize=p["blockSize"], P1=p["P1"], P2=p["P2"],
                              disp12MaxDiff=p["disp12MaxDiff"], uniquenessRatio=p["uniquenessRatio"],
                              speckleWindowSize=0, speckleRange=p["speckleRange"], preFilterCap=63)
    sp = lm.params()  # before the WLS factory's mutation
    rm = sm.createRightMatcher(lm)
    f = wls.createDisparityWLSFilter(lm)
    f.setLambda(8000.0)
    f.setSigmaColor(1.5)
    displ = lm.compute(left, right)
    dispr = rm.compute(right, left)
    _same(displ, exp_l, "left matcher")
    _same(dispr, exp_r, "right matcher")
    _same(f.filter(displ, left, None, dispr), exp_f, "WLS")
    d1, f1 = _lib.engine(0).compute_disparity(left, right, sp, f.params(H, W))
    _same(d1, exp_l, "sm_compute_disparity displ")
    _same(f1, exp_f, "sm_compute_disparity filtered")
    assert (exp_l >= 0).mean() > 0.5 and len(np.unique(exp_f)) > 50  # a live map, not all invalid


def test_compute_disparity_settings_in_the_regime():
    """sm.compute_disparity itself with the settings nearest below FAST_TOP: block_size 7,
    window_size 8 (P1 1536, P2 6144: path_max 15405, past 13107)."""
    import stereo_match_amd as sm

    H, W, D = CHAIN_SHAPE
    left, right = hc.pair("mixed40", H, W, D)
    s = dict(sm.DEFAULT_SETTINGS, window_size=8, block_size=7, num_disparities=D, lmbda=8000, sigma=1.5)
    p = dict(synthetic.parity_params(D, 8), blockSize=7, uniquenessRatio=s["uniqueness_ratio"],
             disp12MaxDiff=s["disp12_max_diff"], preFilterCap=s["pre_filter_cap"], speckleRange=s["speckle_range"])
    assert 13108 <= 49 * 189 + p["P2"] <= 16383
    exp_l, _, _, exp_f = _chain_expected(left, right, p, s["lmbda"], s["sigma"])
    displ, filt = sm.compute_disparity(left, right, s)
    _same(displ, exp_l, "displ")
    _same(filt, exp_f, "filtered")
