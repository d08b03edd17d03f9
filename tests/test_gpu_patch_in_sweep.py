"""The E/W patch pass inside the up + WTA sweep (SM_TUNE_EW_PATCH 1, DESIGN.md §4.4 addendum):
patch waves of the MODE 4 workgroups repair each row's partial before the sweep reaches it, in
place of the k_ew_patch launch between the sweeps.  Every case is bit-exact against the C oracle;
the old chain (SM_TUNE_EW_PATCH -1) gives the same maps and runs the same walks."""
import functools

import numpy as np
import pytest

from oracle import ref_c
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

SWEEP8 = 16384  # sm_api.hip DBG_SWEEP8: the fused sweeps at any pair count
IN_SWEEP, LAUNCH = 1, -1  # SM_TUNE_EW_PATCH
D = 128
CW = 36  # strip width of the wide D = 128 instances (9 own waves x 4 columns)


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _params(**kw):
    return dict(synthetic.headline_params(D), mode=8, **kw)


def _tuned(eng, fn, **tune):
    """fn() with DBG_SWEEP8 and the tuning knobs set; returns (result, counter deltas, patch launches)."""
    eng.set_debug_flags(SWEEP8)
    for k, v in tune.items():
        eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), v)
    eng.set_timing(True, stages=["horizontal"])
    eng.reset_timing()
    c0 = eng.counters()
    try:
        out = fn()
        c1 = eng.counters()
        launches = eng.timing()["horizontal"][1]
    finally:
        eng.set_timing(False)
        eng.set_debug_flags(0)
        for k in tune:
            eng.set_tuning(getattr(eng, "TUNE_" + k.upper()), 0)
    return out, {k: c1[k] - c0[k] for k in c1}, launches


def _run(eng, left, right, p, **tune):
    return _tuned(eng, lambda: eng.compute(left, right, synthetic.to_sm_params(p)), **tune)


def _run_batch(eng, pairs, p, **tune):
    import torch

    n = len(pairs)
    H, W = pairs[0][0].shape
    L = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
    R = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
    out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")

    def fn():
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.compute_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, synthetic.to_sm_params(p),
                                     out.data_ptr())
            eng.synchronize()
        finally:
            eng.set_stream(None)
        return out.cpu().numpy()

    return _tuned(eng, fn, **tune)


@functools.lru_cache(maxsize=None)
def _pair(H, W, seed):
    left, right, _ = synthetic.random_dot_pair(H, W, D, seed=seed)
    return left, right


@functools.lru_cache(maxsize=None)
def _expected(H, W, seed):
    return ref_c.compute(*_pair(H, W, seed), _params())


def _in_sweep(c, launches):
    """The call ran the lines chain with no patch launch and no fallback."""
    assert c["line_groups"] == 1, "the in-sweep lines ran"
    assert launches == 0, "no k_ew_patch launch"
    assert c["sweep_fallbacks"] == 0


@pytest.mark.parametrize("H", [9, 24, 41])
@pytest.mark.parametrize("wide", [True, False], ids=["strips4", "strip1"])
def test_small_shapes(eng, H, wide):
    """One halo block plus a row, rows that are no multiple of the patch waves, more rows than one
    round of them; three strips plus a ragged fourth, and one strip (nothing to patch, the rows'
    flags still published)."""
    W = D + (3 * CW + 5 if wide else 20)
    left, right = _pair(H, W, 500 + H)
    out, c, launches = _run(eng, left, right, _params(), ew_patch=IN_SWEEP)
    exp = _expected(H, W, 500 + H)
    assert np.array_equal(out, exp), f"{np.sum(out != exp)} px differ"
    _in_sweep(c, launches)


def test_every_segment_repaired_batch(eng):
    """A wrong start state and the shortest warmup: nearly every strip of every row is repaired, so
    a partial load that passed its row's patch would show as differing pixels.  Five pairs: each
    pair's strips and patch waves spread over the XCDs."""
    H, W, n = 41, D + 3 * CW + 5, 5
    pairs = [_pair(H, W, 700 + i) for i in range(n)]
    p = _params()
    got, c, launches = _run_batch(eng, pairs, p, ew_patch=IN_SWEEP, ew_guess=1, ew_warmup=1)
    exp = ref_c.compute_many(pairs, p)
    for i in range(n):
        assert np.array_equal(got[i], exp[i]), (i, int(np.sum(got[i] != exp[i])))
    _in_sweep(c, launches)
    # three interior boundaries per row and direction, nearly all of them repaired
    assert c["ew_repairs"] >= n * H * 2 * 3 // 2, c["ew_repairs"]


def _bands(H, W, period, seed):
    """Textureless vertical bands alternating with random texture (tests/test_gpu_ew_start.py)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    flat = (np.arange(W) // period) % 2 == 0
    img[:, flat] = 90
    return img


CARRY = {
    "wide_bands": lambda H, W: (_bands(H, W, 150, 2), np.roll(_bands(H, W, 150, 2), -3, axis=1)),
    "const": lambda H, W: (np.full((H, W), 77, np.uint8), np.full((H, W), 77, np.uint8)),
}


@pytest.mark.parametrize("name", list(CARRY))
def test_carries_and_equivalence(eng, name):
    """Textureless bands wider than a strip: walks that never meet inside their strip, carried on
    by phase B.  In the sweep and as a launch: the maps equal the oracle's and each other, the same
    walks run (equal repair and open-strip counts), no fallback.  That `wide_bands` leaves open
    walks was checked on the CPU with oracle.sgm_np's recurrence step over the census costs (the
    speculative and the true trajectory of every interior strip boundary stepped side by side
    from the 9-column cost-derived start): 161 of 207 phase-A walks never meet at 36-column
    strips, 299 of 367 at 20, 533 of 583 at 12 (the strip widths a one-pair call can take)."""
    H, W = 23, 3 * D + 257
    left, right = CARRY[name](H, W)
    p = _params()
    exp = ref_c.compute(left, right, p)
    res = {}
    for key, where in (("sweep", IN_SWEEP), ("launch", LAUNCH)):
        out, c, launches = _run(eng, left, right, p, ew_patch=where)
        assert np.array_equal(out, exp), f"{key}: {np.sum(out != exp)} px differ"
        assert c["sweep_fallbacks"] == 0 and c["line_groups"] == 1
        assert launches == (0 if where == IN_SWEEP else 1), (key, launches)
        res[key] = c
    print(name, {k: (v["ew_repairs"], v["ew_open"]) for k, v in res.items()})
    assert res["sweep"]["ew_repairs"] == res["launch"]["ew_repairs"]
    assert res["sweep"]["ew_open"] == res["launch"]["ew_open"]
    if name == "wide_bands":
        assert res["sweep"]["ew_open"] > 0, "the input produces open walks"


def test_equivalence_random(eng):
    """A textured pair with the default start state: the same maps, walks and open strips from the
    patch waves as from the launch."""
    H, W = 41, D + 3 * CW + 5
    left, right = _pair(H, W, 541)
    res = {}
    for key, where in (("sweep", IN_SWEEP), ("launch", LAUNCH)):
        out, c, _ = _run(eng, left, right, _params(), ew_patch=where, ew_warmup=1)
        assert np.array_equal(out, _expected(H, W, 541)), key
        res[key] = c
    for k in ("ew_repairs", "ew_open", "sweep_fallbacks"):
        assert res["sweep"][k] == res["launch"][k], (k, res)
    assert res["sweep"]["sweep_fallbacks"] == 0


def test_kitti_batch(eng):
    """The workload's own size, 8 KITTI pairs in one launch (248 workgroups, one per CU, over the
    8 XCDs: their co-residency and spread cannot be reproduced smaller): every pair equals the
    oracle."""
    H, W, _ = synthetic.CONFIGS["kitti"]
    n = 8
    pairs = [synthetic.random_dot_pair(H, W, D, seed=4100 + i)[:2] for i in range(n)]
    p = _params()
    got, c, launches = _run_batch(eng, pairs, p, ew_patch=IN_SWEEP)
    exp = ref_c.compute_many(pairs, p)
    for i in range(n):
        assert np.array_equal(got[i], exp[i]), (i, int(np.sum(got[i] != exp[i])))
    _in_sweep(c, launches)


def test_patch_tuning_arguments(eng):
    for bad in (-2, 2):
        with pytest.raises(ValueError):
            eng.set_tuning(eng.TUNE_EW_PATCH, bad)
    for ok in (-1, 1, 0):
        eng.set_tuning(eng.TUNE_EW_PATCH, ok)
