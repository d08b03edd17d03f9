"""GPU: call patterns on one context.  sm_ctx owns scratch shared across calls and subsystems (the
staging images, the two buffer sets, the strip hand-off granules with their 16-bit epoch tag, the
line / band states, the twin context and the side streams), and every other GPU test makes one
call and then synchronises.  Here: asynchronous calls queued back to back with one host sync at
the end, a stream switch between two calls, small geometries after large ones of another layout,
host-pointer calls of every subsystem interleaved on the shared staging, one batch repeated, and
the wrap of the hand-off epoch (SM_TUNE_HOP_EPOCH).  Every result is checked against its oracle
(bit-exact, as in the entry points' own tests), sm_synchronize must not report a hand-off
time-out, and SM_COUNTER_SWEEP_FALLBACKS must not move: the guarded fallback would recompute the
right answer over a broken hand-off."""
import numpy as np
import pytest

import filters_np
import nlm_np
import rectify_np
import strided as S
from oracle import ref_c, reproject_np, sgm_np
from stereo_match_amd import _lib, filters, pointcloud, synthetic

pytestmark = pytest.mark.gpu

SWEEP8, NARROW, OVERLAP = 16384, 1 << 19, 64
SMALL = (23, 150, 32)
STRIPS = (24, 128 + 3 * 36 + 5, 128)  # three strips plus a ragged fourth (tests/test_gpu_ew_start.py)


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


class Queue:
    """Calls queued on torch's current stream under debug flags; one sm_synchronize at the end,
    which must not raise, and no sweep group may have fallen back."""

    def __init__(self, eng, flags=0, stream=True):
        self.eng, self.flags, self.stream = eng, flags, stream

    def __enter__(self):
        import torch

        self.c0 = self.eng.counters()
        if self.stream:
            self.eng.set_stream(torch.cuda.current_stream().cuda_stream)
        self.eng.set_debug_flags(self.flags)
        return self

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                self.eng.synchronize()
        finally:
            self.eng.set_debug_flags(0)
            self.eng.set_stream(None)
        if et is None:
            self.c1 = self.eng.counters()
            assert self.c1["sweep_fallbacks"] == self.c0["sweep_fallbacks"], "a sweep group fell back"
        return False


def upload(images):
    import torch

    L = torch.tensor(np.stack([a for a, _ in images]), device="cuda")
    R = torch.tensor(np.stack([b for _, b in images]), device="cuda")
    return L, R


def assert_maps(got, exp, what=""):
    for i, e in enumerate(exp):
        assert np.array_equal(got[i], e), f"{what} pair {i}: {int((got[i] != e).sum())} px differ"


# ---- back to back, no host sync
@pytest.mark.parametrize("flags", [0, OVERLAP], ids=["default", "overlap"])
@pytest.mark.parametrize("cost,mode", [(1, 8), (0, 5)], ids=["census8", "sgbm5"])
def test_three_batches_back_to_back(eng, cost, mode, flags):
    """Three 7-pair calls (launch groups of 4 + 3 under flag 64) with different pairs and outputs:
    the second call's kernels reuse the buffer sets the first call's second stream may still read."""
    H, W, D = SMALL
    n = 7
    p = S.sgbm_params(cost, D, mode)
    sp = synthetic.to_sm_params(p)
    ins = [upload(S.pairs(H, W, D, n, seed)) for seed in (1, 2, 3)]
    outs = [S.guarded(n, H, W) for _ in ins]
    with Queue(eng, flags):
        for (L, R), o in zip(ins, outs):
            eng.compute_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, sp, o[1])
    for seed, o in zip((1, 2, 3), outs):
        assert_maps(S.maps_of(o, n, H, W), S.expected(H, W, D, n, S.key(p), seed), f"call {seed}")


@pytest.mark.parametrize("cost,mode", [(0, 5), (1, 8)], ids=["sgbm5", "census8"])
def test_two_compute_disparity_calls_back_to_back(eng, cost, mode):
    """The twin context, lr_stream and wls_stream of call 1 against call 2's kernels."""
    H, W, D = SMALL
    n = 3
    settings = S.sgbm_params(cost, D, mode)
    wp, wd = S.default_wls(settings)
    ins = [upload(S.pairs(H, W, D, n, seed)) for seed in (4, 5)]
    outs = [[S.guarded(n, H, W) for _ in range(3)] for _ in ins]
    with Queue(eng):
        for (L, R), o in zip(ins, outs):
            eng.compute_disparity_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W,
                                               synthetic.to_sm_params(settings), wp, *(x[1] for x in o))
    for seed, o in zip((4, 5), outs):
        dl, dr = S.lr_maps(H, W, D, n, S.key(settings), seed)
        ef = S.expected_wls(H, W, D, n, S.key(settings), S.key(wd), seed)
        gl, gr, gf = (S.maps_of(x, n, H, W) for x in o)
        assert_maps(gl, dl, f"displ, call {seed}")
        assert_maps(gr, dr, f"dispr, call {seed}")
        assert_maps(gf, ef, f"filtered, call {seed}")


def test_device_chain_matchers_wls_speckles(eng):
    """Left matcher, right matcher, the WLS filter on their outputs, the speckle filter on its
    output in place: nothing returns to the host in between."""
    H, W, D = SMALL
    n = 3
    settings = synthetic.parity_params(D)
    wp, wd = S.default_wls(settings)
    lp = dict(settings, uniquenessRatio=0, disp12MaxDiff=1000000)
    rp = sgm_np.right_matcher_params(settings)
    L, R = upload(S.pairs(H, W, D, n, 6))
    dl, dr, fo = (S.guarded(n, H, W) for _ in range(3))
    with Queue(eng):
        eng.compute_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, synthetic.to_sm_params(lp), dl[1])
        eng.compute_batch_device(R.data_ptr(), L.data_ptr(), n, H * W, H, W, W, synthetic.to_sm_params(rp), dr[1])
        eng.wls_filter_batch_device(dl[1], dr[1], L.data_ptr(), n, H * W, W, H, W, wp, fo[1])
        eng.filter_speckles_device(fo[1], n, H, W, -16, 60, 32)
    el, er = S.lr_maps(H, W, D, n, S.key(settings), 6)
    assert_maps(S.maps_of(dl, n, H, W), el, "displ")
    assert_maps(S.maps_of(dr, n, H, W), er, "dispr")
    ef = S.expected_wls(H, W, D, n, S.key(settings), S.key(wd), 6)
    got = S.maps_of(fo, n, H, W)
    changed = 0
    for i in range(n):
        exp = sgm_np.filter_speckles(ef[i], -16, 60, 32)
        changed += int((exp != ef[i]).sum())
        assert np.array_equal(got[i], exp), f"speckle-filtered pair {i}: {int((got[i] != exp).sum())} px differ"
    assert changed > 0, "the speckle filter removes something here"


def test_stream_switch_between_two_calls(eng):
    """Call 1 on stream s1, then, after s2.wait_stream(s1), call 2 on s2 through sm_set_stream."""
    import torch

    H, W, D = SMALL
    n = 7
    p = S.sgbm_params(1, D, 8)
    sp = synthetic.to_sm_params(p)
    ins = [upload(S.pairs(H, W, D, n, seed)) for seed in (1, 2)]
    outs = [S.guarded(n, H, W) for _ in ins]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()  # the inputs and the sentinel-filled outputs are in place
    c0 = eng.counters()
    eng.set_debug_flags(OVERLAP)
    try:
        eng.set_stream(s1.cuda_stream)
        eng.compute_batch_device(ins[0][0].data_ptr(), ins[0][1].data_ptr(), n, H * W, H, W, W, sp, outs[0][1])
        s2.wait_stream(s1)
        eng.set_stream(s2.cuda_stream)
        eng.compute_batch_device(ins[1][0].data_ptr(), ins[1][1].data_ptr(), n, H * W, H, W, W, sp, outs[1][1])
        eng.synchronize()
        s1.synchronize()
        s2.synchronize()
    finally:
        eng.set_debug_flags(0)
        eng.set_stream(None)
    assert eng.counters()["sweep_fallbacks"] == c0["sweep_fallbacks"]
    for seed, o in zip((1, 2), outs):
        assert_maps(S.maps_of(o, n, H, W), S.expected(H, W, D, n, S.key(p), seed), f"call {seed}")


# ---- geometry and layout sequence
def _batch(eng, shape, n, p, flags, seed=0):
    H, W, D = shape
    L, R = upload(S.pairs(H, W, D, n, seed))
    out = S.guarded(n, H, W)
    with Queue(eng, flags) as q:
        eng.compute_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, synthetic.to_sm_params(p), out[1])
    got = S.maps_of(out, n, H, W)
    assert_maps(got, S.expected(H, W, D, n, S.key(p), seed), str(shape))
    return got.copy(), q


def _host(eng, shape, p, flags, seed=0):
    H, W, D = shape
    a, b = S.pairs(H, W, D, 1, seed)[0]
    with Queue(eng, flags, stream=False):
        out = eng.compute(a, b, synthetic.to_sm_params(p))
    assert np.array_equal(out, S.expected(H, W, D, 1, S.key(p), seed)[0]), shape


@pytest.mark.parametrize("extra", [0, NARROW], ids=["auto_strips", "narrow_strips"])
def test_geometry_and_layout_sequence(eng, extra):
    """Each large call is the poison for the small one after it: stale hand-off granules, line and
    band states and partial sums of another layout."""
    big = (60, 330, 128)
    p1 = S.sgbm_params(1, 128, 8)
    first, q = _batch(eng, big, 3, p1, SWEEP8 | extra)  # fused sweeps, in-sweep lines
    if not extra:
        assert q.c1["line_groups"] > q.c0["line_groups"], "the in-sweep lines ran"
    _host(eng, (7, 45, 16), S.sgbm_params(0, 16, 5), extra)
    Hv, Wv, Dv = 33, 200, 48
    l, r = S.pairs(Hv, Wv, Dv, 1)[0]
    vol = synthetic.absdiff_volume(l, r, Dv)[0]
    pv = synthetic.cost_volume_params(Dv)
    with Queue(eng, extra, stream=False):
        o = eng.aggregate_cost_f32(vol, synthetic.to_sm_params(pv), 0.0, synthetic.VOLUME_SCALE)
    assert np.array_equal(o, ref_c.compute_volume(vol, pv, 0.0, synthetic.VOLUME_SCALE))
    _batch(eng, (40, 260, 64), 2, S.sgbm_params(0, 64, 8), SWEEP8 | extra)
    _host(eng, (5, 30, 16), S.sgbm_params(1, 16, 8), extra)
    last, _ = _batch(eng, big, 3, p1, SWEEP8 | extra)
    assert np.array_equal(first, last)


# ---- shared staging across subsystems
Q_CALC = np.float32([[1, 0, 0, -640], [0, -1, 0, 360], [0, 0, 0, -1164], [0, 0, 1, 0]])


def _verts_equal(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn],
                                                                                 want.view(np.uint32)[~wn])


def test_host_calls_interleaved_on_the_shared_staging(eng):
    """compute, remap, StereoBM, gauss2d / image_measure, the WLS filter, the point cloud, the
    denoiser with two h in a row (its weight-table cache), compute again: small, large, small
    sizes on the context's staging images, output map and pinned buffer."""
    H, W, D = SMALL
    p = S.sgbm_params(1, D, 8)
    a, b = S.pairs(H, W, D, 1)[0]

    def compute_small():
        assert np.array_equal(eng.compute(a, b, synthetic.to_sm_params(p)), S.expected(H, W, D, 1, S.key(p))[0])

    rng = np.random.default_rng(77)
    compute_small()
    src = rng.integers(0, 256, (37, 67, 3), dtype=np.uint8)
    mx = rng.uniform(-3, 70, (19, 259)).astype(np.float32)
    my = rng.uniform(-3, 40, (19, 259)).astype(np.float32)
    dst, gray = eng.remap(src, mx, my, True, True)
    exp = rectify_np.remap(src, mx, my)
    assert np.array_equal(dst, exp) and np.array_equal(gray, rectify_np.bgr2gray(exp))
    Hb, Wb, Db = 33, 229, 64
    bp = dict(numDisparities=Db, blockSize=9)
    la, lb = S.pairs(Hb, Wb, Db, 1)[0]
    assert np.array_equal(eng.bm_compute(la, lb, S.bm_params(bp)), S.expected_bm(Hb, Wb, Db, 1, S.key(bp))[0])
    f64 = filters_np.image_f64(37, 67, 5)
    half = filters._half(3, 4.0)
    assert np.array_equal(eng.gauss2d(f64, half, half), filters_np.gaussian_filter(f64, 3))
    u8 = filters_np.image_u8(37, 67, 6, 3)
    w1, w2 = filters._measure_kernels()
    assert np.array_equal(eng.image_measure(u8, w1, w2, 30.0), filters_np.image_measure(u8))
    compute_small()
    settings = synthetic.parity_params(D)
    _, wd = S.default_wls(settings)
    dl, dr = S.lr_maps(H, W, D, 1, S.key(settings))
    assert np.array_equal(eng.wls_filter(dl[0], a, dr[0], S.wls_params(wd, H, W)),
                          S.expected_wls(H, W, D, 1, S.key(settings), S.key(wd))[0])
    i = np.arange(37 * 53, dtype=np.int64).reshape(37, 53)
    d = ((i * 37 % 97) * 4 - 16).astype(np.int16)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    verts, colors = eng.cloud_extract(d, 0, img, Q_CALC, pointcloud._cloud_params(None, None, False, False))
    with np.errstate(all="ignore"):
        pts = np.ascontiguousarray(reproject_np.reproject_image_to_3d(d, Q_CALC, False).reshape(-1, 3), np.float32)
    assert _verts_equal(verts, pts) and np.array_equal(colors, img[..., ::-1].reshape(-1, 3))
    noisy = nlm_np.noisy_blobs(37, 67, 11)
    for h in (10, 30):
        assert np.array_equal(eng.nlm_denoise(noisy, h, 7, 21), nlm_np.denoise(noisy, h, 7, 21)[0]), h
    compute_small()
    eng.synchronize()


# ---- repeatability
@pytest.mark.parametrize("cost,mode,flags", [(0, 5, 0), (1, 8, SWEEP8)], ids=["sgbm5_default", "census8_sweeps"])
def test_same_strided_batch_five_times(eng, cost, mode, flags):
    """The strip hand-off is lock-free: five runs of one strided 3-pair batch on the reused
    context, queued back to back, give the oracle's maps every time."""
    H, W, D = STRIPS
    n = 3
    p = S.sgbm_params(cost, D, mode)
    images = S.pairs(H, W, D, n)
    st = W + 13
    ps = H * st + 77
    L, pl = S.embed([a for a, _ in images], st, ps, 1, 0xFF)
    R, pr = S.embed([b for _, b in images], st, ps, 0, 0x00)
    outs = [S.guarded(n, H, W) for _ in range(5)]
    with Queue(eng, flags):
        for o in outs:
            eng.compute_batch_device(pl, pr, n, ps, H, W, st, synthetic.to_sm_params(p), o[1])
    exp = S.expected(H, W, D, n, S.key(p))
    for r, o in enumerate(outs):
        assert_maps(S.maps_of(o, n, H, W), exp, f"run {r}")


# ---- the epoch wrap of the strip hand-off granules
@pytest.mark.parametrize("cost,mode", [(1, 8), (0, 5), (1, 5), (0, 8)], ids=["census8", "sgbm5", "census5", "sgbm8"])
def test_hop_epoch_wrap(cost, mode):
    """The granules carry a 16-bit epoch tag; after 65535 sweep launches sm_api.hip clears them and
    restarts at epoch 1.  A few multi-strip calls at low epochs, a few from 0xFFF0 (high tags in
    the granules), then 12 calls from 0xFFFA across the wrap (one sweep launch per call at 5
    paths, two at 8: at least 7 launches after it).  A stale tag accepted as fresh gives wrong
    pixels, a fresh one rejected a fallback."""
    H, W, D = STRIPS
    p = S.sgbm_params(cost, D, mode)
    sp = synthetic.to_sm_params(p)
    a, b = S.pairs(H, W, D, 1)[0]
    exp = S.expected(H, W, D, 1, S.key(p))[0]
    e = _lib.Engine(0)
    try:
        e.set_debug_flags(SWEEP8)
        c0 = e.counters()
        for epoch, calls in ((0, 2), (0xFFF0, 3), (0xFFFA, 12)):
            e.set_tuning(e.TUNE_HOP_EPOCH, epoch)
            for k in range(calls):
                out = e.compute(a, b, sp)
                assert np.array_equal(out, exp), f"from epoch {epoch:#x}, call {k}: {int((out != exp).sum())} px differ"
        e.synchronize()
        c1 = e.counters()
        assert c1["sweep_fallbacks"] == c0["sweep_fallbacks"]
    finally:
        e.close()


def test_hop_epoch_wrap_reaches_the_twin_context():
    """sm_set_tuning forwards the key: the right matcher of sm_compute_disparity runs on the twin
    context's own granules, which cross the wrap with the left one's."""
    H, W, D = STRIPS
    settings = synthetic.parity_params(D)
    wp, wd = S.default_wls(settings)
    a, b = S.pairs(H, W, D, 1)[0]
    dl, _ = S.lr_maps(H, W, D, 1, S.key(settings))
    ef = S.expected_wls(H, W, D, 1, S.key(settings), S.key(wd))[0]
    e = _lib.Engine(0)
    try:
        e.set_debug_flags(SWEEP8)
        c0 = e.counters()
        for epoch, calls in ((0, 1), (0xFFFA, 10)):
            e.set_tuning(e.TUNE_HOP_EPOCH, epoch)
            for k in range(calls):
                d, f = e.compute_disparity(a, b, synthetic.to_sm_params(settings), wp)
                assert np.array_equal(d, dl[0]) and np.array_equal(f, ef), (epoch, k)
        e.synchronize()
        assert e.counters()["sweep_fallbacks"] == c0["sweep_fallbacks"]
    finally:
        e.close()


def test_hop_epoch_tuning_arguments(eng):
    for bad in (-1, 0x10000):
        with pytest.raises(ValueError):
            eng.set_tuning(eng.TUNE_HOP_EPOCH, bad)
    eng.set_tuning(eng.TUNE_HOP_EPOCH, 0)  # changes nothing
