"""GPU: the matcher-core entry points on strided, gapped and misaligned inputs.  Every other GPU
test hands these entry points packed images (stride == W * channels, pair stride == H * stride);
here every batch lies in a poisoned buffer (tests/strided.py embed: row padding, gaps between the
pairs, a lead-in and a tail, left and right at different alignments), each case runs with two
different fills, the outputs lie between sentinel guards, and the oracle is always fed the packed
images.  Bars as in the entry points' own tests: the matcher, StereoBM and the speckle filter
bit-exact against oracle/ref_c.py, oracle/bm_np.py and oracle/sgm_np.py; the WLS filter bit-exact
against oracle/wls_np.py (tests/test_gpu_wls.py's comparison).  The guarded per-direction fallback
would hide a broken strip hand-off, so SM_COUNTER_SWEEP_FALLBACKS must not move."""
import ctypes

import numpy as np
import pytest

import strided as S
from oracle import sgm_np
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

PERDIR, SWEEP8, NARROW, WIDE, OVERLAP = 4096, 16384, 16384 | (1 << 19), 16384 | (1 << 21), 64

# (H, W, D): ragged in every tile dimension, more than one sweep strip; one W < D
SHAPES = [(23, 150, 32), (33, 229, 64), (9, 40, 64)]
# three strips plus a ragged fourth of the wide D = 128 lines instance (tests/test_gpu_ew_start.py)
LINES_SHAPE = (24, 128 + 3 * 36 + 5, 128)


def stride_set(k, H, W, cn=1):
    """(stride, pair_stride, left base offset, right base offset): 0 and 1 odd strides with a gap
    and / or alignments that differ modulo 16 between left and right, 2 aligned and wider than W."""
    row = W * cn
    if k == 0:
        st = row + 1
        return st, H * st + 77, 1, 0
    if k == 1:
        st = row + 13
        return st, H * st, 0, 1
    st = -(-(row + 1) // 256) * 256
    return st, H * st, 0, 0


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


class Call:
    """Debug flags, tuning keys and torch's current stream around a call; no fallback in it."""

    def __init__(self, eng, flags=0, **tune):
        self.eng, self.flags, self.tune = eng, flags, tune

    def __enter__(self):
        import torch

        e = self.eng
        self.c0 = e.counters()
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.set_debug_flags(self.flags)
        for k, v in self.tune.items():
            e.set_tuning(getattr(e, "TUNE_" + k.upper()), v)
        return self

    def __exit__(self, et, ev, tb):
        e = self.eng
        try:
            if et is None:
                e.synchronize()  # raises if a sweep strip hand-off timed out
        finally:
            e.set_debug_flags(0)
            for k in self.tune:
                e.set_tuning(getattr(e, "TUNE_" + k.upper()), 0)
            e.set_stream(None)
        if et is None:
            self.c1 = e.counters()
            assert self.c1["sweep_fallbacks"] == self.c0["sweep_fallbacks"], "a sweep group fell back"
        return False

    def grew(self, name):
        return self.c1[name] - self.c0[name]


def run_batch(eng, images, k, p, flags=0, cn=1, wta=False, single=False, **tune):
    """sm_compute_batch_device_cn (sm_compute_device: single; sm_compute_wta_batch_device: wta) on
    the pairs embedded with stride set k, once per fill: [(maps, wta maps or None, Call)]."""
    n = len(images)
    H, W = images[0][0].shape[:2]
    st, ps, ol, orr = stride_set(k, H, W, cn)
    sp = synthetic.to_sm_params(p)
    res = []
    for fill in S.FILLS:
        L, pl = S.embed([a for a, _ in images], st, ps, ol, fill)
        R, pr = S.embed([b for _, b in images], st, ps, orr, fill)
        assert ol == orr or pl % 16 != pr % 16
        out = S.guarded(n, H, W)
        wout = S.guarded(n, H, W) if wta else None
        with Call(eng, flags, **tune) as c:
            if wta:
                eng.compute_wta_batch_device(pl, pr, n, ps, H, W, st, sp, out[1], wout[1])
            elif single:
                eng.compute_device(pl, pr, H, W, st, sp, out[1])
            else:
                eng.compute_batch_device(pl, pr, n, ps, H, W, st, sp, out[1], channels=cn)
        assert S.unchanged(L) and S.unchanged(R), "the call wrote into its input"
        res.append((S.maps_of(out, n, H, W), S.maps_of(wout, n, H, W) if wta else None, c))
    return res


def check(res, exp, what=""):
    for fill, (got, _, _) in zip(S.FILLS, res):
        for i, e in enumerate(exp):
            assert np.array_equal(got[i], e), f"{what} fill {fill:#x} pair {i}: {int((got[i] != e).sum())} px differ"


# ---- sm_compute_batch_device, gray: costs x paths x engines, shapes and stride sets rotating
ENGINES = [("default", 0, 3), ("perdir", PERDIR, 3), ("sweep8_1pair", SWEEP8, 1), ("narrow", NARROW, 2),
           ("wide", WIDE, 2), ("overlap_7pairs", OVERLAP, 7)]
GRAY = []
for _ci, (_cost, _mode) in enumerate([(1, 8), (1, 5), (0, 5), (0, 8)]):
    for _ei, (_name, _flags, _n) in enumerate(ENGINES):
        _k = _ci + _ei
        _si = (_k + _ei // 3) % 3
        # W < D has no valid column (every pixel invalid whatever is read): such a combination
        # runs on one of the other shapes too
        for _s in ([_si] if _si < 2 else [2, _ei % 2]):
            GRAY.append(pytest.param(_cost, _mode, _flags, _n, SHAPES[_s], _k % 3,
                                     id=f"c{_cost}p{_mode}_{_name}_shape{_s}_set{_k % 3}"))


@pytest.mark.parametrize("cost,mode,flags,n,shape,k", GRAY)
def test_batch_device_gray(eng, cost, mode, flags, n, shape, k):
    H, W, D = shape
    p = S.sgbm_params(cost, D, mode)
    res = run_batch(eng, S.pairs(H, W, D, n), k, p, flags)
    check(res, S.expected(H, W, D, n, S.key(p)))


@pytest.mark.parametrize("k", [0, 2])
def test_batch_device_in_sweep_lines(eng, k):
    """Census, 8 paths, the fused sweeps with the E/W paths inside the down sweep (the bench's
    engine): SM_COUNTER_LINE_GROUPS shows that this engine read the strided images."""
    H, W, D = LINES_SHAPE
    p = S.sgbm_params(1, D, 8)
    res = run_batch(eng, S.pairs(H, W, D, 2), k, p, SWEEP8)
    check(res, S.expected(H, W, D, 2, S.key(p)))
    assert all(c.grew("line_groups") > 0 for _, _, c in res), "the in-sweep lines ran"


@pytest.mark.parametrize("cost,k", [(1, 1), (0, 0)])
def test_batch_device_row_bands(eng, cost, k):
    """5 paths, one pair, three row bands (tests/test_gpu_round6.py): SM_COUNTER_BAND_GROUPS."""
    H, W, D = (33, 229, 64) if cost else (33, 150, 32)
    p = S.sgbm_params(cost, D, 5)
    res = run_batch(eng, S.pairs(H, W, D, 1), k, p, SWEEP8, bands=3)
    check(res, S.expected(H, W, D, 1, S.key(p)))
    assert all(c.grew("band_groups") > 0 for _, _, c in res), "the banded instance ran"


# ---- sm_compute_batch_device_cn, 3 channels
# the wide x86-saturation path: tests/test_gpu_wide.py's TRY_TRY at 32 disparities
TRY_TRY_32 = dict(minDisparity=16, numDisparities=32, blockSize=16, P1=8 * 3 * 9, P2=32 * 3 * 9, disp12MaxDiff=1,
                  uniquenessRatio=10, speckleWindowSize=100, speckleRange=32, preFilterCap=0, mode=5, cost=0)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("path", ["int16_exact_bs7", "wide_bs16"])
def test_batch_device_bgr(eng, path, k):
    """channels = 3: stride 3 W + 1 with a gap, 3 W + 13, and aligned."""
    H, W, D = SHAPES[0]
    p = dict(synthetic.parity_params(D), blockSize=7) if path == "int16_exact_bs7" else TRY_TRY_32
    res = run_batch(eng, S.bgr_pairs(H, W, D, 3), k, p, cn=3)
    check(res, S.expected(H, W, D, 3, S.key(p), 0, 3))


def test_batch_device_bgr_stride_3w_plus_5(eng):
    H, W, D, n = 33, 229, 64, 3
    p = dict(synthetic.parity_params(D), blockSize=7)
    images = S.bgr_pairs(H, W, D, n)
    st = 3 * W + 5
    ps = H * st + 77
    sp = synthetic.to_sm_params(p)
    for fill in S.FILLS:
        L, pl = S.embed([a for a, _ in images], st, ps, 1, fill)
        R, pr = S.embed([b for _, b in images], st, ps, 0, fill)
        out = S.guarded(n, H, W)
        with Call(eng):
            eng.compute_batch_device(pl, pr, n, ps, H, W, st, sp, out[1], channels=3)
        got = S.maps_of(out, n, H, W)
        for i, e in enumerate(S.expected(H, W, D, n, S.key(p), 0, 3)):
            assert np.array_equal(got[i], e), (fill, i)


# ---- sm_compute_device and sm_compute_wta_batch_device
@pytest.mark.parametrize("cost,mode,shape,k", [(1, 8, SHAPES[0], 0), (0, 5, SHAPES[1], 1), (1, 5, SHAPES[2], 0),
                                               (0, 8, SHAPES[1], 2)])
def test_compute_device_single_pair(eng, cost, mode, shape, k):
    H, W, D = shape
    p = S.sgbm_params(cost, D, mode)
    res = run_batch(eng, S.pairs(H, W, D, 1), k, p, single=True)
    check(res, S.expected(H, W, D, 1, S.key(p)))


@pytest.mark.parametrize("cost,mode,flags,shape,k", [(1, 8, 0, SHAPES[1], 0), (0, 5, 0, SHAPES[0], 1),
                                                     (0, 8, PERDIR, SHAPES[1], 2), (1, 5, SWEEP8, SHAPES[0], 0),
                                                     (0, 5, 0, SHAPES[2], 1)])
def test_wta_batch_device(eng, cost, mode, flags, shape, k):
    """Both outputs (the disparity maps and the integer WTA index) against ref_c.compute_wta."""
    H, W, D = shape
    p = S.sgbm_params(cost, D, mode)
    res = run_batch(eng, S.pairs(H, W, D, 3), k, p, flags, wta=True)
    exp = S.expected_wta(H, W, D, 3, S.key(p))
    for fill, (got, wta, _) in zip(S.FILLS, res):
        for i, (d, w) in enumerate(exp):
            assert np.array_equal(got[i], d), f"disparity, fill {fill:#x} pair {i}"
            assert np.array_equal(wta[i], w), f"WTA index, fill {fill:#x} pair {i}"


# ---- sm_bm_compute_batch_device
BM_CASES = [(SHAPES[0], dict(blockSize=9), 0), (SHAPES[1], dict(blockSize=15, minDisparity=-3, disp12MaxDiff=1), 1),
            (SHAPES[1], dict(blockSize=5, textureThreshold=200, uniquenessRatio=5, speckleWindowSize=30,
                             speckleRange=16), 2),
            (SHAPES[0], dict(blockSize=21, preFilterCap=15), 0)]


@pytest.mark.parametrize("shape,extra,k", BM_CASES, ids=[f"case{i}" for i in range(len(BM_CASES))])
def test_bm_batch_device(eng, shape, extra, k):
    H, W, D = shape
    n = 3
    p = dict(numDisparities=D, **extra)
    images = S.pairs(H, W, D, n)
    st, ps, ol, orr = stride_set(k, H, W)
    for fill in S.FILLS:
        L, pl = S.embed([a for a, _ in images], st, ps, ol, fill)
        R, pr = S.embed([b for _, b in images], st, ps, orr, fill)
        out = S.guarded(n, H, W)
        with Call(eng):
            eng.bm_compute_batch_device(pl, pr, n, ps, H, W, st, S.bm_params(p), out[1])
        assert S.unchanged(L) and S.unchanged(R)
        got = S.maps_of(out, n, H, W)
        for i, e in enumerate(S.expected_bm(H, W, D, n, S.key(p))):
            assert np.array_equal(got[i], e), f"fill {fill:#x} pair {i}: {int((got[i] != e).sum())} px differ"


# ---- sm_wls_filter_batch_device
WLS_CASES = [
    # (shape, stride set, oracle params, with dispr)
    (SHAPES[0], 0, dict(lmbda=8000.0, sigma=1.5, radius=3, left_offset=32), True),
    (SHAPES[1], 1, dict(lmbda=80000.0, sigma=1.2, radius=3, left_offset=64), True),
    (SHAPES[1], 2, dict(lmbda=8000.0, sigma=0.7, radius=2, left_offset=64), True),
    (SHAPES[0], 1, dict(lmbda=8000.0, sigma=1.5, use_confidence=False), False),
    # a ROI away from every border: y0 / x0 combine with the guide's stride
    (SHAPES[1], 0, dict(lmbda=8000.0, sigma=1.5, radius=4, left_offset=67, right_offset=3, top_offset=2,
                        bottom_offset=1), True),
    (SHAPES[0], 0, dict(lmbda=10.0, sigma=3.0, use_confidence=False, left_offset=5, top_offset=3, bottom_offset=2,
                        right_offset=7), False),
]


@pytest.mark.parametrize("shape,k,wd,conf", WLS_CASES, ids=[f"case{i}" for i in range(len(WLS_CASES))])
def test_wls_filter_batch_device(eng, shape, k, wd, conf):
    """guide_stride > W, guide_pair_stride > H * guide_stride; the maps are packed ([n][H][W], as
    the header documents).  Exactly tests/test_gpu_wls.py's comparison: array_equal."""
    import torch

    H, W, D = shape
    n = 3
    settings = synthetic.parity_params(D)
    dl, dr = S.lr_maps(H, W, D, n, S.key(settings))
    exp = S.expected_wls(H, W, D, n, S.key(settings), S.key(wd), 0, conf)
    st, ps, ol, _ = stride_set(k, H, W)
    ps += (0, 77, 256)[k]  # every WLS case has a gap behind each guide
    for fill in S.FILLS:
        G, pg = S.embed([a for a, _ in S.pairs(H, W, D, n)], st, ps, ol, fill)
        tl = torch.tensor(np.stack(dl), device="cuda")
        tr = torch.tensor(np.stack(dr), device="cuda")
        out = S.guarded(n, H, W)
        with Call(eng):
            eng.wls_filter_batch_device(tl.data_ptr(), tr.data_ptr() if conf else None, pg, n, ps, st, H, W,
                                        S.wls_params(wd, H, W), out[1])
        assert S.unchanged(G)
        assert np.array_equal(tl.cpu().numpy(), np.stack(dl)) and np.array_equal(tr.cpu().numpy(), np.stack(dr))
        got = S.maps_of(out, n, H, W)
        for i, e in enumerate(exp):
            assert np.array_equal(got[i], e), f"fill {fill:#x} pair {i}: {int((got[i] != e).sum())} px differ"


# ---- sm_compute_disparity_batch_device: the twin context, lr_stream and wls_stream on strided images
@pytest.mark.parametrize("cost,mode,shape,k,n", [(0, 5, SHAPES[0], 0, 3), (0, 5, SHAPES[1], 1, 1),
                                                 (1, 8, SHAPES[1], 0, 2), (0, 8, SHAPES[0], 2, 3)])
def test_compute_disparity_batch_device(eng, cost, mode, shape, k, n):
    H, W, D = shape
    settings = S.sgbm_params(cost, D, mode)
    wp, wd = S.default_wls(settings)
    dl, dr = S.lr_maps(H, W, D, n, S.key(settings))
    ef = S.expected_wls(H, W, D, n, S.key(settings), S.key(wd))
    images = S.pairs(H, W, D, n)
    st, ps, ol, orr = stride_set(k, H, W)
    for fill in S.FILLS:
        L, pl = S.embed([a for a, _ in images], st, ps, ol, fill)
        R, pr = S.embed([b for _, b in images], st, ps, orr, fill)
        outs = [S.guarded(n, H, W) for _ in range(3)]
        with Call(eng):
            eng.compute_disparity_batch_device(pl, pr, n, ps, H, W, st, synthetic.to_sm_params(settings), wp,
                                               *(o[1] for o in outs))
        assert S.unchanged(L) and S.unchanged(R)
        gl, gr, gf = (S.maps_of(o, n, H, W) for o in outs)
        for i in range(n):
            assert np.array_equal(gl[i], dl[i]), f"displ, fill {fill:#x} pair {i}"
            assert np.array_equal(gr[i], dr[i]), f"dispr, fill {fill:#x} pair {i}"
            assert np.array_equal(gf[i], ef[i]), f"filtered, fill {fill:#x} pair {i}"


# ---- the host-pointer entry points, through ctypes: the Engine wrappers pack first
def host_view(img, fill, pad=13):
    """A view with strides[0] == W * cn + pad into a poisoned buffer with a row above and below;
    (view [H, W * cn], buffer)."""
    H = img.shape[0]
    row = int(np.prod(img.shape[1:]))
    buf = np.full((H + 2, row + pad), fill, np.uint8)
    view = buf[1:H + 1, :row]
    view[...] = img.reshape(H, row)
    assert view.strides[0] == row + pad and not view.flags.c_contiguous
    return view, buf


def _ok(eng, rc):
    assert rc == _lib.SM_OK, (rc, eng._lib.sm_last_error(eng.ctx))


@pytest.mark.parametrize("cn", [1, 3])
def test_host_sm_compute_cn(eng, cn):
    H, W, D = SHAPES[0]
    p = dict(synthetic.parity_params(D), blockSize=7) if cn == 3 else S.sgbm_params(1, D, 8)
    a, b = (S.bgr_pairs if cn == 3 else S.pairs)(H, W, D, 1)[0]
    for fill in S.FILLS:
        (va, ba), (vb, bb) = host_view(a, fill), host_view(b, fill)
        snap = ba.copy(), bb.copy()
        out = np.full((H + 2, W), S.SENTINEL, np.int16)
        _ok(eng, eng._lib.sm_compute_cn(eng.ctx, va.ctypes.data, vb.ctypes.data, H, W, va.strides[0], cn,
                                        ctypes.byref(synthetic.to_sm_params(p)), out[1:].ctypes.data))
        assert np.array_equal(out[1:H + 1], S.expected(H, W, D, 1, S.key(p), 0, cn)[0]), fill
        assert (out[0] == S.SENTINEL).all() and (out[H + 1] == S.SENTINEL).all()
        assert np.array_equal(ba, snap[0]) and np.array_equal(bb, snap[1])


@pytest.mark.parametrize("cost,mode", [(1, 8), (0, 5)])
def test_host_sm_compute_with_wta_out(eng, cost, mode):
    H, W, D = SHAPES[1]
    p = S.sgbm_params(cost, D, mode)
    a, b = S.pairs(H, W, D, 1)[0]
    ed, ew = S.expected_wta(H, W, D, 1, S.key(p))[0]
    for fill in S.FILLS:
        (va, _), (vb, _) = host_view(a, fill), host_view(b, fill)
        out, wta = np.empty((H, W), np.int16), np.empty((H, W), np.int16)
        _ok(eng, eng._lib.sm_compute(eng.ctx, va.ctypes.data, vb.ctypes.data, H, W, va.strides[0],
                                     ctypes.byref(synthetic.to_sm_params(p)), out.ctypes.data, wta.ctypes.data))
        assert np.array_equal(out, ed) and np.array_equal(wta, ew), fill


def test_host_sm_bm_compute(eng):
    H, W, D = SHAPES[1]
    p = dict(numDisparities=D, blockSize=9)
    a, b = S.pairs(H, W, D, 1)[0]
    for fill in S.FILLS:
        (va, _), (vb, _) = host_view(a, fill), host_view(b, fill)
        out = np.empty((H, W), np.int16)
        prm = S.bm_params(p)
        _ok(eng, eng._lib.sm_bm_compute(eng.ctx, va.ctypes.data, vb.ctypes.data, H, W, va.strides[0],
                                        ctypes.byref(prm), out.ctypes.data))
        assert np.array_equal(out, S.expected_bm(H, W, D, 1, S.key(p))[0]), fill


@pytest.mark.parametrize("conf", [True, False])
def test_host_sm_wls_filter(eng, conf):
    H, W, D = SHAPES[1]
    settings = synthetic.parity_params(D)
    wd = dict(lmbda=8000.0, sigma=1.5, radius=3, left_offset=D + 2, top_offset=1, use_confidence=conf)
    dl, dr = S.lr_maps(H, W, D, 1, S.key(settings))
    exp = S.expected_wls(H, W, D, 1, S.key(settings), S.key(wd), 0, conf)[0]
    for fill in S.FILLS:
        vg, _ = host_view(S.pairs(H, W, D, 1)[0][0], fill)
        out = np.empty((H, W), np.int16)
        prm = S.wls_params(wd, H, W)
        _ok(eng, eng._lib.sm_wls_filter(eng.ctx, dl[0].ctypes.data, dr[0].ctypes.data if conf else None,
                                        vg.ctypes.data, vg.strides[0], H, W, ctypes.byref(prm), out.ctypes.data))
        assert np.array_equal(out, exp), fill


def test_host_sm_compute_disparity(eng):
    H, W, D = SHAPES[0]
    settings = synthetic.parity_params(D)
    wp, wd = S.default_wls(settings)
    a, b = S.pairs(H, W, D, 1)[0]
    dl, _ = S.lr_maps(H, W, D, 1, S.key(settings))
    ef = S.expected_wls(H, W, D, 1, S.key(settings), S.key(wd))[0]
    for fill in S.FILLS:
        (va, _), (vb, _) = host_view(a, fill), host_view(b, fill)
        d, f = np.empty((H, W), np.int16), np.empty((H, W), np.int16)
        _ok(eng, eng._lib.sm_compute_disparity(eng.ctx, va.ctypes.data, vb.ctypes.data, H, W, va.strides[0],
                                               ctypes.byref(synthetic.to_sm_params(settings)), ctypes.byref(wp),
                                               d.ctypes.data, f.ctypes.data))
        assert np.array_equal(d, dl[0]) and np.array_equal(f, ef), fill


# ---- refusals
def test_stride_below_the_row_is_refused(eng):
    """stride < W * channels: SM_E_ARG from every entry point above, nothing written, and the
    context still computes."""
    import torch

    H, W, D = SHAPES[0]
    sp = synthetic.to_sm_params(synthetic.parity_params(D))
    bp = S.bm_params(dict(numDisparities=D, blockSize=9))
    wp = _lib.wls_default_params(sp)
    img = torch.zeros(3 * H * W * 3, dtype=torch.uint8, device="cuda")
    maps = torch.zeros(3 * H * W, dtype=torch.int16, device="cuda")
    outs = [torch.full((3 * H * W,), S.SENTINEL, dtype=torch.int16, device="cuda") for _ in range(3)]
    i, m, o = img.data_ptr(), maps.data_ptr(), [t.data_ptr() for t in outs]
    device_calls = [
        lambda: eng.compute_batch_device(i, i, 3, H * W, H, W, W - 1, sp, o[0]),
        lambda: eng.compute_batch_device(i, i, 3, 3 * H * W, H, W, 3 * W - 1, sp, o[0], channels=3),
        lambda: eng.compute_device(i, i, H, W, W - 1, sp, o[0]),
        lambda: eng.compute_wta_batch_device(i, i, 3, H * W, H, W, W - 1, sp, o[0], o[1]),
        lambda: eng.bm_compute_batch_device(i, i, 3, H * W, H, W, W - 1, bp, o[0]),
        lambda: eng.wls_filter_batch_device(m, m, i, 3, H * W, W - 1, H, W, wp, o[0]),
        lambda: eng.compute_disparity_batch_device(i, i, 3, H * W, H, W, W - 1, sp, wp, *o),
    ]
    for k, call in enumerate(device_calls):
        with pytest.raises(ValueError):
            call()
        assert b"stride" in eng._lib.sm_last_error(eng.ctx), k
    eng.synchronize()
    assert all(bool((t == S.SENTINEL).all()) for t in outs)
    a = np.zeros((H, 3 * W), np.uint8)
    d = np.zeros((H, W), np.int16)
    out = np.full((2, H, W), S.SENTINEL, np.int16)
    hp, dp, op = a.ctypes.data, d.ctypes.data, out.ctypes.data
    lib, ctx = eng._lib, eng.ctx
    host_calls = [
        lambda: lib.sm_compute_cn(ctx, hp, hp, H, W, 3 * W - 1, 3, ctypes.byref(sp), op),
        lambda: lib.sm_compute_cn(ctx, hp, hp, H, W, W - 1, 1, ctypes.byref(sp), op),
        lambda: lib.sm_compute(ctx, hp, hp, H, W, W - 1, ctypes.byref(sp), op, out[1].ctypes.data),
        lambda: lib.sm_bm_compute(ctx, hp, hp, H, W, W - 1, ctypes.byref(bp), op),
        lambda: lib.sm_wls_filter(ctx, dp, dp, hp, W - 1, H, W, ctypes.byref(wp), op),
        lambda: lib.sm_compute_disparity(ctx, hp, hp, H, W, W - 1, ctypes.byref(sp), ctypes.byref(wp), op,
                                         out[1].ctypes.data),
    ]
    for k, call in enumerate(host_calls):
        assert call() == _lib.SM_E_ARG, k
    assert (out == S.SENTINEL).all()
    p = S.sgbm_params(1, D, 8)
    a, b = S.pairs(H, W, D, 1)[0]
    assert np.array_equal(eng.compute(a, b, synthetic.to_sm_params(p)), S.expected(H, W, D, 1, S.key(p))[0])


# ---- the Python surface with non-packed inputs
PH, PW, PD = SHAPES[0]
VIEWS = ["torch_column_crop", "torch_channel_slice", "numpy_column_crop", "numpy_flipped", "numpy_fortran"]


def make_view(img, kind):
    """(view, base, snapshot of base): `view` holds img's values in a non-packed layout."""
    import torch

    H, W = img.shape
    rng = np.random.default_rng(H + W)
    if kind.endswith("column_crop"):
        base = rng.integers(0, 256, (H, W + 15)).astype(img.dtype)
        base[:, 5:5 + W] = img
        if kind.startswith("torch"):
            base = torch.tensor(base, device="cuda")
        view = base[:, 5:5 + W]
    elif kind == "torch_channel_slice":
        base = rng.integers(0, 256, (H, W, 3)).astype(img.dtype)
        base[:, :, 1] = img
        base = torch.tensor(base, device="cuda")
        view = base[:, :, 1]
    elif kind == "numpy_flipped":
        base = np.ascontiguousarray(img[::-1])
        view = base[::-1]
    else:
        base = np.asfortranarray(img)
        view = base
    if kind.startswith("torch"):
        assert not view.is_contiguous()
        snap = base.clone()
    else:
        assert not view.flags.c_contiguous
        assert np.array_equal(np.ascontiguousarray(view), img)
        snap = base.copy()
    return view, base, snap


def same(base, snap):
    return bool((base == snap).all())


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


@pytest.mark.parametrize("kind", VIEWS)
@pytest.mark.parametrize("cost,mode", [(1, 8), (0, 5)])
def test_stereo_sgbm_compute_views(kind, cost, mode):
    import stereo_match_amd as sm

    p = S.sgbm_params(cost, PD, mode)
    a, b = S.pairs(PH, PW, PD, 1)[0]
    m = sm.StereoSGBM_create(minDisparity=0, numDisparities=PD, blockSize=p["blockSize"], P1=p["P1"], P2=p["P2"],
                             disp12MaxDiff=p["disp12MaxDiff"], preFilterCap=p["preFilterCap"],
                             uniquenessRatio=p["uniquenessRatio"], speckleWindowSize=0, speckleRange=p["speckleRange"],
                             mode=sm.STEREO_SGBM_MODE_HH if mode == 8 else sm.STEREO_SGBM_MODE_SGBM,
                             cost="census" if cost else "sgbm")
    (va, ba, sa), (vb, bb, sb) = make_view(a, kind), make_view(b, kind)
    out = host(m.compute(va, vb))
    assert np.array_equal(out, S.expected(PH, PW, PD, 1, S.key(p))[0])
    assert same(ba, sa) and same(bb, sb), "the caller's image changed"


@pytest.mark.parametrize("kind", VIEWS)
def test_stereo_bm_compute_views(kind):
    import stereo_match_amd as sm

    p = dict(numDisparities=PD, blockSize=9)
    a, b = S.pairs(PH, PW, PD, 1)[0]
    (va, ba, sa), (vb, bb, sb) = make_view(a, kind), make_view(b, kind)
    out = host(sm.StereoBM_create(numDisparities=PD, blockSize=9).compute(va, vb))
    assert np.array_equal(out, S.expected_bm(PH, PW, PD, 1, S.key(p))[0])
    assert same(ba, sa) and same(bb, sb)


@pytest.mark.parametrize("kind", VIEWS)
def test_wls_filter_object_views(kind):
    import stereo_match_amd as sm
    from stereo_match_amd import wls

    settings = synthetic.parity_params(PD)
    _, wd = S.default_wls(settings, 8000.0, 1.5)
    dl, dr = S.lr_maps(PH, PW, PD, 1, S.key(settings))
    exp = S.expected_wls(PH, PW, PD, 1, S.key(settings), S.key(wd))[0]
    m = sm.StereoSGBM_create(numDisparities=PD, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
                             preFilterCap=63)
    f = wls.createDisparityWLSFilter(m)
    f.setLambda(8000.0)
    f.setSigmaColor(1.5)
    g = make_view(S.pairs(PH, PW, PD, 1)[0][0], kind)
    l, r = make_view(dl[0], kind), make_view(dr[0], kind)
    out = host(f.filter(l[0], g[0], None, r[0]))
    assert np.array_equal(out, exp), f"{int((out != exp).sum())} px differ"
    assert all(same(v[1], v[2]) for v in (g, l, r))


@pytest.mark.parametrize("kind", VIEWS)
def test_compute_disparity_views(kind):
    import stereo_match_amd as sm

    s = dict(sm.DEFAULT_SETTINGS, window_size=5, num_disparities=PD, lmbda=8000, sigma=1.5)
    settings = dict(synthetic.parity_params(PD), blockSize=s["block_size"], minDisparity=s["min_disparity"],
                    preFilterCap=s["pre_filter_cap"], speckleRange=s["speckle_range"],
                    uniquenessRatio=s["uniqueness_ratio"], disp12MaxDiff=s["disp12_max_diff"],
                    speckleWindowSize=s["speckle_window_size"])
    _, wd = S.default_wls(settings, 8000.0, 1.5)
    dl, _ = S.lr_maps(PH, PW, PD, 1, S.key(settings))
    ef = S.expected_wls(PH, PW, PD, 1, S.key(settings), S.key(wd))[0]
    a, b = S.pairs(PH, PW, PD, 1)[0]
    (va, ba, sa), (vb, bb, sb) = make_view(a, kind), make_view(b, kind)
    d, f = sm.compute_disparity(va, vb, s)
    assert np.array_equal(host(d), dl[0]) and np.array_equal(host(f), ef)
    assert same(ba, sa) and same(bb, sb)


def test_compute_fills_a_strided_disparity_view():
    import stereo_match_amd as sm

    a, b = S.pairs(PH, PW, PD, 1)[0]
    p = synthetic.parity_params(PD)
    m = sm.StereoSGBM_create(numDisparities=PD, blockSize=5, P1=p["P1"], P2=p["P2"], disp12MaxDiff=1,
                             uniquenessRatio=15, preFilterCap=63, speckleRange=2)
    for matcher, exp in ((m, S.expected(PH, PW, PD, 1, S.key(p))[0]),
                         (sm.StereoBM_create(PD, 9),
                          S.expected_bm(PH, PW, PD, 1, S.key(dict(numDisparities=PD, blockSize=9)))[0])):
        buf = np.full((PH + 2, PW + 9), S.SENTINEL, np.int16)
        view = buf[1:PH + 1, 3:3 + PW]
        ret = matcher.compute(a, b, disparity=view)
        assert ret is view and np.array_equal(view, exp)
        buf[1:PH + 1, 3:3 + PW] = S.SENTINEL
        assert (buf == S.SENTINEL).all(), "compute wrote outside the view"


def test_filter_speckles_on_a_strided_view():
    import torch

    import stereo_match_amd as sm

    p = synthetic.parity_params(PD)
    disp = S.expected(PH, PW, PD, 1, S.key(p))[0]
    exp = sgm_np.filter_speckles(disp, -16, 40, 32)
    assert (np.asarray(exp) != disp).any(), "the filter removes something here"
    buf = np.full((PH + 2, PW + 9), S.SENTINEL, np.int16)
    view = buf[1:PH + 1, 3:3 + PW]
    view[...] = disp
    ret, _ = sm.filterSpeckles(view, -16, 40, 32)
    assert ret is view and np.array_equal(view, exp)
    buf[1:PH + 1, 3:3 + PW] = S.SENTINEL
    assert (buf == S.SENTINEL).all()
    t = torch.tensor(np.ascontiguousarray(buf), device="cuda")
    with pytest.raises(ValueError):
        sm.filterSpeckles(t[1:PH + 1, 3:3 + PW], -16, 40, 32)
    assert bool((t == S.SENTINEL).all())
