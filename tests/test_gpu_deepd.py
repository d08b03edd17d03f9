"""GPU: numDisparities 272..512 (sm_deep.hpp) through every matcher entry point, bit-exact
against oracle/sgm_ref.c (ref_c) on the banded pairs of tests/deepd_cases.py, whose oracle maps
put 41 to 55 % of their valid pixels on planes >= 256 (tests/test_deepd_oracle.py).  Every
comparison is np.array_equal.  The new range runs on the per-direction engine alone, so the
in-sweep-lines and row-band counters must not move in any of these calls."""
import numpy as np
import pytest

import deepd_cases as C
import strided as S
from oracle import ref_c, sgm_np
from stereo_match_amd import _lib, matcher, synthetic, wls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


class NoSweeps:
    """The calls inside run neither the in-sweep lines nor the row bands nor a sweep fallback."""

    NAMES = ("line_groups", "band_groups", "sweep_fallbacks")

    def __init__(self, *engines):
        self.engines = engines

    def __enter__(self):
        self.c0 = [e.counters() for e in self.engines]
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            for e, c0 in zip(self.engines, self.c0):
                c1 = e.counters()
                for name in self.NAMES:
                    assert c1[name] == c0[name], f"{name} moved: the new range reached the fused sweeps"
        return False


def sgbm_matcher(p: dict):
    """StereoSGBM_create from an oracle-style dict (mode 5 / 8, cost 0 / 1 / 2)."""
    kw = {k: v for k, v in p.items() if k not in ("cost", "mode")}
    mode = matcher.STEREO_SGBM_MODE_HH if p["mode"] == 8 else matcher.STEREO_SGBM_MODE_SGBM
    return matcher.StereoSGBM_create(**kw, mode=mode, cost="census" if p.get("cost") == 1 else "sgbm")


def same(got, exp, what):
    assert np.array_equal(got, exp), f"{what}: {int((np.asarray(got) != exp).sum())} of {exp.size} px differ"


# ---- parity: the 24 image cases (disparity map and integer WTA index), the 3 volume cases
@pytest.mark.parametrize("D,minD,kind", C.IMAGE_CASES, ids=[f"D{d}_minD{m}_{k}" for d, m, k in C.IMAGE_CASES])
def test_parity_wta(eng, D, minD, kind):
    a, b = C.image_pair(D, minD)
    exp_d, exp_w = C.expected_wta(D, minD, kind)
    with NoSweeps(eng):
        got_d, got_w = eng.compute_wta(a, b, synthetic.to_sm_params(C.params(kind, D, minD)))
    same(got_w, exp_w, "WTA index")
    same(got_d, exp_d, "disparity")


@pytest.mark.parametrize("Dv,shifts", C.VOLUME_CASES, ids=[f"Dv{d}" for d, _ in C.VOLUME_CASES])
def test_parity_volume(eng, Dv, shifts):
    vol = C.volume(Dv, shifts)
    exp = C.expected_volume(Dv, shifts)
    p = C.volume_params(Dv)
    with NoSweeps(eng, _lib.engine(0)):
        got = eng.aggregate_cost_f32(vol, synthetic.to_sm_params(p), C.VOL_OFFSET, C.VOL_SCALE)
        got2 = sgbm_matcher(p).computeFromCost(vol, C.VOL_OFFSET, C.VOL_SCALE)
    same(got, exp, "aggregate_cost_f32")
    same(got2, exp, "computeFromCost")


def test_parity_volume_five_paths(eng):
    """MODE_SGBM over a volume (the lane8 tie-break's 6-bit rank)."""
    Dv, shifts = C.VOLUME_CASES[1]
    p = dict(C.volume_params(Dv), mode=5)
    exp = ref_c.compute_volume(C.volume(Dv, shifts), p, C.VOL_OFFSET, C.VOL_SCALE)
    with NoSweeps(eng):
        got = eng.aggregate_cost_f32(C.volume(Dv, shifts), synthetic.to_sm_params(p), C.VOL_OFFSET, C.VOL_SCALE)
    same(got, exp, "aggregate_cost_f32, 5 paths")


# ---- the speckle filter inside the matcher
@pytest.mark.parametrize("kind,ws,removes", [("census8", 50, False), ("sgbm5", 100, True)])
def test_speckle(eng, kind, ws, removes):
    """speckleWindowSize 50 / speckleRange 2 on the census map (whose regions are all larger: the
    filter runs and keeps them), and a window of 100 on the sgbm5 map, where the oracle's filter
    removes 166 pixels."""
    extra = (("speckleRange", 2), ("speckleWindowSize", ws))
    a, b = C.image_pair(320, 0)
    exp = C.expected(320, 0, kind, extra=extra)
    assert removes == (not np.array_equal(exp, C.expected(320, 0, kind)))
    with NoSweeps(eng):
        got = eng.compute(a, b, synthetic.to_sm_params(C.params(kind, 320, 0, **dict(extra))))
    same(got, exp, "speckle-filtered map")


# ---- batches: host pointers (sm_compute_batch) and torch tensors on a non-default stream
@pytest.mark.parametrize("D,kind", [(320, "census8"), (272, "sgbm5")])
def test_batches(eng, D, kind):
    import torch

    seeds = (5, 6, 7)
    pairs = [C.image_pair(D, 0, s) for s in seeds]
    exp = [C.expected(D, 0, kind, s) for s in seeds]
    sp = synthetic.to_sm_params(C.params(kind, D, 0))
    H, W = pairs[0][0].shape
    with NoSweeps(eng):
        got = _lib.compute_batch([eng], [a for a, _ in pairs], [b for _, b in pairs], sp)
    for i in range(3):
        same(got[i], exp[i], f"sm_compute_batch pair {i}")
    stream = torch.cuda.Stream()
    with NoSweeps(eng), torch.cuda.stream(stream):
        tl = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
        tr = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
        out = torch.full((3, H, W), S.SENTINEL, dtype=torch.int16, device="cuda")
        eng.set_stream(stream.cuda_stream)
        try:
            eng.compute_batch_device(tl.data_ptr(), tr.data_ptr(), 3, H * W, H, W, W, sp, out.data_ptr())
            stream.synchronize()
        finally:
            eng.set_stream(None)
        got = out.cpu().numpy()
    for i in range(3):
        same(got[i], exp[i], f"compute_batch_device pair {i}")


def test_matcher_surface_numpy_and_torch():
    """StereoSGBM_create(...).compute on numpy arrays and on torch CUDA tensors."""
    import torch

    D, kind = 288, "sgbm8"
    a, b = C.image_pair(D, -7)
    exp = C.expected(D, -7, kind)
    p = C.params(kind, D, -7)
    m = sgbm_matcher(p)
    with NoSweeps(_lib.engine(0)):
        same(m.compute(a, b), exp, "numpy")
        got = m.compute(torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda"))
        torch.cuda.synchronize()
        same(got.cpu().numpy(), exp, "torch")


# ---- the right matcher (minDisparity down to -(D - 1)) and the full call
def test_right_matcher():
    D, kind = 272, "sgbm5"
    a, b = C.image_pair(D, 0)
    p = C.params(kind, D, 0)
    left = sgbm_matcher(p)
    right = matcher.createRightMatcher(left)
    assert right.getMinDisparity() == -271
    exp = ref_c.compute(b, a, sgm_np.right_matcher_params(p))
    assert (exp >= -271 * 16).mean() >= C.MIN_VALID, "the oracle's right map is nearly empty"
    with NoSweeps(_lib.engine(0)):
        same(right.compute(b, a), exp, "right matcher")


@pytest.mark.parametrize("D,kind", [(272, "sgbm5"), (320, "census8")])
def test_compute_disparity(eng, D, kind):
    """sm_compute_disparity on one pair and sm_compute_disparity_batch_device on two, composed as
    tests/test_gpu_strides.py::test_compute_disparity_batch_device composes its expectation."""
    import torch

    seeds = (5, 6)
    settings = C.params(kind, D, 0)
    wp, wd = S.default_wls(settings)
    dl, dr = C.lr_maps(D, 0, kind, seeds)
    ef = C.expected_wls(D, 0, kind, seeds, S.key(wd))
    pairs = [C.image_pair(D, 0, s) for s in seeds]
    H, W = pairs[0][0].shape
    sp = synthetic.to_sm_params(settings)
    with NoSweeps(eng):
        gl, gf = eng.compute_disparity(pairs[0][0], pairs[0][1], sp, wp)
    same(gl, dl[0], "displ, one pair")
    same(gf, ef[0], "filtered, one pair")
    tl = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
    tr = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
    outs = [torch.full((2, H, W), S.SENTINEL, dtype=torch.int16, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    with NoSweeps(eng):
        eng.compute_disparity_batch_device(tl.data_ptr(), tr.data_ptr(), 2, H * W, H, W, W, sp, wp,
                                           *(o.data_ptr() for o in outs))
        eng.synchronize()
    gl, gr, gf = (o.cpu().numpy() for o in outs)
    for i in range(2):
        same(gl[i], dl[i], f"displ pair {i}")
        same(gr[i], dr[i], f"dispr pair {i}")
        same(gf[i], ef[i], f"filtered pair {i}")


def test_python_compute_disparity_and_wls_factory():
    """stereo_vision.compute_disparity and createDisparityWLSFilter(left) at D = 272."""
    from stereo_match_amd import stereo_vision

    D, kind = 272, "sgbm5"
    settings = C.params(kind, D, 0)
    a, b = C.image_pair(D, 0)
    left = sgbm_matcher(settings)
    f = wls.createDisparityWLSFilter(left)
    assert left.getDisp12MaxDiff() == 1000000 and left.getUniquenessRatio() == 0 and f.left_offset == D
    _, wd = S.default_wls(settings)
    dl, _ = C.lr_maps(D, 0, kind, (5,))
    ef = C.expected_wls(D, 0, kind, (5,), S.key(wd))
    ws = 5  # parity_params: P1 = 8 * 3 * ws^2, P2 = 32 * 3 * ws^2
    assert (settings["P1"], settings["P2"]) == (8 * 3 * ws * ws, 32 * 3 * ws * ws)
    ds = dict(min_disparity=0, num_disparities=D, block_size=settings["blockSize"], window_size=ws,
              disp12_max_diff=settings["disp12MaxDiff"], uniqueness_ratio=settings["uniquenessRatio"],
              speckle_window_size=0, speckle_range=settings["speckleRange"], pre_filter_cap=settings["preFilterCap"],
              lmbda=8000.0, sigma=1.5)
    with NoSweeps(_lib.engine(0)):
        displ, filt = stereo_vision.compute_disparity(a, b, ds)
    same(displ, dl[0], "displ")
    same(filt, ef[0], "filtered")


# ---- one context across the 256 boundary: its buffers grow and shrink
def test_context_reuse():
    e = _lib.Engine(0)
    try:
        for D in (128, 512, 64, 272):
            for kind in ("census8", "sgbm5"):
                a, b = C.image_pair(D, 0) if D > 256 else S.pairs(24, 229, D, 1)[0]
                p = C.params(kind, D, 0)
                exp = C.expected(D, 0, kind) if D > 256 else ref_c.compute(a, b, p)
                same(e.compute(a, b, synthetic.to_sm_params(p)), exp, f"D {D} {kind}")
    finally:
        e.close()


# ---- refusals: SM_E_UNSUPPORTED with the named reason, and the context still works
def _refused(eng, fn, *needles):
    with pytest.raises(_lib.SmError) as ei:
        fn()
    assert ei.value.code == _lib.SM_E_UNSUPPORTED
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)
    a, b = C.image_pair(272, 0)
    same(eng.compute(a, b, synthetic.to_sm_params(C.params("census8", 272, 0))), C.expected(272, 0, "census8"),
         "the call after the refusal")


def test_refuses_above_512(eng):
    a, b = C.image_pair(512, 0)
    for kind in ("census8", "sgbm5"):
        _refused(eng, lambda: eng.compute(a, b, synthetic.to_sm_params(C.params(kind, 528, 0))), "528", "> 512")
    vol = np.zeros((513, 4, 700), np.float32)
    _refused(eng, lambda: eng.aggregate_cost_f32(vol, synthetic.to_sm_params(C.volume_params(513))), "513", "> 512")


def test_refuses_bgr_above_256(eng):
    a, b = C.image_pair(272, 0)
    p = synthetic.to_sm_params(C.params("sgbm5", 272, 0))
    _refused(eng, lambda: eng.compute(S.bgr(a, 0), S.bgr(b, 0), p), "272", "> 256", "gray")


def test_refuses_large_blocks_above_256(eng):
    a, b = C.image_pair(272, 0)
    p = synthetic.to_sm_params(C.params("sgbm5", 272, 0, blockSize=13))
    _refused(eng, lambda: eng.compute(a, b, p), "272", "> 256", "blockSize")


def test_refuses_forced_sweeps_above_256(eng):
    a, b = C.image_pair(272, 0)

    def call():
        eng.set_debug_flags(16384)
        try:
            eng.compute(a, b, synthetic.to_sm_params(C.params("census8", 272, 0)))
        finally:
            eng.set_debug_flags(0)

    _refused(eng, call, "272", "> 256", "per-direction", "16384")
