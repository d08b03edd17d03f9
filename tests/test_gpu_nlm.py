"""GPU: fastNlMeansDenoising (sm_nlm.hpp k_nlm_u8; stereo_match_amd/denoise.py) against the
independent numpy restatement tests/nlm_np.py, bit for bit: images smaller than the border,
tile tails, strides, batches, every template size, the LDS and the global weight table, the
table itself, the numpy and torch surfaces, the denoise-then-match chain, argument errors."""
import functools
import os

import numpy as np
import pytest

import nlm_np
import stereo_match_amd as sma
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

DEFAULT = (10, 7, 21)
# every parameter set of the suite: (h, templateWindowSize, searchWindowSize)
PARAMS_37x67 = [(3, 7, 21), (30, 7, 21), (10, 5, 11), (10, 3, 5), (4, 8, 22), (10, 1, 1), (0, 7, 21), (200, 7, 21)]
ALL_PARAMS = [DEFAULT] + PARAMS_37x67 + [(10, 9, 35)]


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _image(H, W, seed=11):
    img = nlm_np.noisy_blobs(H, W, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _expected(H, W, prm, seed=11):
    """(out, wsum) of the restatement, computed once per case and left unchanged."""
    out, wsum = nlm_np.denoise(_image(H, W, seed), *prm)
    out.setflags(write=False)
    wsum.setflags(write=False)
    return out, wsum


def _fpm(prm):
    s = 2 * (prm[2] // 2) + 1
    return 2147483647 // (s * s * 255)


def _assert_regime(wsum, prm):
    """The input must not degenerate to the identity: most pixels average many offsets."""
    assert np.median(wsum) > 4 * _fpm(prm), f"median wsum {np.median(wsum)} <= 4 * fpm: a degenerate input"


# ---- shapes at the default parameters
# 1x1; 3x2 and 5x40 smaller than the border b = 13 (indices reflect several times); 37x67 and
# 45x130 with tile tails in both axes and W % 4 != 0; 130x150 spans three 64 x 64 tiles in
# each axis (the tile is larger than the 32 x 32 a 96x160 image would cover three times)

@pytest.mark.parametrize("H,W", [(1, 1), (3, 2), (5, 40), (37, 67), (45, 130), (130, 150)])
def test_shapes_default(eng, H, W):
    exp, wsum = _expected(H, W, DEFAULT)
    _assert_regime(wsum, DEFAULT)
    out = eng.nlm_denoise(_image(H, W), *DEFAULT)
    assert out.dtype == np.uint8 and out.shape == (H, W)
    assert np.array_equal(out, exp), f"{int((out != exp).sum())} px differ"
    if H * W > 100:
        assert (exp != _image(H, W)).mean() > 0.5


def test_golden_fixture(eng):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlm",
                             "nlm_h10_t7_s21_40x56.npz"), allow_pickle=False)
    out = eng.nlm_denoise(z["src"], *(int(v) for v in z["params"]))
    assert np.array_equal(out, z["out"])


# ---- parameters

@pytest.mark.parametrize("prm", PARAMS_37x67, ids=[str(p) for p in PARAMS_37x67])
def test_parameters_37x67(eng, prm):
    H, W = 37, 67
    exp, wsum = _expected(H, W, prm)
    if prm[0] >= 10 and prm[1] > 1:
        _assert_regime(wsum, prm)
    out = eng.nlm_denoise(_image(H, W), *prm)
    assert np.array_equal(out, exp), f"{int((out != exp).sum())} px differ at {prm}"
    if prm[0] == 0:
        assert np.array_equal(out, _image(H, W))  # only distance 0 has weight


def test_supported_maximum(eng):
    prm = (10, 9, 35)
    exp, wsum = _expected(20, 24, prm)
    _assert_regime(wsum, prm)
    out = eng.nlm_denoise(_image(20, 24), *prm)
    assert np.array_equal(out, exp)


def test_table_paths_are_the_ones_meant():
    """(30, 7, 21) is the long table that still fits in LDS, h = 200 the one that does not."""
    lds_max = 8192  # sm_nlm.hpp NLM_LDS_TAB_MAX
    assert 4096 < np.count_nonzero(nlm_np.weight_table(30, 7, 21)[0]) <= lds_max
    assert np.count_nonzero(nlm_np.weight_table(200, 7, 21)[0]) > lds_max


@pytest.mark.parametrize("prm", ALL_PARAMS, ids=[str(p) for p in ALL_PARAMS])
def test_weight_table(eng, prm):
    tab, fpm, shift = eng.nlm_weight_table(*prm)
    etab, efpm, eshift = nlm_np.weight_table(*prm)
    assert (fpm, shift, len(tab)) == (efpm, eshift, len(etab))
    assert tab.dtype == np.int32 and np.array_equal(tab, etab)


# ---- strides and batches

def test_strided_source(eng):
    H, W = 37, 67
    buf = np.full((H, W + 13), 255, np.uint8)
    buf[:, :W] = _image(H, W)
    view = buf[:, :W]
    assert view.strides[0] == W + 13
    out = eng.nlm_denoise(view, *DEFAULT)
    assert np.array_equal(out, _expected(H, W, DEFAULT)[0])


def test_batch_device_with_gap_and_stride(eng):
    """Three images, rows W + 5 bytes apart, images a row stride more than their size apart."""
    torch = pytest.importorskip("torch")
    H, W, stride = 37, 67, 72
    img_stride = H * stride + 99
    seeds = (11, 12, 13)
    buf = np.full(3 * img_stride, 255, np.uint8)
    for i, sd in enumerate(seeds):
        v = buf[i * img_stride:i * img_stride + H * stride].reshape(H, stride)
        v[:, :W] = _image(H, W, sd)
    d_src = torch.from_numpy(buf).cuda()
    d_dst = torch.zeros((3, H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.set_stream(None)
    eng.nlm_denoise_batch_device(d_src.data_ptr(), 3, img_stride, H, W, stride, *DEFAULT, d_dst.data_ptr())
    eng.synchronize()
    out = d_dst.cpu().numpy()
    for i, sd in enumerate(seeds):
        exp, wsum = _expected(H, W, DEFAULT, sd)
        _assert_regime(wsum, DEFAULT)
        assert np.array_equal(out[i], exp), f"image {i}"


# ---- public surface

def test_numpy_surface_and_dst(eng):
    H, W = 37, 67
    img = _image(H, W)
    exp = _expected(H, W, DEFAULT)[0]
    out = sma.fastNlMeansDenoising(img, None, 10, 7, 21)
    assert isinstance(out, np.ndarray) and np.array_equal(out, exp)
    dst = np.zeros((H, W), np.uint8)
    ret = sma.fastNlMeansDenoising(img, dst, 10, 7, 21)
    assert ret is dst and np.array_equal(dst, exp)
    # the cv2 defaults: h = 3, templateWindowSize = 7, searchWindowSize = 21
    assert np.array_equal(sma.fastNlMeansDenoising(img), _expected(H, W, (3, 7, 21))[0])


def test_torch_surface_on_a_side_stream(eng):
    torch = pytest.importorskip("torch")
    H, W = 37, 67
    seeds = (11, 12)
    host = np.stack([_image(H, W, sd) for sd in seeds])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        batch = torch.from_numpy(host).cuda()
        one = sma.fastNlMeansDenoising(batch[0], None, 10, 7, 21)
        both = sma.fastNlMeansDenoising(batch, None, 10, 7, 21)
    stream.synchronize()
    assert one.is_cuda and one.dtype == torch.uint8 and tuple(one.shape) == (H, W)
    assert tuple(both.shape) == (2, H, W)
    assert np.array_equal(one.cpu().numpy(), _expected(H, W, DEFAULT, seeds[0])[0])
    for i, sd in enumerate(seeds):
        assert np.array_equal(both[i].cpu().numpy(), _expected(H, W, DEFAULT, sd)[0])


def test_chain_denoise_then_match_on_the_device(eng):
    """disparity_test.py's order with the tensors kept on the device: cvtColor -> denoise ->
    block-23 SGBM equals the same matcher on the host-denoised images."""
    torch = pytest.importorskip("torch")
    H, W = 64, 96
    left, right, _ = synthetic.random_dot_pair(H, W, 16, seed=5)
    rng = np.random.default_rng(5)
    bgr = []
    for g in (left, right):
        # a smooth colour scene under the dots, so that the denoiser has something to average
        base = nlm_np.noisy_blobs(H, W, seed=21).astype(np.int32)
        img = np.stack([np.clip((g.astype(np.int32) + 3 * base) // 4 + rng.integers(-6, 7, (H, W)), 0, 255)
                        for _ in range(3)], axis=-1).astype(np.uint8)
        bgr.append(img)
    matcher = sma.StereoSGBM_create(numDisparities=16, blockSize=23, P1=222, P2=887, disp12MaxDiff=20,
                                    uniquenessRatio=0, preFilterCap=1)
    # the host flow
    gray = [sma.cvtColor(b, sma.COLOR_BGR2GRAY) for b in bgr]
    den = [sma.fastNlMeansDenoising(g, None, 10, 7, 21) for g in gray]
    for g, d in zip(gray, den):
        assert np.array_equal(d, nlm_np.denoise(g, 10, 7, 21)[0])
    assert (den[0] != gray[0]).mean() > 0.25
    exp = matcher.compute(den[0], den[1])
    # the device flow
    t = [torch.from_numpy(b).cuda() for b in bgr]
    tg = [sma.cvtColor(x, sma.COLOR_BGR2GRAY) for x in t]
    td = [sma.fastNlMeansDenoising(x, None, 10, 7, 21) for x in tg]
    disp = matcher.compute(td[0], td[1])
    assert disp.is_cuda
    assert np.array_equal(disp.cpu().numpy(), exp)


# ---- errors

def test_errors_leave_the_engine_usable(eng):
    H, W = 37, 67
    img = _image(H, W)
    exp = _expected(H, W, DEFAULT)[0]
    bad = [
        lambda: sma.fastNlMeansDenoising(np.zeros((8, 8, 3), np.uint8), None, 10, 7, 21),  # 3 channels
        lambda: sma.fastNlMeansDenoising(img.astype(np.float32), None, 10, 7, 21),          # float input
        lambda: sma.fastNlMeansDenoising(img, None, 10, 11, 21),                            # template 11
        lambda: sma.fastNlMeansDenoising(img, None, 10, 7, 37),                             # search 37
        lambda: sma.fastNlMeansDenoising(img, None, -1, 7, 21),                             # negative h
        lambda: sma.fastNlMeansDenoising(img, None, float("nan"), 7, 21),                   # NaN h
        lambda: sma.fastNlMeansDenoising(np.zeros((0, 8), np.uint8), None, 10, 7, 21),      # H = 0
        lambda: sma.fastNlMeansDenoising(img, np.zeros((H, W + 1), np.uint8), 10, 7, 21),   # wrong dst
    ]
    for i, call in enumerate(bad):
        with pytest.raises((ValueError, _lib.SmError)):
            call()
        assert np.array_equal(sma.fastNlMeansDenoising(img, None, 10, 7, 21), exp), f"after bad call {i}"
    # the message names what was asked for
    for tws, sws, asked in ((11, 21, "templateWindowSize 11"), (7, 37, "searchWindowSize 37")):
        with pytest.raises(_lib.SmError) as ei:
            sma.fastNlMeansDenoising(img, None, 10, tws, sws)
        assert ei.value.code == _lib.SM_E_UNSUPPORTED and asked in str(ei.value)


def test_stride_below_width_is_refused(eng):
    torch = pytest.importorskip("torch")
    H, W = 37, 67
    d_src = torch.from_numpy(_image(H, W).copy()).cuda()
    d_dst = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.set_stream(None)
    with pytest.raises(ValueError):
        eng.nlm_denoise_batch_device(d_src.data_ptr(), 1, 0, H, W, W - 1, *DEFAULT, d_dst.data_ptr())
    eng.nlm_denoise_batch_device(d_src.data_ptr(), 1, 0, H, W, W, *DEFAULT, d_dst.data_ptr())
    eng.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), _expected(H, W, DEFAULT)[0])
