"""gaussian_filter, image_measure and pyrDown on the CPU: the numpy
restatement tests/filters_np.py against scipy.ndimage itself, bit for bit, where scipy is
installed, and against the fixtures scipy produced (tests/golden/filters) everywhere; known
answers of the pyrDown restatement; the argument errors of the Python surface that need no
device.  The kernels are checked against the same restatement in tests/test_gpu_filters.py."""
import glob
import os

import numpy as np
import pytest

import filters_np
import stereo_match_amd as sma
from stereo_match_amd import filters

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filters")

SHAPES = [(1, 1), (3, 2), (7, 45), (20, 21), (37, 67), (130, 150)]
SIGMAS = [5, 3, 1.2, 0.4, (2, 0.7)]


def _golden_gauss():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "gauss_41x53_*.npz")))
    assert len(paths) == 4, "tests/golden/filters is incomplete (tests/golden/make_golden_filters.py)"
    return [np.load(p, allow_pickle=False) for p in paths]


# ---- against scipy itself

@pytest.mark.parametrize("sigma", SIGMAS, ids=str)
@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_equals_scipy(H, W, sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    a = filters_np.image_f64(H, W, seed=H * 1000 + W)
    exp = ndimage.gaussian_filter(a, sigma=sigma)
    assert np.array_equal(filters_np.gaussian_filter(a, sigma), exp)


def test_restated_image_measure_equals_the_scipy_expression():
    ndimage = pytest.importorskip("scipy.ndimage")
    bgr = filters_np.image_u8(45, 70, seed=8)
    img = filters_np.bgr2gray(bgr).astype(float)
    img = ndimage.gaussian_filter(img, sigma=5)
    blurred = ndimage.gaussian_filter(img, 3)
    assert np.array_equal(filters_np.image_measure(bgr), img + 30 * (img - blurred))


def test_fixture_weights_are_what_scipy_builds_today():
    pytest.importorskip("scipy")
    from scipy.ndimage import _filters

    for z in _golden_gauss():
        for ax in (0, 1):
            sd = float(z["sigma"][ax])
            assert np.array_equal(_filters._gaussian_kernel1d(sd, 0, int(4.0 * sd + 0.5))[::-1], z[f"w{ax}"])


# ---- against the fixtures scipy produced (no scipy needed)

def test_restatement_equals_the_fixtures():
    for z in _golden_gauss():
        s = tuple(z["sigma"])
        assert np.array_equal(filters_np.gaussian_filter(z["src"], s), z["out"]), s
    z = np.load(os.path.join(GOLDEN, "image_measure_37x67.npz"), allow_pickle=False)
    assert np.array_equal(filters_np.bgr2gray(z["bgr"]), z["gray"])
    out = filters_np.image_measure(z["bgr"])
    assert out.dtype == np.float64 and np.array_equal(out, z["out"])
    assert np.abs(z["out"] - z["gray"]).max() > 10  # not a degenerate image


@pytest.mark.parametrize("sigma", [5, 3, 1.2, 0.4, 2, 0.7, 15.8, 16, 0.1])
def test_gaussian_kernel1d(sigma):
    w, r = filters.gaussian_kernel1d(sigma)
    assert r == int(4 * sigma + 0.5) and w.shape == (2 * r + 1,) and w.dtype == np.float64
    ew, er = filters_np.kernel1d(sigma)
    assert er == r and np.array_equal(w, ew)
    assert np.array_equal(w, w[::-1]) and abs(w.sum() - 1) < 1e-15 and w.argmax() == r


def test_gaussian_kernel1d_equals_the_fixture_weights():
    for z in _golden_gauss():
        for ax in (0, 1):
            w, r = filters.gaussian_kernel1d(float(z["sigma"][ax]))
            assert np.array_equal(w, z[f"w{ax}"])
    # the radius cap: sigma 16 (sigma 15.8 stays one below it)
    assert filters.gaussian_kernel1d(15.8)[1] == filters.MAX_RADIUS - 1
    assert filters.gaussian_kernel1d(16)[1] == filters.MAX_RADIUS
    assert filters.gaussian_kernel1d(5, truncate=2.0)[1] == 10


def test_reflect_is_half_sample_symmetric():
    assert list(filters_np.refl(np.arange(-7, 10), 3)) == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2]
    assert list(filters_np.refl(np.arange(-3, 4), 1)) == [0] * 7


# ---- pyrDown restatement

@pytest.mark.parametrize("shape", [(9, 12), (9, 12, 3), (1, 1), (2, 2), (1, 7, 3), (6, 1)])
@pytest.mark.parametrize("value", [0, 1, 77, 255])
def test_pyr_down_constant(shape, value):
    out = filters_np.pyr_down(np.full(shape, value, np.uint8))
    assert out.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) + shape[2:]
    assert out.dtype == np.uint8 and np.all(out == value)


def test_pyr_down_scaled_impulse_gives_the_outer_product_of_k():
    """An impulse of 256 (the kernel's denominator; wider than uint8, so an int image) at an
    even position: the 3 x 3 outputs around it read it through the even taps (1, 6, 1)."""
    src = np.zeros((17, 21), np.int64)
    src[8, 10] = 256
    out = filters_np.pyr_down(src)
    exp = np.zeros((9, 11), np.int64)
    exp[3:6, 4:7] = np.outer([1, 6, 1], [1, 6, 1])
    assert np.array_equal(out, exp)
    # at an odd position the two outputs beside it read it through the taps (4, 4)
    src = np.zeros((17, 21), np.int64)
    src[9, 11] = 256
    exp = np.zeros((9, 11), np.int64)
    exp[4:6, 5:7] = 16
    assert np.array_equal(filters_np.pyr_down(src), exp)
    # every tap of k: the five source rows 2y-2 .. 2y+2 of output row y = 4, column x = 5
    k = np.array([1, 4, 6, 4, 1])
    for i in range(5):
        for j in range(5):
            src = np.zeros((17, 21), np.int64)
            src[6 + i, 8 + j] = 256
            assert filters_np.pyr_down(src)[4, 5] == k[i] * k[j]


def test_pyr_down_uint8_impulse():
    src = np.zeros((17, 21), np.uint8)
    src[8, 10] = 128
    out = filters_np.pyr_down(src)
    k = np.array([1, 4, 6, 4, 1])
    exp = np.zeros((9, 11), np.int64)
    # output (y, x) reads source rows 2y-2..2y+2: the impulse at row 8 has tap 8-2y+2 for y = 3, 4, 5
    for y in range(3, 6):
        for x in range(4, 7):
            exp[y, x] = (k[8 - 2 * y + 2] * k[10 - 2 * x + 2] * 128 + 128) >> 8
    assert np.array_equal(out, exp)
    assert out[4, 5] == 18 and out[3, 5] == (6 * 128 + 128) >> 8 and out[3, 4] == 1


def test_pyr_down_small_and_odd_sizes():
    a = np.array([[10, 200], [30, 90]], np.uint8)
    # 2x2: rows -2..2 reflect to 0,1,0,1,0 (k: 1+6+1 = 8 on row 0, 4+4 = 8 on row 1), columns alike
    assert filters_np.pyr_down(a)[0, 0] == (64 * (10 + 200 + 30 + 90) + 128) >> 8
    assert filters_np.pyr_down(np.array([[201]], np.uint8))[0, 0] == 201
    for H, W in [(3, 5), (37, 67), (64, 128), (130, 151)]:
        assert filters_np.pyr_down(filters_np.image_u8(H, W, 1, 1)).shape == ((H + 1) // 2, (W + 1) // 2)
    # an interior pixel by hand
    img = filters_np.image_u8(11, 13, 2, 1).astype(np.int64)
    k = np.array([1, 4, 6, 4, 1])
    assert filters_np.pyr_down(img.astype(np.uint8))[2, 3] == ((np.outer(k, k) * img[2:7, 4:9]).sum() + 128) >> 8


# ---- argument errors that need no device

def test_gaussian_filter_argument_errors():
    a = np.zeros((4, 5))
    bad = [
        (lambda: sma.gaussian_filter(a.astype(np.float32), 2), "float32"),
        (lambda: sma.gaussian_filter(a.astype(np.uint8), 2), "uint8"),
        (lambda: sma.gaussian_filter(a, 2, order=1), "order"),
        (lambda: sma.gaussian_filter(a, 2, mode="nearest"), "mode"),
        (lambda: sma.gaussian_filter(a, 2, radius=3), "radius"),
        (lambda: sma.gaussian_filter(np.zeros((2, 4, 5)), 2), "axes"),
        (lambda: sma.gaussian_filter(np.zeros((2, 4, 5)), 2, axes=(0, 1)), "axes"),
        (lambda: sma.gaussian_filter(a, 2, axes=(1,)), "axes"),
        (lambda: sma.gaussian_filter(np.zeros(5), 2), "1-D"),
        (lambda: sma.gaussian_filter(a, (1, 2, 3)), "sigma"),
        (lambda: sma.gaussian_filter(a, 2, output=np.float32), "float32"),
        (lambda: sma.gaussian_filter(a, 2, output=np.zeros((4, 6))), "output"),
    ]
    for call, word in bad:
        with pytest.raises(ValueError, match=word):
            call()


def test_image_measure_and_pyr_down_argument_errors():
    with pytest.raises(ValueError, match="uint8"):
        sma.image_measure(np.zeros((4, 5, 3), np.float64))
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        sma.image_measure(np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        sma.pyrDown(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="shape"):
        sma.pyrDown(np.zeros((4, 5, 2), np.uint8))
    with pytest.raises(ValueError, match="dstsize"):
        sma.pyrDown(np.zeros((4, 6), np.uint8), dstsize=(2, 2))
    with pytest.raises(ValueError, match="borderType"):
        sma.pyrDown(np.zeros((4, 6), np.uint8), borderType=0)
