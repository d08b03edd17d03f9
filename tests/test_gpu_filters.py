"""GPU: gaussian_filter, image_measure and pyrDown (sm_filter.hpp; stereo_match_amd/filters.py)
against the independent numpy restatement tests/filters_np.py and the fixtures scipy produced
(tests/golden/filters), bit for bit: images smaller than the radius, lengths r and r + 1, tile
tails, three tiles per axis, the radius cap, strides, batches, the numpy and torch surfaces, the
pyrDown-then-match chain, argument errors."""
import functools
import glob
import os

import numpy as np
import pytest

import filters_np
import stereo_match_amd as sma
from stereo_match_amd import _lib, filters, synthetic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filters")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _f64(H, W, seed=5):
    a = filters_np.image_f64(H, W, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _gauss_expected(H, W, sigma, seed=5):
    out = filters_np.gaussian_filter(_f64(H, W, seed), sigma)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _u8(H, W, channels, seed=6):
    a = filters_np.image_u8(H, W, seed, channels)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _measure_expected(H, W, seed=6):
    out = filters_np.image_measure(_u8(H, W, 3, seed))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _pyr_expected(H, W, channels, seed=6):
    out = filters_np.pyr_down(_u8(H, W, channels, seed))
    out.setflags(write=False)
    return out


def _same(a, b):
    """Bit equality of float64 arrays (NaN-free here, so == is bit equality up to the sign of 0)."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- Gaussian: shapes
# 1x1; 3x2 far smaller than r = 20 (indices reflect several times); 20x21 and 21x20 (a length
# equal to r and to r + 1 on either axis, at sigma 5); 37x67 with tile tails on both axes and
# W % 4 != 0; 130x150 spans three 64 x 32 tiles on each axis

@pytest.mark.parametrize("sigma", [5, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 2), (20, 21), (21, 20), (37, 67), (130, 150)])
def test_gauss_shapes(H, W, sigma):
    out = sma.gaussian_filter(_f64(H, W), sigma)
    exp = _gauss_expected(H, W, sigma)
    assert out.dtype == np.float64 and out.shape == (H, W)
    assert np.array_equal(out, exp), f"{int((out != exp).sum())} px differ"


def test_gauss_sigma_then_sigma():
    """image_measure's chain on a float64 image: sigma 5, then 3 on that result."""
    a = sma.gaussian_filter(_f64(37, 67), 5)
    b = sma.gaussian_filter(a, 3)
    assert np.array_equal(b, filters_np.gaussian_filter(_gauss_expected(37, 67, 5), 3))


def test_gauss_no_contraction():
    """Values around +-1e3 with sign changes: a fused multiply-add in either pass changes the
    last bit of a large share of the outputs."""
    src = _f64(37, 67)
    assert (src > 0).mean() > 0.3 and (src < 0).mean() > 0.3 and np.abs(src).max() > 1e3
    out = sma.gaussian_filter(src, 5)
    assert (out != src).mean() > 0.5
    assert np.array_equal(out, _gauss_expected(37, 67, 5))


@pytest.mark.parametrize("sigma", [(2, 0.7), (0.1, 3), (3, 0.1), 15.8, 16], ids=str)
def test_gauss_sigma_pairs_identity_axis_and_the_cap(sigma):
    """(0.1, 3) and (3, 0.1): r = 0, the identity, on one axis; 15.8: r = 63 (above 64 KiB of
    LDS); 16: r = 64, the cap."""
    out = sma.gaussian_filter(_f64(37, 67), sigma)
    assert np.array_equal(out, _gauss_expected(37, 67, sigma))
    assert (out != _f64(37, 67)).mean() > 0.5


def test_gauss_beyond_the_cap(eng):
    assert filters.gaussian_kernel1d(16.2)[1] == 65
    with pytest.raises(_lib.SmError) as ei:
        sma.gaussian_filter(_f64(37, 67), 16.2)
    assert ei.value.code == _lib.SM_E_UNSUPPORTED and "radius 65" in str(ei.value)
    with pytest.raises(_lib.SmError):
        sma.gaussian_filter(_f64(37, 67), (1, 16.2))
    # the engine is usable afterwards
    assert np.array_equal(sma.gaussian_filter(_f64(37, 67), 5), _gauss_expected(37, 67, 5))


def test_gauss_golden_fixtures():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "gauss_41x53_*.npz")))
    assert len(paths) == 4
    for p in paths:
        z = np.load(p, allow_pickle=False)
        out = sma.gaussian_filter(z["src"], tuple(z["sigma"]))
        assert _same(out, z["out"]), os.path.basename(p)
        assert (out != z["src"]).mean() > 0.5


def test_gauss_strided_numpy_view_and_output():
    H, W = 37, 67
    buf = np.full((H, W + 13), np.nan)
    buf[:, :W] = _f64(H, W)
    view = buf[:, :W]
    assert view.strides[0] == 8 * (W + 13)
    exp = _gauss_expected(H, W, 5)
    assert np.array_equal(sma.gaussian_filter(view, 5), exp)
    dst = np.zeros((H, W + 3))
    ret = sma.gaussian_filter(view, 5, output=dst[:, :W])
    assert np.array_equal(ret, exp) and np.array_equal(dst[:, :W], exp) and not dst[:, W:].any()
    assert np.array_equal(sma.gaussian_filter(view, 5, output=np.float64), exp)


def test_gauss_device_strides_larger_than_the_width(eng):
    """Three images; source rows W + 5 doubles apart and images a gap apart, destination rows
    W + 3 apart: nothing outside the destination pixels is written."""
    torch = pytest.importorskip("torch")
    H, W, ss, ds = 37, 67, 72, 70
    simg, dimg = H * ss + 11, H * ds + 7
    seeds = (5, 6, 7)
    buf = np.full(3 * simg, np.nan)
    for i, sd in enumerate(seeds):
        buf[i * simg:i * simg + H * ss].reshape(H, ss)[:, :W] = _f64(H, W, sd)
    d_src = torch.from_numpy(buf).cuda()
    d_dst = torch.full((3 * dimg,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.set_stream(None)
    wy = filters.gaussian_kernel1d(5)[0][20:]
    wx = filters.gaussian_kernel1d(3)[0][12:]
    eng.gauss2d_batch_device(d_src.data_ptr(), 3, simg, H, W, ss, wy, wx, d_dst.data_ptr(), dimg, ds)
    eng.synchronize()
    out = d_dst.cpu().numpy()
    for i, sd in enumerate(seeds):
        img = out[i * dimg:i * dimg + H * ds].reshape(H, ds)
        assert np.array_equal(img[:, :W], _gauss_expected(H, W, (5, 3), sd)), f"image {i}"
        assert np.all(img[:, W:] == -7.0)
        assert np.all(out[i * dimg + H * ds:(i + 1) * dimg] == -7.0)


def test_gauss_batch_equals_single_calls():
    torch = pytest.importorskip("torch")
    H, W = 37, 67
    batch = np.stack([_f64(H, W, sd) for sd in (5, 6, 7)])
    singles = np.stack([sma.gaussian_filter(batch[i], 5) for i in range(3)])
    for i, sd in enumerate((5, 6, 7)):
        assert np.array_equal(singles[i], _gauss_expected(H, W, 5, sd))
    assert np.array_equal(sma.gaussian_filter(batch, 5, axes=(1, 2)), singles)
    assert np.array_equal(sma.gaussian_filter(batch, 5, axes=(-2, -1)), singles)
    t = torch.from_numpy(batch).cuda()
    out = sma.gaussian_filter(t, 5, axes=(1, 2))
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (3, H, W)
    assert np.array_equal(out.cpu().numpy(), singles)
    one = sma.gaussian_filter(t[1], 5)
    assert np.array_equal(one.cpu().numpy(), singles[1])
    # a non-contiguous batch: every second image of a larger one
    t2 = torch.from_numpy(np.repeat(batch, 2, axis=0)).cuda()[::2]
    assert not t2.is_contiguous()
    assert np.array_equal(sma.gaussian_filter(t2, 5, axes=(1, 2)).cpu().numpy(), singles)
    dst = torch.zeros_like(t)
    assert sma.gaussian_filter(t, 5, output=dst, axes=(1, 2)) is dst
    assert np.array_equal(dst.cpu().numpy(), singles)


# ---- image_measure

def test_image_measure_golden():
    z = np.load(os.path.join(GOLDEN, "image_measure_37x67.npz"), allow_pickle=False)
    out = sma.image_measure(z["bgr"])
    assert out.dtype == np.float64 and _same(out, z["out"])
    assert _same(sma.image_measure(z["bgr"], True), z["out"])  # test_mode is ignored


# 5x40: smaller than both radii on axis 0; 130x150: three tiles on each axis
@pytest.mark.parametrize("H,W", [(5, 40), (37, 67), (130, 150)])
def test_image_measure_shapes(H, W):
    out = sma.image_measure(_u8(H, W, 3))
    exp = _measure_expected(H, W)
    assert out.dtype == np.float64 and out.shape == (H, W)
    assert np.array_equal(out, exp), f"{int((out != exp).sum())} px differ"


def test_image_measure_gray_stage_is_cvtcolor():
    """The fused gray conversion gives cvtColor's bytes: the filters on cvtColor's output and
    the expression evaluated by numpy give image_measure's bits."""
    bgr = _u8(37, 67, 3)
    gray = sma.cvtColor(bgr, sma.COLOR_BGR2GRAY)
    assert np.array_equal(gray, filters_np.bgr2gray(bgr))
    a = sma.gaussian_filter(gray.astype(np.float64), 5)
    b = sma.gaussian_filter(a, 3)
    assert np.array_equal(sma.image_measure(bgr), a + 30 * (a - b))


def test_image_measure_torch_batch_and_surfaces():
    torch = pytest.importorskip("torch")
    H, W = 37, 67
    seeds = (6, 7, 8)
    host = np.stack([_u8(H, W, 3, sd) for sd in seeds])
    t = torch.from_numpy(host).cuda()
    out = sma.image_measure(t)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (3, H, W)
    one = sma.image_measure(t[0])
    assert tuple(one.shape) == (H, W)
    for i, sd in enumerate(seeds):
        assert np.array_equal(out[i].cpu().numpy(), _measure_expected(H, W, sd)), f"image {i}"
    # numpy and torch surfaces: the same bits
    assert np.array_equal(one.cpu().numpy().view(np.uint64), sma.image_measure(host[0]).view(np.uint64))


# ---- pyrDown
# 1x1 and 2x2 (every tap reflected); 3x5; 37x67 (odd sizes, scalar stores: 34 bytes per row);
# 64x128 (rows of 64 / 192 bytes: the aligned dword path); 130x151 (rows of 76 / 228 bytes,
# dword stores with an odd source width); more than one block per row: the wide case below

@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (37, 67), (64, 128), (130, 151)])
def test_pyr_down_shapes(H, W, channels):
    src = _u8(H, W, channels)
    out = sma.pyrDown(src)
    exp = _pyr_expected(H, W, channels)
    assert out.dtype == np.uint8 and out.shape == exp.shape
    assert np.array_equal(out, exp), f"{int((out != exp).sum())} values differ"


def test_pyr_down_two_blocks_per_row():
    """A destination row of 1030 x 3 bytes needs more than one 256-lane block (1024 bytes)."""
    out = sma.pyrDown(_u8(4, 2059, 3))
    assert np.array_equal(out, _pyr_expected(4, 2059, 3))


def test_pyr_down_extremes_and_dst():
    assert np.all(sma.pyrDown(np.full((9, 14, 3), 255, np.uint8)) == 255)
    assert not sma.pyrDown(np.zeros((9, 14), np.uint8)).any()
    src = _u8(37, 67, 3)
    dst = np.zeros((19, 34, 3), np.uint8)
    assert sma.pyrDown(src, dst) is dst and np.array_equal(dst, _pyr_expected(37, 67, 3))
    assert np.array_equal(sma.pyrDown(src, dstsize=(34, 19), borderType=filters.BORDER_DEFAULT), dst)
    # a strided numpy view
    buf = np.full((37, 67 + 9, 3), 255, np.uint8)
    buf[:, :67] = src
    assert np.array_equal(sma.pyrDown(buf[:, :67]), dst)


@pytest.mark.parametrize("channels,ds", [(1, 36), (1, 35), (3, 104), (3, 103)])
def test_pyr_down_device_strides(eng, channels, ds):
    """Two images; source rows 7 bytes longer than the image's, destination rows ``ds`` bytes
    apart: a multiple of 4 (dword stores) and not (byte stores).  Nothing else is written."""
    torch = pytest.importorskip("torch")
    H, W = 37, 67
    dH, dW = 19, 34
    ss = W * channels + 7
    simg, dimg = H * ss + 5, dH * ds + (4 if ds % 4 == 0 else 3)
    seeds = (6, 7)
    buf = np.full(2 * simg, 255, np.uint8)
    for i, sd in enumerate(seeds):
        buf[i * simg:i * simg + H * ss].reshape(H, ss)[:, :W * channels] = _u8(H, W, channels, sd).reshape(H, -1)
    d_src = torch.from_numpy(buf).cuda()
    d_dst = torch.full((2 * dimg,), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.set_stream(None)
    eng.pyr_down_batch_device(d_src.data_ptr(), 2, simg, H, W, ss, channels, d_dst.data_ptr(), dimg, ds)
    eng.synchronize()
    out = d_dst.cpu().numpy()
    for i, sd in enumerate(seeds):
        img = out[i * dimg:i * dimg + dH * ds].reshape(dH, ds)
        assert np.array_equal(img[:, :dW * channels], _pyr_expected(H, W, channels, sd).reshape(dH, -1)), f"image {i}"
        assert np.all(img[:, dW * channels:] == 99)
        assert np.all(out[i * dimg + dH * ds:(i + 1) * dimg] == 99)


def test_pyr_down_torch_batch():
    torch = pytest.importorskip("torch")
    H, W = 37, 67
    for channels in (1, 3):
        host = np.stack([_u8(H, W, channels, sd) for sd in (6, 7, 8)])
        out = sma.pyrDown(torch.from_numpy(host).cuda())
        assert out.is_cuda and out.dtype == torch.uint8
        assert tuple(out.shape) == (3, 19, 34) + ((3,) if channels == 3 else ())
        for i, sd in enumerate((6, 7, 8)):
            assert np.array_equal(out[i].cpu().numpy(), _pyr_expected(H, W, channels, sd))
        one = sma.pyrDown(torch.from_numpy(host[1]).cuda())
        assert np.array_equal(one.cpu().numpy(), _pyr_expected(H, W, channels, 7))


@pytest.mark.parametrize("channels", [1, 3])
def test_pyr_down_then_match_on_the_device(channels):
    """try_try.py's order with the tensors kept on the device: pyrDown of both frames, then the
    matcher, equals the same matcher on the host-downsampled pair."""
    torch = pytest.importorskip("torch")
    left, right, _ = synthetic.random_dot_pair(96, 160, 16, seed=9)
    if channels == 3:
        left, right = (np.stack([g, g // 2 + 40, 255 - g], axis=-1) for g in (left, right))
    matcher = sma.StereoSGBM_create(numDisparities=16)
    small = [sma.pyrDown(g) for g in (left, right)]
    for s, g in zip(small, (left, right)):
        assert np.array_equal(s, filters_np.pyr_down(g))
    exp = matcher.compute(small[0], small[1])
    assert (exp >= 0).any() and len(np.unique(exp)) > 4  # not a map of one value
    t = [sma.pyrDown(torch.from_numpy(np.ascontiguousarray(g)).cuda()) for g in (left, right)]
    disp = matcher.compute(t[0], t[1])
    assert disp.is_cuda
    assert np.array_equal(disp.cpu().numpy(), exp)


# ---- errors

def test_argument_errors_leave_the_engine_usable(eng):
    torch = pytest.importorskip("torch")
    bad = [
        lambda: sma.gaussian_filter(np.zeros((0, 8)), 2),                             # H = 0
        lambda: sma.gaussian_filter(np.zeros((8, 0)), 2),                             # W = 0
        lambda: sma.gaussian_filter(np.zeros((8, 8), np.float32), 2),                 # dtype
        lambda: sma.gaussian_filter(torch.zeros((8, 8), device="cuda"), 2),           # float32 tensor
        lambda: sma.gaussian_filter(torch.zeros((8, 8), dtype=torch.float64), 2),     # CPU tensor
        lambda: sma.image_measure(np.zeros((0, 8, 3), np.uint8)),                     # H = 0
        lambda: sma.image_measure(np.zeros((8, 8, 4), np.uint8)),                     # 4 channels
        lambda: sma.image_measure(np.zeros((8, 8, 3), np.float64)),                   # dtype
        lambda: sma.image_measure(torch.zeros((8, 8), dtype=torch.uint8, device="cuda")),  # no channels
        lambda: sma.pyrDown(np.zeros((0, 8), np.uint8)),                              # H = 0
        lambda: sma.pyrDown(np.zeros((8, 8, 2), np.uint8)),                           # 2 channels
        lambda: sma.pyrDown(np.zeros((8, 8), np.int16)),                              # dtype
        lambda: sma.pyrDown(torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device="cuda")),  # 4 channels
        lambda: sma.pyrDown(np.zeros((8, 8), np.uint8), np.zeros((4, 5), np.uint8)),  # wrong dst
    ]
    for i, call in enumerate(bad):
        with pytest.raises((ValueError, _lib.SmError)):
            call()
        assert np.array_equal(sma.pyrDown(_u8(3, 5, 1)), _pyr_expected(3, 5, 1)), f"after bad call {i}"
    # the C-ABI's own checks
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    w = np.array([0.5, 0.25])
    eng.set_stream(None)
    with pytest.raises(ValueError, match="stride"):
        eng.gauss2d_batch_device(d.data_ptr(), 1, 0, 4, 8, 7, w, w, d.data_ptr() + 256, 0, 8)
    with pytest.raises(ValueError, match="16384"):
        eng.gauss2d_batch_device(d.data_ptr(), 1, 0, 4, 16385, 16385, w, w, d.data_ptr(), 0, 16385)
    with pytest.raises(ValueError, match="channels 2"):
        eng.pyr_down_batch_device(d.data_ptr(), 1, 0, 4, 4, 8, 2, d.data_ptr() + 256, 0, 4)
    eng.synchronize()
