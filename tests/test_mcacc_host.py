"""The accurate MC-CNN matching cost's CPU twin (sm_mcacc.hpp), which is the oracle
of the GPU tests: exact integers against an int64 numpy evaluation written from the network's
definition, float weights against torch on the CPU, the sigmoid against float64, argument errors.
No device is needed."""
import numpy as np
import pytest

import mcacc_cases as C
import stereo_match_amd as sm
from stereo_match_amd import _lib

# the exhaustive sweep's largest error of the sigmoid, in units of the last place
# of the float64 value rounded to float32 (tools/mcacc_sigmoid_sweep.cpp)
SIGMOID_MAX_ULP = 2.4808  # 2.4807 at z = -16.635704


# 160 and 352: a partial 128-column tile of the device's dense layer behind full ones; 256: two full ones
@pytest.mark.parametrize("F,U", [(2, 32), (3, 96), (2, 96), (3, 32), (3, 160), (2, 256), (3, 352)])
def test_exact_integers(F, U):
    """Every partial sum is an integer below 2^24, so the float32 twin must give the int64 values
    exactly, whatever the order of its sums; swapped halves or the wrong role give other values."""
    m = C.integer_model(2, F, U)
    fa, fb = C.integer_features("tiny", 0), C.integer_features("tiny", 1)
    D, m0 = 9, -3
    for left in (True, False):
        want, peak = C.int_volume(m, fa, fb, D, m0, left)
        assert 0 < peak < 2**24
        got = m.join(fa, fb, D, m0, a_is_left=left, raw=True, host=True)
        assert got.shape == (1, D) + fa.shape[:2] and got.dtype == np.float32
        assert C.same_bits(got[0], want), (F, U, left, int((got[0] != want).sum()))
    left, _ = C.int_volume(m, fa, fb, D, m0, True)
    wrong_role = m.join(fa, fb, D, m0, a_is_left=False, raw=True, host=True)[0]
    swapped = m.join(fb, fa, D, m0, a_is_left=True, raw=True, host=True)[0]
    ok = ~np.isnan(left)
    assert (wrong_role[ok] != left[ok]).mean() > 0.5 and (swapped[ok] != left[ok]).mean() > 0.5
    # a transposed hidden matrix is another network
    fws = [np.array(w) for w in m.fc_weights]
    fws[1] = np.ascontiguousarray(fws[1].T)
    other = sm.McCnnAccurate(m.weights, m.biases, fws, m.fc_biases).join(fa, fb, D, m0, raw=True, host=True)[0]
    assert (other[ok] != left[ok]).mean() > 0.5
    # the sigmoid of the same logits
    s = m.join(fa, fb, D, m0, host=True)[0]
    assert np.array_equal(s[ok], -_lib.mcacc_sigmoid_host(-left[ok]))


def test_integer_conv_net():
    """The 112-map integer net (two nonzero weights per output map, each at another input map and
    tap): its second layer equals a float64 numpy convolution of its first to 1e-4 -- sums of two
    terms, so a swapped tap or a transposed weight is far outside that."""
    m = C.integer_model(2)
    img = C.image("tiny", 0)
    f0 = sm.McCnnAccurate(m.weights[:1], m.biases[:1], m.fc_weights, m.fc_biases).features(img, host=True)
    f1 = C.twin_features("tiny", 2, 0, integer=True)
    H, W = img.shape
    pad = np.zeros((H + 2, W + 2, C.C))
    pad[1:-1, 1:-1] = f0
    w = m.weights[1].astype(np.float64)
    want = np.zeros((H, W, C.C))
    for ky in range(3):
        for kx in range(3):
            want += pad[ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].T
    want = np.maximum(want + m.biases[1], 0)
    assert np.abs(f1 - want).max() <= 1e-4 and np.abs(want).max() > 1


def torch_features(m, img, dtype):
    import torch
    import torch.nn.functional as F

    x = img.astype(np.float64)
    x = (x - x.mean()) / x.std(ddof=1)
    t = torch.from_numpy(x).to(dtype)[None, None]
    for w, b in zip(m.weights, m.biases):
        t = F.relu(F.conv2d(t, torch.tensor(w, dtype=dtype), torch.tensor(b, dtype=dtype), padding=1))
    return t[0].permute(1, 2, 0).contiguous()


def torch_volume(m, fa, fb, D, m0):
    """linear over the concatenated features (left first), ReLU, ..., sigmoid; NaN outside: [D, H, W]."""
    import torch
    import torch.nn.functional as F

    H, W, _ = fa.shape
    ws = [torch.tensor(w, dtype=fa.dtype) for w in m.fc_weights]
    bs = [torch.tensor(b, dtype=fa.dtype) for b in m.fc_biases]
    vol = torch.full((D, H, W), float("nan"), dtype=fa.dtype)
    for d in range(D):
        s = m0 + d
        lo, hi = max(0, s), min(W, W + s)
        if lo < hi:
            h = torch.cat((fa[:, lo:hi], fb[:, lo - s:hi - s]), 2)
            for i, (w, b) in enumerate(zip(ws, bs)):
                h = F.linear(h, w, b)
                if i < len(ws) - 1:
                    h = F.relu(h)
            vol[d, :, lo:hi] = -torch.sigmoid(h[..., 0])
    return vol


@pytest.mark.parametrize("name,D", [("tiny", 20), ("ragged", 12)])
def test_twin_against_torch_cpu(name, D):
    """max|twin - f64| <= BOUND x max|torch f32 - f64| on the features and on the volume's finite
    cells; equal NaN masks.  The bounds are twice the measured ratios, rounded up (DESIGN.md §4.20
    has the measurements): a sequential 1008-term chain against torch's blocked sums."""
    import torch

    m = C.model(4, 3, 384)
    a, b = C.image(name, 0), C.image(name, 1)
    ref = {}
    for dt in (torch.float64, torch.float32):
        fa, fb = torch_features(m, a, dt), torch_features(m, b, dt)
        ref[dt] = (fa.numpy(), fb.numpy(), torch_volume(m, fa, fb, D, 0).numpy())
    twin_a, twin_b = C.twin_features(name, 4, 0), C.twin_features(name, 4, 1)
    twin_v = m.join(twin_a, twin_b, D, 0, host=True)
    assert twin_v.shape == (1, D) + a.shape and twin_v.dtype == np.float32
    for what, twin, i in (("features a", twin_a, 0), ("features b", twin_b, 1)):
        err = np.abs(twin.astype(np.float64) - ref[torch.float64][i]).max()
        base = np.abs(ref[torch.float32][i].astype(np.float64) - ref[torch.float64][i]).max()
        print(f"{name} {what}: twin {err:.3e}, torch f32 {base:.3e}, ratio {err / base:.2f}")
        assert err <= FEATURE_BOUND * base, (what, err, base)
    v64, v32 = ref[torch.float64][2], ref[torch.float32][2]
    nan = np.isnan(v64)
    assert np.array_equal(np.isnan(twin_v[0]), nan) and np.array_equal(np.isnan(v32), nan)
    err = np.abs(twin_v[0].astype(np.float64) - v64)[~nan].max()
    base = np.abs(v32.astype(np.float64) - v64)[~nan].max()
    print(f"{name} volume: twin {err:.3e}, torch f32 {base:.3e}, ratio {err / base:.2f}")
    assert err <= VOLUME_BOUND * base, (err, base)
    assert np.nanmin(twin_v) >= -1.0 and np.nanmax(twin_v) <= 0.0


# measured: features 2.39, 3.36, 2.58, 2.54 -> 2 x 3.36 rounded up; volume 1.41, 1.41 -> 2 x 1.41 rounded up
FEATURE_BOUND = 7
VOLUME_BOUND = 3


def sigmoid_ulps(z):
    """Error of the twin's sigmoid against float64 1 / (1 + exp(-z)), in units of the last place of
    that value as a float32."""
    s = _lib.mcacc_sigmoid_host(z).astype(np.float64)
    ref = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    ulp = np.ldexp(1.0, np.floor(np.log2(ref)).astype(np.int64) - 23)
    return np.abs(s - ref) / ulp, s


def test_sigmoid_sample():
    """Every 509th bit pattern of [-80, 80] (4.2 million of the 2.2 x 10^9 the sweep visited) stays
    within the sweep's recorded maximum; the function does not decrease along the sample."""
    top = int(np.float32(80.0).view(np.uint32))
    bits = np.arange(0, top + 1, 509, dtype=np.uint32)
    assert 2 * bits.size >= 1 << 22
    for sign in (0, 0x80000000):
        z = (bits | np.uint32(sign)).view(np.float32)
        err, s = sigmoid_ulps(z)
        assert err.max() <= SIGMOID_MAX_ULP, (float(z[err.argmax()]), float(err.max()))
        order = np.argsort(z, kind="stable")
        assert np.all(np.diff(s[order]) >= 0)


def test_sigmoid_special_values():
    f = _lib.mcacc_sigmoid_host
    z = np.array([0.0, -0.0, np.inf, -np.inf, 80.0, -80.0, 1e30, -1e30, 100.0, -100.0, np.nan], np.float32)
    s = f(z)
    assert s[0] == 0.5 and s[1] == 0.5
    assert s[2] == 1.0 and s[4] == 1.0 and s[6] == 1.0 and s[8] == 1.0
    floor = s[5]
    assert 0 < floor < 2e-35 and abs(float(floor) / np.exp(-80.0) - 1) < 1e-6
    assert s[3] == floor and s[7] == floor and s[9] == floor  # beyond the clamp: the clamp's value, not 0
    assert np.isnan(s[10])
    assert np.isnan(f(np.array([-np.nan], np.float32)))[0]
    # 1 - s(z) and s(-z) agree to rounding, and the function is exactly 1 from some z on
    z = np.linspace(-30, 30, 2001).astype(np.float32)
    assert np.abs(f(z).astype(np.float64) + f(-z).astype(np.float64) - 1).max() < 2e-7
    assert f(np.array([17.5], np.float32))[0] == 1.0


def test_cost_volumes_host():
    """The right matcher's volume pairs the same columns through the same projections: equal values
    at the cells both volumes hold."""
    m = C.model(2, 2, 32)
    left, right = C.image("tiny", 0), C.image("tiny", 1)
    matcher = sm.StereoSGBM_create(minDisparity=-2, numDisparities=16)
    vl, vr = m.cost_volumes(left, right, matcher, host=True)
    rm = sm.createRightMatcher(matcher)
    assert C.same_bits(vl, m.cost_volume(left, right, 16, -2, host=True))
    assert C.same_bits(vr, m.cost_volume(right, left, rm.numDisparities, rm.minDisparity, a_is_left=False, host=True))
    W = left.shape[1]
    n = 0
    for d in range(16):
        s = -2 + d
        dr = -s - rm.minDisparity
        x = np.arange(W)
        ok = (x - s >= 0) & (x - s < W)
        assert 0 <= dr < 16
        assert np.array_equal(vr[0, dr][:, x[ok] - s], vl[0, d][:, ok])
        n += int(ok.sum())
    assert n > 500
    # with the wrong role the right volume is another function
    wrong = m.cost_volume(right, left, rm.numDisparities, rm.minDisparity, a_is_left=True, host=True)
    assert not C.same_bits(wrong, vr)


def test_batch_and_strides_host():
    m = C.model(2, 1, 32)
    batch = C.image("tiny", 3, batch=3)
    fb = m.features(batch, host=True)
    assert fb.shape == (3, 13, 45, 112) and fb.min() >= 0  # ReLU after the last layer too
    for i in range(3):
        assert np.array_equal(fb[i], m.features(batch[i], host=True))
    wide = np.zeros((3, 13, 64), np.uint8)
    wide[:, :, 5:50] = batch
    assert np.array_equal(m.features(wide[:, :, 5:50], host=True), fb)
    v = m.join(fb, fb[::-1], 5, 1, host=True)
    for i in range(3):
        assert C.same_bits(v[i], m.join(fb[i], fb[2 - i], 5, 1, host=True)[0])
    for far in (10**9, -10**9, 2**31 - 1, -2**31):
        assert np.isnan(m.join(fb[0], fb[1], 3, far, host=True)).all()


def test_argument_errors(tmp_path):
    good = C.model(2, 2, 32)
    w, b, fw, fb = good.weights, good.biases, good.fc_weights, good.fc_biases
    A = sm.McCnnAccurate
    with pytest.raises(ValueError):  # 64 maps
        A([w[0][:64]], [b[0][:64]], fw, fb)
    with pytest.raises(ValueError):  # wrong kernel size
        A([np.zeros((112, 1, 5, 5), np.float32)], [b[0]], fw, fb)
    with pytest.raises(ValueError):  # wrong dtype
        A([w[0].astype(np.float64)], [b[0]], fw, fb)
    with pytest.raises(ValueError):
        A(w, b, [x.astype(np.float64) for x in fw], fb)
    with pytest.raises(ValueError):  # layer 1 with one input map
        A([w[0], w[0]], [b[0], b[0]], fw, fb)
    with pytest.raises(ValueError):  # L = 0, L = 7
        A([], [], fw, fb)
    with pytest.raises(ValueError):
        A([w[0]] + [w[1]] * 6, [b[0]] * 7, fw, fb)
    with pytest.raises(ValueError):  # F = 0: the output unit alone
        A(w, b, [np.zeros((1, 224), np.float32)], [np.zeros(1, np.float32)])
    with pytest.raises(ValueError):
        A.random(2, 0, 32)
    with pytest.raises(ValueError):  # F = 5
        A.random(2, 5, 32)
    for units in (0, 16, 48, 416):  # U: a multiple of 32, 32 .. 384
        with pytest.raises(ValueError):
            A.random(2, 2, units)
    with pytest.raises(ValueError):  # fw0 with 128 input columns
        A(w, b, [fw[0][:, :128]] + fw[1:], fb)
    with pytest.raises(ValueError):  # a hidden matrix that is not U x U
        A(w, b, [fw[0], fw[1][:, :16], fw[2]], fb)
    with pytest.raises(ValueError):  # the output unit with two rows
        A(w, b, [fw[0], fw[1], np.zeros((2, 32), np.float32)], fb)
    with pytest.raises(ValueError):  # a bias of the wrong length
        A(w, b, fw, [fb[0][:16], fb[1], fb[2]])
    with pytest.raises(ValueError):  # one bias missing
        A(w, b, fw, fb[:2])
    img = C.image("tiny", 0)
    with pytest.raises(ValueError):  # a constant image
        good.features(np.full((13, 45), 9, np.uint8), host=True)
    with pytest.raises(ValueError):  # non-uint8 input
        good.features(img.astype(np.float32), host=True)
    with pytest.raises(ValueError, match="uint8"):
        good.cost_volume(img.tolist(), img.tolist(), 4, host=True)
    for D in (0, 257):
        with pytest.raises(ValueError):
            good.cost_volume(img, img, D, host=True)
    with pytest.raises(ValueError):
        good.cost_volume(img, img[:, :-1], 8, host=True)
    f64 = np.zeros((13, 45, 64), np.float32)
    with pytest.raises(ValueError):  # the fast net's features
        good.join(f64, f64, 4, host=True)
    with pytest.raises(ValueError):
        sm.McCnnStereo(object())
    # the C entry points check on their own
    F = _lib.load().sm_mcacc_join_host
    f = np.zeros((1, 2, 3, 112), np.float32)
    v = np.zeros((1, 2, 2, 3), np.float32)
    args = (f.ctypes.data, f.ctypes.data, 1, 2, 3, 2, 0, 1, 0, v.ctypes.data)
    assert F(2, 32, _lib._ptr_array(fw), _lib._ptr_array(fb), *args) == 0
    assert F(0, 32, _lib._ptr_array(fw), _lib._ptr_array(fb), *args) != 0
    assert F(2, 48, _lib._ptr_array(fw), _lib._ptr_array(fb), *args) != 0
    path = str(tmp_path / "net.npz")
    good.save_npz(path)
    again = A.from_npz(path)
    assert (again.layers, again.fc_layers, again.units) == (2, 2, 32)
    assert all(np.array_equal(x, y) for x, y in zip(again.weights + again.biases + again.fc_weights + again.fc_biases,
                                                    w + b + fw + fb))
    with pytest.raises(ValueError):
        again.fc_weights[0][0, 0] = 1.0
