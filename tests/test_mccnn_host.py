"""The MC-CNN matching cost's CPU twin (sm_mccnn.hpp), which is the oracle of the
GPU tests: against torch's CPU conv2d, on a rolled pair, the join's geometry, argument errors.
No device is needed."""
import numpy as np
import pytest

import mccnn_cases as C
import stereo_match_amd as sm


def torch_reference(m, img, dtype):
    """The same network with torch.nn.functional.conv2d on the CPU: features [H, W, 64]."""
    import torch
    import torch.nn.functional as F

    x = img.astype(np.float64)
    x = (x - x.mean()) / x.std(ddof=1)
    t = torch.from_numpy(x).to(dtype)[None, None]
    for i, (w, b) in enumerate(zip(m.weights, m.biases)):
        t = F.conv2d(t, torch.tensor(w, dtype=dtype), torch.tensor(b, dtype=dtype), padding=1)
        if i < m.layers - 1:
            t = F.relu(t)
    t = t / t.pow(2).sum(1, keepdim=True).sqrt()
    return t[0].permute(1, 2, 0).contiguous()


def torch_volume(fa, fb, D, m):
    """-sum_c A[y, x, c] B[y, x - (m + d), c] in the features' dtype, NaN outside: [D, H, W]."""
    import torch

    H, W, _ = fa.shape
    vol = torch.full((D, H, W), float("nan"), dtype=fa.dtype)
    for d in range(D):
        s = m + d
        lo, hi = max(0, s), min(W, W + s)
        if lo < hi:
            vol[d, :, lo:hi] = -(fa[:, lo:hi] * fb[:, lo - s:hi - s]).sum(2)
    return vol


@pytest.mark.parametrize("name,D", [("tiny", 20), ("ragged", 12)])
def test_twin_against_torch_cpu(name, D):
    """max|twin - f64| <= 4 max|torch f32 - f64|, features and the volume's finite cells; equal NaN
    masks.  4: a sequential 576-term chain against torch's blocked sums."""
    import torch

    m = C.model(4)
    a, b = C.image(name, 0), C.image(name, 1)
    ref = {}
    for dt in (torch.float64, torch.float32):
        fa, fb = torch_reference(m, a, dt), torch_reference(m, b, dt)
        ref[dt] = (fa.numpy(), fb.numpy(), torch_volume(fa, fb, D, 0).numpy())
    twin_a, twin_b = C.twin_features(name, 4, 0), C.twin_features(name, 4, 1)
    twin_v = m.join(twin_a, twin_b, D, 0, host=True)
    assert twin_v.shape == (1, D) + a.shape and twin_v.dtype == np.float32
    for what, twin, i in (("features a", twin_a, 0), ("features b", twin_b, 1)):
        err = np.abs(twin.astype(np.float64) - ref[torch.float64][i]).max()
        base = np.abs(ref[torch.float32][i].astype(np.float64) - ref[torch.float64][i]).max()
        print(f"{name} {what}: twin {err:.3e}, torch f32 {base:.3e}, ratio {err / base:.2f}")
        assert err <= 4 * base, (what, err, base)
    v64, v32 = ref[torch.float64][2], ref[torch.float32][2]
    nan = np.isnan(v64)
    assert np.array_equal(np.isnan(twin_v[0]), nan) and np.array_equal(np.isnan(v32), nan)
    err = np.abs(twin_v[0].astype(np.float64) - v64)[~nan].max()
    base = np.abs(v32.astype(np.float64) - v64)[~nan].max()
    print(f"{name} volume: twin {err:.3e}, torch f32 {base:.3e}, ratio {err / base:.2f}")
    assert err <= 4 * base, (err, base)


def test_rolled_pair():
    """right = roll(left, -5): same mean and std, so the interior features are the same bits, plane 5
    is -1 and the argmin over the planes is 5 at every interior pixel."""
    L, D = 4, 12
    m = C.model(L)
    left = C.image("ragged", 0)
    right = np.roll(left, -5, axis=1)
    fl, fr = m.features(left, host=True), m.features(right, host=True)
    H, W = left.shape
    lo, hi = L + 5 + 1, W - (L + 5) - 1  # columns more than L + 5 from either side
    assert hi - lo > 20
    assert np.array_equal(fl[:, lo:hi], fr[:, lo - 5:hi - 5])
    vol = m.join(fl, fr, D, 0, host=True)[0]
    assert np.abs(vol[5, :, lo:hi] + 1).max() <= 1e-6
    assert np.all(np.nanargmin(vol[:, :, lo:hi], axis=0) == 5)
    # cost_volume is the two steps
    assert C.same_bits(m.cost_volume(left, right, D, host=True)[0], vol)


@pytest.mark.parametrize("m0", [-7, 0, 4])
def test_join_geometry(m0):
    """Negative, zero and positive minDisparity; the swapped call is the plane-reversed,
    column-shifted volume where both are finite."""
    D = 9
    m = C.model(4)
    fa, fb = C.twin_features("tiny", 4, 0), C.twin_features("tiny", 4, 1)
    H, W, _ = fa.shape
    vol = m.join(fa, fb, D, m0, host=True)[0]
    mr = -(m0 + D) + 1
    volr = m.join(fb, fa, D, mr, host=True)[0]
    for d in range(D):
        s = m0 + d
        x = np.arange(W)
        ok = (x - s >= 0) & (x - s < W)
        assert np.array_equal(np.isnan(vol[d]), np.broadcast_to(~ok, (H, W)))
        want = -(fa[:, ok].astype(np.float64) * fb[:, x[ok] - s]).sum(2)
        assert np.abs(vol[d][:, ok] - want).max() <= 1e-6
        # left (x, d) pairs with right (x - s, d'), m_r + d' = -s
        dr = -s - mr
        assert 0 <= dr < D
        assert np.array_equal(volr[dr][:, x[ok] - s], vol[d][:, ok])


def test_more_planes_than_columns():
    m = C.model(1)
    f = C.twin_features("tiny", 1, 0)
    H, W, _ = f.shape
    vol = m.join(f, f, W + 20, 0, host=True)[0]
    assert vol.shape == (W + 20, H, W)
    assert np.isnan(vol[W:]).all()
    assert not np.isnan(vol[0]).any() and np.isnan(vol[W - 1][:, :W - 1]).all() and not np.isnan(vol[W - 1][:, W - 1]).any()
    for far in (10**9, -10**9, 2**31 - 1, -2**31):
        assert np.isnan(m.join(f, f, 3, far, host=True)).all()


def test_cost_volumes_host():
    m = C.model(2)
    left, right = C.image("tiny", 0), C.image("tiny", 1)
    matcher = sm.StereoSGBM_create(minDisparity=-2, numDisparities=16)
    vl, vr = m.cost_volumes(left, right, matcher, host=True)
    rm = sm.createRightMatcher(matcher)
    assert C.same_bits(vl, m.cost_volume(left, right, 16, -2, host=True))
    assert C.same_bits(vr, m.cost_volume(right, left, rm.numDisparities, rm.minDisparity, host=True))


def test_batch_and_strides_host():
    m = C.model(2)
    batch = C.image("tiny", 3, batch=3)
    fb = m.features(batch, host=True)
    for i in range(3):
        assert np.array_equal(fb[i], m.features(batch[i], host=True))
    wide = np.zeros((3, 13, 64), np.uint8)
    wide[:, :, 5:50] = batch
    assert np.array_equal(m.features(wide[:, :, 5:50], host=True), fb)


def test_argument_errors(tmp_path):
    good = C.model(2)
    w, b = good.weights, good.biases
    with pytest.raises(ValueError):  # wrong C
        sm.McCnnFast([w[0][:32]], [b[0][:32]])
    with pytest.raises(ValueError):  # wrong kernel size
        sm.McCnnFast([np.zeros((64, 1, 5, 5), np.float32)], [b[0]])
    with pytest.raises(ValueError):  # wrong dtype
        sm.McCnnFast([w[0].astype(np.float64)], [b[0]])
    with pytest.raises(ValueError):  # layer 1 with one input map
        sm.McCnnFast([w[0], w[0]], [b[0], b[0]])
    with pytest.raises(ValueError):  # L = 0
        sm.McCnnFast([], [])
    with pytest.raises(ValueError):  # L = 7
        sm.McCnnFast([w[0]] + [w[1]] * 6, [b[0]] * 7)
    with pytest.raises(ValueError):
        sm.McCnnFast.random(7)
    img = C.image("tiny", 0)
    with pytest.raises(ValueError):  # a constant image
        good.features(np.full((13, 45), 9, np.uint8), host=True)
    with pytest.raises(ValueError):  # non-uint8 input
        good.features(img.astype(np.float32), host=True)
    with pytest.raises(ValueError):
        good.cost_volume(img, img, 257, host=True)
    with pytest.raises(ValueError):
        good.cost_volume(img, img, 0, host=True)
    with pytest.raises(ValueError):
        good.cost_volume(img, img[:, :-1], 8, host=True)
    path = str(tmp_path / "net.npz")
    good.save_npz(path)
    again = sm.McCnnFast.from_npz(path)
    assert again.layers == 2 and all(np.array_equal(x, y) for x, y in zip(again.weights + again.biases, w + b))


def test_lists_and_frozen_weights():
    """A nested list goes through np.asarray like any array-like: it has no uint8 dtype, which is a
    ValueError (never an AttributeError); the net's arrays are private read-only copies."""
    m = C.model(2)
    img = C.image("tiny", 0)
    with pytest.raises(ValueError, match="uint8"):
        m.cost_volume(img.tolist(), img.tolist(), 4, host=True)
    with pytest.raises(ValueError):
        m.cost_volumes([[1.5, 2.5]], [[1.5, 2.5]], sm.StereoSGBM_create(numDisparities=16), host=True)
    w = [np.array(x) for x in m.weights]
    again = sm.McCnnFast(w, m.biases)
    w[0][:] = 0
    assert np.array_equal(again.weights[0], m.weights[0])
    with pytest.raises(ValueError):
        again.weights[0][0, 0, 0, 0] = 1.0
