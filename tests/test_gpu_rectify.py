"""GPU: the rectification front end (sm_rectify.hpp: k_rectify_map, k_remap_u8, k_bgr2gray;
stereo_match_amd/rectify.py) against the independent numpy restatement tests/rectify_np.py,
bit for bit: maps, remap (tails, strides, borders, ties, non-finite coordinates), the fused
gray output, batches, the torch path, the raw-frames-to-disparity chain, argument errors."""
import numpy as np
import pytest

import rectify_np
from stereo_match_amd import _lib, rectify, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _rig(seed, W, H, f=None):
    """A seeded rig in the style of tests/test_rectify_host.py, scaled to the image size."""
    rng = np.random.default_rng(seed)
    f = f or 0.9 * W
    Ks = [np.array([[f + rng.uniform(-5, 5), 0, W / 2 + rng.uniform(-3, 3)],
                    [0, f + rng.uniform(-5, 5), H / 2 + rng.uniform(-3, 3)], [0, 0, 1.0]]) for _ in range(2)]
    om = rng.uniform(-0.03, 0.03, 3)
    T = np.array([-0.12, 0.0, 0.0]) + rng.uniform(-0.01, 0.01, 3)
    return Ks[0], Ks[1], om, T


CAMERAS = {
    "zero": np.zeros(5),
    "mild": np.array([-0.05, 0.01, 0.001, -0.0005, 0.002]),
    "barrel": np.array([-0.4, 0.12, 0.0, 0.0, -0.01]),
}


# ---- maps

@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("H,W", [(45, 77), (1, 1)])
def test_rectify_map_small(eng, cam, H, W):
    _check_map(eng, cam, H, W)


def test_rectify_map_full_frame(eng):
    _check_map(eng, "mild", 720, 1280)


def _check_map(eng, cam, H, W):
    dist = CAMERAS[cam]
    K1, K2, om, T = _rig(7, 1280, 720)
    R1, R2, P1, P2, Q, _, _ = rectify.stereoRectify(K1, dist, K2, dist, (1280, 720), om, T)
    for K, R, P in ((K1, R1, P1), (K2, R2, P2)):
        c = rectify._rectify_cam(K, dist, R, P)
        iR = np.array(c.iR[:], np.float64)  # the very doubles the device gets
        mx, my = eng.rectify_map(c, H, W)
        ex, ey = rectify_np.rectify_map(K, dist, iR, H, W)
        assert mx.dtype == np.float32 and mx.shape == (H, W)
        assert np.array_equal(mx.view(np.uint32), ex.view(np.uint32))
        assert np.array_equal(my.view(np.uint32), ey.view(np.uint32))
    mx2, my2 = rectify.initUndistortRectifyMap(K2, dist, R2, P2, (W, H))
    assert np.array_equal(mx2.view(np.uint32), mx.view(np.uint32)) and np.array_equal(my2.view(np.uint32),
                                                                                      my.view(np.uint32))


# ---- remap

def _source(name):
    rng = np.random.default_rng(len(name))
    if name == "c3_37x67":
        return rng.integers(0, 256, (37, 67, 3), dtype=np.uint8)
    if name == "c1_33x130":
        return rng.integers(0, 256, (33, 130), dtype=np.uint8)
    if name == "c3_1x1":
        return np.array([[[13, 200, 77]]], np.uint8)
    if name == "c1_5x4":
        return rng.integers(0, 256, (5, 4), dtype=np.uint8)
    if name == "c3_37x67_strided":  # src_stride > W * cn: a view into a wider buffer
        buf = rng.integers(0, 256, (37, 75, 3), dtype=np.uint8)
        return buf[:, :67]
    raise KeyError(name)


SOURCES = ["c3_37x67", "c1_33x130", "c3_1x1", "c1_5x4", "c3_37x67_strided"]


def _maps(h, w, H, W, seed):
    """Seeded maps over [-3, w+3) x [-3, h+3) with the special values sprinkled in."""
    rng = np.random.default_rng(seed)
    n = H * W
    mx = rng.uniform(-3, w + 3, n).astype(np.float32)
    my = rng.uniform(-3, h + 3, n).astype(np.float32)
    kind = rng.integers(0, 8, n)
    # exact integers
    sel = kind == 1
    mx[sel] = rng.integers(-2, w + 2, sel.sum())
    my[sel] = rng.integers(-2, h + 2, sel.sum())
    # exact ties k/32 + 1/64 (even and odd k, both signs)
    sel = kind == 2
    mx[sel] = (rng.integers(-64, 32 * (w + 1), sel.sum()) / 32.0 + 1.0 / 64).astype(np.float32)
    my[sel] = (rng.integers(-64, 32 * (h + 1), sel.sum()) / 32.0 + 1.0 / 64).astype(np.float32)
    # special values at fixed places (as many as fit), in x, in y and in both
    one = np.float32(1)
    specials = [np.float32(-0.0), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(1e30),
                np.float32(-1e30), np.float32(16777216.0), np.float32(-16777216.0), np.float32(16777215.0),
                np.nextafter(np.float32(w - 1), np.float32(np.inf)), np.nextafter(np.float32(w - 1), -one * 9),
                np.float32(w - 1), np.nextafter(np.float32(-1), np.float32(0)),
                np.nextafter(np.float32(-1), np.float32(-2)), np.float32(-1),
                np.nextafter(np.float32(h - 1), np.float32(np.inf)), np.nextafter(np.float32(h - 1), -one * 9)]
    pos = rng.permutation(n)
    for k, v in enumerate(specials * 3):
        if k >= n:
            break
        which = k // len(specials)
        if which in (0, 2):
            mx[pos[k]] = v
        if which in (1, 2):
            my[pos[k]] = v
    return mx.reshape(H, W), my.reshape(H, W)


@pytest.mark.parametrize("name", SOURCES)
@pytest.mark.parametrize("H,W", [(1, 1), (19, 3), (1, 4), (19, 5), (19, 67), (1, 259), (19, 259), (19, 260)])
def test_remap_matches_restatement(eng, name, H, W):
    src = _source(name)
    h, w = src.shape[:2]
    mx, my = _maps(h, w, H, W, seed=H * 1000 + W)
    exp = rectify_np.remap(src, mx, my)
    dst, none = eng.remap(src, mx, my, True, False)
    assert none is None and np.array_equal(dst, exp)
    assert np.array_equal(rectify.remap(src, mx, my), exp)
    if src.ndim == 3:
        exp_gray = rectify_np.bgr2gray(exp)
        none, gray = eng.remap(src, mx, my, False, True)
        assert none is None and np.array_equal(gray, exp_gray)
        dst2, gray2 = eng.remap(src, mx, my, True, True)
        assert np.array_equal(dst2, exp) and np.array_equal(gray2, exp_gray)
        assert np.array_equal(gray2, rectify_np.bgr2gray(dst2))


@pytest.mark.parametrize("shape", [(37, 67, 3), (33, 130), (1, 1, 3), (5, 4), (20, 64, 3)])
def test_identity_map_returns_the_source(eng, shape):
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, shape, dtype=np.uint8)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    out = rectify.remap(src, xx.astype(np.float32), yy.astype(np.float32))
    assert np.array_equal(out, src)


def test_gray_matches_restatement(eng):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (1025, 1024, 3), dtype=np.uint8)  # 2^20 random triples + one more row
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    img[1024, :8] = corners
    got = rectify.cvtColor(img, rectify.COLOR_BGR2GRAY)
    assert got.shape == (1025, 1024) and np.array_equal(got, rectify_np.bgr2gray(img))
    assert got[1024, :8].tolist() == rectify_np.bgr2gray(corners).tolist()


# ---- batch, torch

def test_batch_with_image_stride_equals_single_calls(eng):
    import torch

    rng = np.random.default_rng(21)
    h, w, H, W, n = 37, 67, 19, 68, 3
    stride = w * 3 + 5
    img_stride = h * stride + 333  # larger than the image
    buf = rng.integers(0, 256, n * img_stride, dtype=np.uint8)
    mx, my = _maps(h, w, H, W, seed=2)
    singles = []
    for i in range(n):
        v = np.lib.stride_tricks.as_strided(buf[i * img_stride:], (h, w, 3), (stride, 3, 1))
        singles.append(eng.remap(v, mx, my, True, True))
        assert np.array_equal(singles[-1][0], rectify_np.remap(np.ascontiguousarray(v), mx, my))
    dev = torch.device("cuda", 0)
    d_buf, d_mx, d_my = (torch.from_numpy(a).to(dev) for a in (buf, mx, my))
    d_dst = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=dev)
    d_gray = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.remap_batch_device(d_buf.data_ptr(), n, img_stride, h, w, stride, 3, d_mx.data_ptr(), d_my.data_ptr(), H, W,
                           d_dst.data_ptr(), d_gray.data_ptr())
    eng.synchronize()
    for i in range(n):
        assert np.array_equal(d_dst[i].cpu().numpy(), singles[i][0])
        assert np.array_equal(d_gray[i].cpu().numpy(), singles[i][1])
    # seven images: more than one thread's share of the batch, gray only
    d_gray7 = torch.zeros((7, H, W), dtype=torch.uint8, device=dev)
    d_buf7 = torch.from_numpy(np.concatenate([buf, buf, buf[:img_stride]])).to(dev)
    torch.cuda.synchronize()
    eng.remap_batch_device(d_buf7.data_ptr(), 7, img_stride, h, w, stride, 3, d_mx.data_ptr(), d_my.data_ptr(), H, W,
                           None, d_gray7.data_ptr())
    eng.synchronize()
    for i in range(7):
        assert np.array_equal(d_gray7[i].cpu().numpy(), singles[i % 3][1])


def test_torch_path_on_a_side_stream():
    import torch

    rng = np.random.default_rng(31)
    src = rng.integers(0, 256, (37, 67, 3), dtype=np.uint8)
    mx, my = _maps(37, 67, 19, 259, seed=9)
    exp = rectify.remap(src, mx, my)
    assert np.array_equal(exp, rectify_np.remap(src, mx, my))
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    try:
        with torch.cuda.stream(st):
            t_src, t_mx, t_my = (torch.from_numpy(a).to(dev) for a in (src, mx, my))
            out = rectify.remap(t_src, t_mx, t_my)
            gray = rectify.cvtColor(out)
        st.synchronize()
        assert out.is_cuda and np.array_equal(out.cpu().numpy(), exp)
        assert np.array_equal(gray.cpu().numpy(), rectify_np.bgr2gray(exp))
    finally:
        _lib.engine(0).set_stream(None)


# ---- the chain: raw frames -> displ, filtered, img_rect1, Q

def _bgr(gray, seed):
    """A BGR image built from a gray one: channels differ (tests/test_gpu_wide.py style)."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 20, gray.shape, dtype=np.uint8)
    return np.ascontiguousarray(np.stack([gray, np.roll(gray, 1, 0) // 2 + noise, 255 - gray], -1))


def test_chain_raw_frames_to_disparity():
    import stereo_match_amd as sm

    H, W, D = 96, 224, 64
    gl, gr, _ = synthetic.random_dot_pair(H, W, D, seed=1)
    vis_l, vis_r = _bgr(gl, 1), _bgr(gr, 2)
    K1, K2, om, T = _rig(3, W, H)
    dist = CAMERAS["mild"]
    settings = dict(sm.DEFAULT_SETTINGS, window_size=5, num_disparities=D)  # synthetic.parity_params(64)
    sr = rectify.StereoRectifier(K1, dist, K2, dist, (W, H), om, T)
    e = _lib.engine(0)
    try:
        before = e.counters()["sweep_fallbacks"]
        displ, filtered, img_rect1, Q = sr.compute_disparity(vis_l, vis_r, settings)
        after = e.counters()["sweep_fallbacks"]
        rect_l, rect_r, gray_l, gray_r = (t.cpu().numpy() for t in sr.rectify(vis_l, vis_r))
    finally:
        e.set_stream(None)
    assert after - before == 0

    R1, R2, P1, P2, Q0, _, _ = rectify.stereoRectify(K1, dist, K2, dist, (W, H), om, T)
    assert np.array_equal(Q, Q0)
    exp = []
    for K, R, P, vis in ((K1, R1, P1, vis_l), (K2, R2, P2, vis_r)):
        c = rectify._rectify_cam(K, dist, R, P)
        mx, my = rectify_np.rectify_map(K, dist, np.array(c.iR[:]), H, W)
        exp.append(rectify_np.remap(vis, mx, my))
    assert np.array_equal(img_rect1, exp[0])
    assert np.array_equal(rect_l, exp[0]) and np.array_equal(rect_r, exp[1])
    g_l, g_r = rectify_np.bgr2gray(exp[0]), rectify_np.bgr2gray(exp[1])
    assert np.array_equal(gray_l, g_l) and np.array_equal(gray_r, g_r)
    d_ref, f_ref = sm.compute_disparity(g_l, g_r, settings)
    assert np.array_equal(displ, d_ref) and np.array_equal(filtered, f_ref)

    # the reference's own function on the same rig, from poses
    pose_l, pose_r = np.eye(4), np.eye(4)
    Rm = rectify._rodrigues_vec(om)
    pose_r[:3, :3], pose_r[:3, 3] = Rm.T, -Rm.T @ T  # inv(pose_r) @ pose_l = [R | T]
    r1, r2, Qo = rectify.rectify_opencv(pose_l, pose_r, K1, K2, vis_l, vis_r, dist, dist)
    rot, tr = rectify.relative_pose(pose_l, pose_r)
    Ro = rectify.stereoRectify(K1, dist, K2, dist, (W, H), rot, tr)
    for K, R, P, vis, got in ((K1, Ro[0], Ro[2], vis_l, r1), (K2, Ro[1], Ro[3], vis_r, r2)):
        c = rectify._rectify_cam(K, dist, R, P)
        mx, my = rectify_np.rectify_map(K, dist, np.array(c.iR[:]), H, W)
        assert np.array_equal(got, rectify_np.remap(vis, mx, my))
    assert np.array_equal(Qo, Ro[4])


# ---- argument errors

def test_argument_errors_leave_the_context_usable(eng):
    src3 = np.zeros((5, 6, 3), np.uint8)
    src1 = np.zeros((5, 6), np.uint8)
    mx = np.zeros((4, 4), np.float32)

    def code():
        return eng._lib.sm_last_error(eng.ctx)

    with pytest.raises(ValueError):
        eng.remap(src3, mx, mx, False, False)  # both outputs null
    with pytest.raises(ValueError):
        eng.remap(np.zeros((5, 6, 2), np.uint8), mx, mx, True, False)  # channels = 2
    with pytest.raises(ValueError):
        eng.remap(src1, mx, mx, True, True)  # gray of a 1-channel source
    with pytest.raises(ValueError):
        eng.remap(src3, np.zeros((4, 0), np.float32), np.zeros((4, 0), np.float32), True, False)  # W = 0
    big = np.zeros((1, 16385), np.float32)
    with pytest.raises(ValueError):
        eng.remap(src3, big, big, True, False)  # W = 16385
    with pytest.raises(ValueError):
        eng.rectify_map(rectify._rectify_cam(np.eye(3), None, None, None), 1, 16385)
    assert code()  # the last error text is set
    # the raw return code is SM_E_ARG
    rc = eng._lib.sm_remap_u8(eng.ctx, src3.ctypes.data, 5, 6, 18, 3, mx.ctypes.data, mx.ctypes.data, 4, 4, None, None)
    assert rc == _lib.SM_E_ARG
    # ... and the context still works
    out, gray = eng.remap(src3 + 7, mx, mx, True, True)
    assert (out == 7).all() and (gray == 7).all()
