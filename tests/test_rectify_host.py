"""Host side of the rectification front end (stereo_match_amd/rectify.py): stereoRectify's
geometry (reference-free: epipolar rows, Q round trip), the argument rules, rectify_opencv's
pose derivation, and known-answer tests of the numpy restatement tests/rectify_np.py."""
import numpy as np
import pytest

import rectify_np
from stereo_match_amd import _lib, rectify

W, H = 1280, 720
TOL = 1e-8  # px, resp. scene units: the correct procedure measures ~1e-11, a wrong sign / axis 1e-3 or worse


def _rodrigues(om):
    th = np.linalg.norm(om)
    if th == 0:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _rigs():
    rng = np.random.default_rng(20240607)
    rigs = []
    for n in range(200):
        Ks = []
        for _ in range(2):
            f = 1100 + rng.uniform(-50, 50)
            Ks.append(np.array([[f, 0, 640 + rng.uniform(-20, 20)], [0, f, 360 + rng.uniform(-20, 20)], [0, 0, 1.0]]))
        R = _rodrigues(rng.uniform(-0.1, 0.1, 3))
        T = np.array([-0.12, 0.0, 0.0]) + rng.uniform(-0.02, 0.02, 3)
        if n == 0:
            T = np.array([0.01, -0.12, 0.005])  # a vertical rig
        if n == 1:
            T = np.array([0.12, 0.01, -0.01])   # T_x > 0
        X = np.stack([rng.uniform(-1, 1, 50), rng.uniform(-1, 1, 50), rng.uniform(2, 10, 50)])
        rigs.append((Ks[0], Ks[1], R, T, X))
    return rigs


RIGS = _rigs()


@pytest.mark.parametrize("flags", [rectify.CALIB_ZERO_DISPARITY, 0])
def test_stereo_rectify_geometry(flags):
    worst_row = worst_q = 0.0
    for K1, K2, R, T, X in RIGS:
        R1, R2, P1, P2, Q, roi1, roi2 = rectify.stereoRectify(K1, None, K2, None, (W, H), R, T, flags=flags, alpha=-1)
        for Rk in (R1, R2):
            assert np.abs(Rk @ Rk.T - np.eye(3)).max() < TOL
            assert abs(np.linalg.det(Rk) - 1.0) < TOL
        vertical = abs(T[1]) > abs(T[0])
        idx = 1 if vertical else 0
        Xr = R1 @ X
        p1 = P1[:, :3] @ Xr
        p2 = P2 @ np.vstack([Xr, np.ones((1, X.shape[1]))])
        u1, u2 = p1[:2] / p1[2], p2[:2] / p2[2]
        # the same scene point through camera 2's own rectified chain: R2 (R X + T)
        q2 = P2[:, :3] @ (R2 @ (R @ X + T[:, None]))
        assert np.abs(q2[:2] / q2[2] - u2).max() < TOL
        row = np.abs(u1[idx ^ 1] - u2[idx ^ 1]).max()  # same row (same column for the vertical rig)
        worst_row = max(worst_row, row)
        assert row < TOL
        d = u1[idx] - u2[idx]
        back = Q @ np.vstack([u1, d[None], np.ones((1, X.shape[1]))])
        err = np.abs(back[:3] / back[3] - Xr).max()
        worst_q = max(worst_q, err)
        assert err < TOL
        if flags & rectify.CALIB_ZERO_DISPARITY:
            assert P1[0, 2] == P2[0, 2] and P1[1, 2] == P2[1, 2]
        else:
            assert P1[idx ^ 1, 2] == P2[idx ^ 1, 2]
        t = R2 @ T
        f = P1[0, 0]
        assert P1[1, 1] == f and P2[0, 0] == f and P2[1, 1] == f
        assert abs(P2[idx, 3] - t[idx] * f) < TOL and P2[idx ^ 1, 3] == 0
        assert abs(t[idx ^ 1]) < TOL and abs(t[2]) < TOL  # the baseline lies on the axis
        assert (T[idx] > 0) == (t[idx] > 0)
        assert f == min(K1[idx ^ 1, idx ^ 1], K2[idx ^ 1, idx ^ 1])
        assert roi1 == (0, 0, W, H) and roi2 == (0, 0, W, H)
    print(f"worst row disagreement {worst_row:.3g} px, worst Q reprojection error {worst_q:.3g}")
    assert worst_row < 1e-10 and worst_q < 1e-10  # measured ~1e-11; more than 1e-10 means something is off


def test_stereo_rectify_k1_shrinks_the_focal_length():
    K1, K2, R, T, _ = RIGS[5]
    k1 = -0.2
    P1 = rectify.stereoRectify(K1, [k1, 0, 0, 0, 0], K2, None, (W, H), R, T)[2]
    f = K1[1, 1] * (1 + k1 * (W * W + H * H) / (4 * K1[1, 1] ** 2))
    assert P1[0, 0] == min(f, K2[1, 1])


def test_stereo_rectify_alpha_in_unit_interval_is_unsupported():
    K1, K2, R, T, _ = RIGS[2]
    for alpha in (0, 0.5, 1):
        with pytest.raises(_lib.SmError) as e:
            rectify.stereoRectify(K1, None, K2, None, (W, H), R, T, alpha=alpha)
        assert e.value.code == _lib.SM_E_UNSUPPORTED and "alpha" in str(e.value)


def test_bad_shapes_raise_value_error():
    K1, K2, R, T, _ = RIGS[2]
    with pytest.raises(ValueError):
        rectify.stereoRectify(K1[:2], None, K2, None, (W, H), R, T)
    with pytest.raises(ValueError):
        rectify.stereoRectify(K1, None, K2, None, (W, H), R[:2], T)
    with pytest.raises(ValueError):
        rectify.stereoRectify(K1, None, K2, None, (W, H), R, T[:2])
    with pytest.raises(ValueError):
        rectify.stereoRectify(K1, np.zeros(3), K2, None, (W, H), R, T)
    with pytest.raises(ValueError):
        rectify.stereoRectify(K1, None, K2, None, (W,), R, T)
    with pytest.raises(ValueError):
        rectify.relative_pose(np.eye(3), np.eye(4))


def test_rectify_opencv_pose_derivation():
    """rotation / translation are the blocks of inv(pose_r) @ pose_l (disparity_calculation.py:163-165)."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        pl, pr = np.eye(4), np.eye(4)
        pl[:3, :3], pr[:3, :3] = _rodrigues(rng.uniform(-1, 1, 3)), _rodrigues(rng.uniform(-1, 1, 3))
        pl[:3, 3], pr[:3, 3] = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
        rot, tr = rectify.relative_pose(pl, pr)
        rel = np.linalg.inv(pr) @ pl
        assert np.abs(rot - rel[:3, :3]).max() < 1e-12 and np.abs(tr - rel[:3, 3]).max() < 1e-12


# ---- known-answer tests of the restatement itself

def _grid(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return xx.astype(np.float32), yy.astype(np.float32)


@pytest.mark.parametrize("cn", [1, 3])
def test_np_identity_map_returns_the_source(cn):
    rng = np.random.default_rng(cn)
    src = rng.integers(0, 256, (9, 14) if cn == 1 else (9, 14, 3), dtype=np.uint8)
    mx, my = _grid(9, 14)
    assert np.array_equal(rectify_np.remap(src, mx, my), src)


def test_np_hand_computed_bilinear():
    src = np.array([[10, 20], [30, 40]], np.uint8)
    # x = 0.25 (fx 8), y = 0.75 (fy 24): a00 = 24*8, a01 = 8*8, a10 = 24*24, a11 = 8*24
    got = rectify_np.remap(src, np.array([[0.25]], np.float32), np.array([[0.75]], np.float32))
    assert got[0, 0] == (192 * 10 + 64 * 20 + 576 * 30 + 192 * 40 + 512) >> 10 == 28
    # the middle: all four weights 256
    got = rectify_np.remap(src, np.array([[0.5]], np.float32), np.array([[0.5]], np.float32))
    assert got[0, 0] == 25


def test_np_ties_round_half_to_even():
    src = np.array([[0, 255]], np.uint8)
    # m*32 = 4.5 -> 4 (even), 5.5 -> 6: weights of the right tap 4/32 and 6/32
    mx = np.array([[4.5 / 32, 5.5 / 32]], np.float32)
    got = rectify_np.remap(src, mx, np.zeros((1, 2), np.float32))
    assert got.tolist() == [[(4 * 32 * 255 + 512) >> 10, (6 * 32 * 255 + 512) >> 10]]
    # negative ties: -0.5 -> -0 (ix 0, f 0), -1.5 -> -2 (ix -1, f 30)
    mx = np.array([[-0.5 / 32, -1.5 / 32]], np.float32)
    got = rectify_np.remap(np.array([[200, 0]], np.uint8), mx, np.zeros((1, 2), np.float32))
    assert got.tolist() == [[200, (30 * 32 * 200 + 512) >> 10]]


def test_np_outside_taps_and_borders():
    src = np.full((3, 4), 200, np.uint8)
    z = np.zeros((1, 1), np.float32)

    def at(x, y):
        return int(rectify_np.remap(src, z + np.float32(x), z + np.float32(y))[0, 0])

    assert at(-2, 1) == 0 and at(5, 1) == 0 and at(1, -1.5) == 0 and at(1, 4) == 0  # all four taps outside
    assert at(np.nan, 1) == 0 and at(1, np.inf) == 0 and at(-np.inf, 1) == 0 and at(1e30, 1) == 0
    half = (16 * 32 * 200 + 512) >> 10
    assert at(-0.5, 1) == half   # left border: taps x = -1 (0) and x = 0
    assert at(3.5, 1) == half    # right border
    assert at(1, -0.5) == half   # top
    assert at(1, 2.5) == half    # bottom
    assert at(-0.5, -0.5) == (16 * 16 * 200 + 512) >> 10  # corner: one tap inside
    assert at(3, 2) == 200 and at(-0.0, 0) == 200


def test_np_gray_known_answers():
    px = np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    assert rectify_np.bgr2gray(px).tolist() == [255, 0, 29, 150, 76]


def test_np_rectify_map_identity_camera():
    """iR = inv(K), no distortion: the map is the pixel grid."""
    K = np.array([[1000.0, 0, 31.5], [0, 1000.0, 17.25], [0, 0, 1]])
    mx, my = rectify_np.rectify_map(K, np.zeros(5), np.linalg.inv(K), 6, 9)
    gx, gy = _grid(6, 9)
    assert np.abs(mx - gx).max() < 1e-4 and np.abs(my - gy).max() < 1e-4
