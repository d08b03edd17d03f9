"""GPU: reprojectImageTo3D and the per-map minimum (csrc/sm_reproject.hpp: k_reproject, k_disp_min,
k_keys_to_float; csrc/sm_api_cloud.hip; stereo_match_amd/reproject.py) against
oracle/reproject_np.py on the inputs of tests/reproject_cases.py.  Every comparison is bit for
bit where the value is not a NaN and NaN position for NaN position (the sign of a NaN that
0 * inf makes is the processor's own).  tests/test_reproject_oracle.py checks the oracle and the
cases themselves on the CPU."""
import functools
import itertools

import numpy as np
import pytest

import reproject_cases as C
import stereo_match_amd as sm
from oracle import reproject_np
from stereo_match_amd import _lib

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"NaN positions differ on {int((gn != wn).sum())} values"
    bad = got.view(np.uint32)[~gn] != want.view(np.uint32)[~wn]
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ"


def marked(out):
    return tuple(np.flatnonzero(np.asarray(out)[..., 2].reshape(-1) == C.BIG_Z).tolist())


@functools.lru_cache(maxsize=None)
def _oracle_grid(H, W, kind, Qn, hm):
    out = reproject_np.reproject_image_to_3d(C.grid_map(H, W, kind, Qn), C.Q_of(Qn), hm)
    out.setflags(write=False)
    return out


def run_device(eng, maps, Q, hm, fill=None):
    """[n, H, W] maps through reproject_device on torch's current stream: float32 [n, H, W, 3]."""
    import torch

    n, H, W = maps.shape
    t = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    out = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
    if fill is not None:
        out.fill_(fill)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.reproject_device(t.data_ptr(), 0 if maps.dtype == np.int16 else 1, n, H, W, Q, hm, out.data_ptr())
    return out.cpu().numpy()


@pytest.fixture
def eng():
    e = _lib.engine(0)
    yield e
    e.set_stream(None)


# ---- the shape grid
@pytest.mark.parametrize("hm", [False, True])
@pytest.mark.parametrize("Qn", ["calc", "dense"])
@pytest.mark.parametrize("kind", ["s16", "f32"])
@pytest.mark.parametrize("H,W", C.SHAPES)
def test_shape_grid(H, W, kind, Qn, hm):
    """One pixel, one row, widths around the 256 threads of a block, two blocks a row, an odd
    shape and a map of more than 256 * 1024 pixels whose unique minimum only k_disp_min's second
    grid-stride step sees.  The dense float32 maps hold the cancellation pixels on which FP
    contraction changes the float32 result (test_reproject_oracle.py)."""
    d = C.grid_map(H, W, kind, Qn)
    want = _oracle_grid(H, W, kind, Qn, hm)
    got = sm.reprojectImageTo3D(d, C.Q_of(Qn), handleMissingValues=hm)
    assert_same(got, want)
    assert marked(got) == ((C.min_position(H, W),) if hm else ())


# ---- special values and the FLT_EPSILON window, rule 1
@pytest.mark.parametrize("Qn", ["calc", "dense"])
@pytest.mark.parametrize("case", C.SPECIAL_CASES)
def test_special_values(case, Qn):
    outs = []
    for sign in (+1, -1):
        d = C.special_map(case, sign)
        got = sm.reprojectImageTo3D(d, C.Q_of(Qn), handleMissingValues=True)
        assert_same(got, reproject_np.reproject_image_to_3d(d, C.Q_of(Qn), True))
        assert marked(got) == C.SPECIAL_MARKED[case]
        outs.append(got)
    assert_same(outs[0], outs[1])  # the NaNs' sign changes nothing
    if case == "specials":
        assert len(marked(outs[0])) == 7


@pytest.mark.parametrize("md", C.LADDER_MD)
def test_ladder(md):
    want_marked = tuple(sorted(p for p, f in zip(C.LADDER_AT, C.LADDER_FLAGS[md]) if f))
    assert len(want_marked) in (2, 3)
    outs = []
    for sign in (+1, -1):
        d = C.ladder_map(md, sign)
        got = sm.reprojectImageTo3D(d, C.Q_CALC, handleMissingValues=True)
        assert_same(got, reproject_np.reproject_image_to_3d(d, C.Q_CALC, True))
        assert marked(got) == want_marked
        outs.append(got)
    assert_same(outs[0], outs[1])


@pytest.mark.parametrize("H,W,nan_at,min_at", C.position_cases())
def test_nan_and_minimum_positions(H, W, nan_at, min_at):
    outs = []
    for sign in (+1, -1):
        d = C.position_map(H, W, nan_at, min_at, sign)
        got = sm.reprojectImageTo3D(d, C.Q_CALC, handleMissingValues=True)
        assert marked(got) == (min_at,)
        outs.append(got)
    assert_same(outs[0], reproject_np.reproject_image_to_3d(C.position_map(H, W, nan_at, min_at, +1), C.Q_CALC, True))
    assert_same(outs[0], outs[1])


# ---- batches through reproject_device
def _three_minima(kind):
    """Three 37 x 53 maps with the minima -16, 3 and 40 (each at its own position)."""
    base = C.grid_map(37, 53, kind)
    lo = {"s16": 50, "f32": np.float32(50.5)}[kind]
    maps = np.stack([np.maximum(base, lo) for _ in range(3)])
    for i, (m, at) in enumerate(((-16, 700), (3, 64), (40, 1960))):
        maps[i].reshape(-1)[at] = m
    return maps


@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_batch_three_different_minima(eng, kind):
    maps = _three_minima(kind)
    want = [reproject_np.reproject_image_to_3d(m, C.Q_REF, True) for m in maps]
    assert [marked(w) for w in want] == [(700,), (64,), (1960,)]
    for a, b in itertools.permutations(range(3), 2):
        got = run_device(eng, maps[[a, b]], C.Q_REF, True)
        assert_same(got[0], want[a])
        assert_same(got[1], want[b])
    got = run_device(eng, maps, C.Q_REF, True)
    for i in range(3):
        assert_same(got[i], want[i])


@pytest.mark.parametrize("sign", [+1, -1])
def test_batch_one_image_with_nans(eng, sign):
    maps = _three_minima("f32")
    C.put_nans(maps[1], (0, 65, 1000, 1959), sign)
    want = [reproject_np.reproject_image_to_3d(m, C.Q_REF, True) for m in maps]
    assert [marked(w) for w in want] == [(700,), (64,), (1960,)]
    got = run_device(eng, maps, C.Q_REF, True)
    for i in range(3):
        assert_same(got[i], want[i])


def _sixty_five(kind):
    """65 maps of 4 x 5, map i with its own minimum -i - 1 at pixel i % 20: the 65th is the
    second block of k_keys_to_float."""
    rng = np.random.default_rng(65)
    maps = rng.integers(0, 200, (65, 4, 5)).astype(np.int16 if kind == "s16" else np.float32)
    for i in range(65):
        maps[i].reshape(-1)[i % 20] = -i - 1
    return maps


@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_batch_of_65(eng, kind):
    maps = _sixty_five(kind)
    got = run_device(eng, maps, C.Q_REF, True)
    for i in range(65):
        assert_same(got[i], reproject_np.reproject_image_to_3d(maps[i], C.Q_REF, True))
        assert marked(got[i]) == (i % 20,)


def test_batch_of_none_leaves_the_output_alone(eng):
    import torch

    t = torch.zeros((1, 4, 5), dtype=torch.int16, device="cuda")
    out = torch.full((1, 4, 5, 3), -7.0, dtype=torch.float32, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.reproject_device(t.data_ptr(), 0, 0, 4, 5, C.Q_REF, True, out.data_ptr())
    assert (out.cpu().numpy() == -7.0).all()


# ---- one context, consecutive calls
def test_consecutive_calls_on_one_context():
    """A context of its own, so that the minima buffer's history is this test's: a larger minimum
    after a smaller one (a key left over from the first call would mark nothing), the buffer
    growing from 1 map to 65 and being reused for 1, and int16 followed by float32."""
    e = _lib.Engine(0)
    try:
        maps = _three_minima("s16")
        first, second = maps[0], maps[2]
        assert first.min() == -16 and second.min() == 40
        got = e.reproject(first, C.Q_REF, True)
        assert_same(got, reproject_np.reproject_image_to_3d(first, C.Q_REF, True))
        got = e.reproject(second, C.Q_REF, True)
        assert_same(got, reproject_np.reproject_image_to_3d(second, C.Q_REF, True))
        assert marked(got) == (1960,)
        many = _sixty_five("s16")
        got = run_device(e, many, C.Q_REF, True)
        for i in range(65):
            assert_same(got[i], reproject_np.reproject_image_to_3d(many[i], C.Q_REF, True))
        e.set_stream(None)
        got = e.reproject(second, C.Q_REF, True)
        assert marked(got) == (1960,)
        assert_same(got, reproject_np.reproject_image_to_3d(second, C.Q_REF, True))
        f = _three_minima("f32")[1]
        got = e.reproject(f, C.Q_DENSE, True)
        assert marked(got) == (64,)
        assert_same(got, reproject_np.reproject_image_to_3d(f, C.Q_DENSE, True))
    finally:
        e.set_stream(None)
        e.close()


# ---- division by zero and overflow
@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_exact_zero_denominator(kind):
    d, zero = C.zero_w_map(kind)
    want = reproject_np.reproject_image_to_3d(d, C.Q_ZERO)
    got = sm.reprojectImageTo3D(d, C.Q_ZERO)
    assert_same(got, want)
    assert np.isnan(got).any() and np.isposinf(got).any() and np.isneginf(got).any()
    assert not np.isfinite(got[zero]).any() and np.isfinite(got[~zero]).all()
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(want))


@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_float32_overflow(kind):
    """Q_IN: X overflows float32 where Y and Z are finite; d = 0 in column 1 is 0 * inf."""
    d = C.grid_map(37, 53, kind).copy()
    d[:, 1] = 0
    d[::3, ::4] = 0
    want = reproject_np.reproject_image_to_3d(d, C.Q_IN)
    got = sm.reprojectImageTo3D(d, C.Q_IN)
    assert_same(got, want)
    assert np.isnan(got).any() and np.isposinf(got).any() and np.isneginf(got).any()
    rows = ~np.isfinite(got).all(-1)
    assert np.isfinite(got[rows]).any()  # X alone overflows
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(want))


# ---- the Python surface
@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_column_slice_of_a_wider_array(kind):
    wide = np.concatenate([C.grid_map(37, 53, kind)[:, ::-1], C.grid_map(37, 53, kind)], 1)
    view = wide[:, 53:]
    assert not view.flags.c_contiguous and np.array_equal(view, C.grid_map(37, 53, kind))
    assert_same(sm.reprojectImageTo3D(view, C.Q_CALC, handleMissingValues=True), _oracle_grid(37, 53, kind, "calc", True))


@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_strided_tensor_on_a_side_stream(kind):
    import torch

    d = C.grid_map(37, 53, kind)
    wide = torch.from_numpy(np.concatenate([d[:, ::-1], d], 1)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side):
            view = wide[:, 53:]
            assert not view.is_contiguous()
            out = sm.reprojectImageTo3D(view, C.Q_CALC, handleMissingValues=True)
            assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (37, 53, 3)
        side.synchronize()
        assert_same(out.cpu().numpy(), _oracle_grid(37, 53, kind, "calc", True))
    finally:
        _lib.engine(0).set_stream(None)


def test_3dimage_is_filled_and_returned():
    d = C.grid_map(37, 53, "s16")
    buf = np.full((37, 53, 3), -7.0, np.float32)
    out = sm.reprojectImageTo3D(d, C.Q_CALC, buf, True)
    assert out is buf
    assert_same(buf, _oracle_grid(37, 53, "s16", "calc", True))


def test_refusals_leave_the_engine_usable():
    import torch

    d = C.grid_map(37, 53, "s16")
    want = _oracle_grid(37, 53, "s16", "calc", True)

    def still_right():
        assert_same(sm.reprojectImageTo3D(d, C.Q_CALC, handleMissingValues=True), want)

    for ddepth in (6, 3, 0):  # CV_64F, CV_16S, CV_8U
        with pytest.raises(_lib.SmError, match="ddepth=CV_32F") as e:
            sm.reprojectImageTo3D(d, C.Q_CALC, ddepth=ddepth)
        assert e.value.code == _lib.SM_E_UNSUPPORTED
        still_right()
    for dt in (np.uint8, np.int32, np.float64):
        with pytest.raises(ValueError, match="2-D int16 or float32 array"):
            sm.reprojectImageTo3D(d.astype(dt), C.Q_CALC)
        still_right()
    with pytest.raises(ValueError, match="2-D int16 or float32 array"):
        sm.reprojectImageTo3D(np.stack([d, d]), C.Q_CALC)
    still_right()
    try:
        for t in (torch.from_numpy(np.stack([d, d])).cuda(), torch.from_numpy(d.astype(np.int32)).cuda(),
                  torch.from_numpy(d.astype(np.float64)).cuda(), torch.from_numpy(d.astype(np.uint8)).cuda()):
            with pytest.raises(ValueError, match="2-D int16 or float32 tensor"):
                sm.reprojectImageTo3D(t, C.Q_CALC)
        got = sm.reprojectImageTo3D(torch.from_numpy(d.copy()).cuda(), C.Q_CALC, handleMissingValues=True)
        assert_same(got.cpu().numpy(), want)
    finally:
        _lib.engine(0).set_stream(None)
    for Q in (np.eye(3), np.zeros(15), np.zeros((4, 5))):
        with pytest.raises(ValueError, match="reshape"):
            sm.reprojectImageTo3D(d, Q)
        still_right()
    # the engine's own entry refuses what the wrapper would have
    with pytest.raises(ValueError, match="2-D int16 or float32 array"):
        _lib.engine(0).reproject(d.astype(np.uint8), C.Q_CALC)
    still_right()


@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_project_points_3d_divides_by_16(kind):
    """stereo_vision.project_points_3D divides by 16 whatever the dtype (its identity test is
    always true) and takes Q as float32."""
    d = C.grid_map(37, 53, kind)
    q32 = C.Q_DENSE.astype(np.float32)
    want = reproject_np.reproject_image_to_3d(d.astype(np.float32) / np.float32(16), q32)
    assert_same(sm.project_points_3D(d, C.Q_DENSE), want)
    assert not np.array_equal(want, reproject_np.reproject_image_to_3d(d.astype(np.float32) / np.float32(16), C.Q_DENSE))


def test_q_as_float32_and_as_a_flat_list():
    d = C.grid_map(37, 53, "f32", "dense")
    q32 = C.Q_DENSE.astype(np.float32)
    want32 = reproject_np.reproject_image_to_3d(d, q32, True)
    assert_same(sm.reprojectImageTo3D(d, q32, handleMissingValues=True), want32)
    assert_same(sm.reprojectImageTo3D(d, [float(v) for v in C.Q_DENSE.reshape(-1)], handleMissingValues=True),
                _oracle_grid(37, 53, "f32", "dense", True))
    assert not np.array_equal(want32, _oracle_grid(37, 53, "f32", "dense", True))
