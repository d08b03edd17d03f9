"""GPU: masked point-cloud extraction and the ASCII PLY formatter (sm_cloud.hpp;
stereo_match_amd/pointcloud.py).  The expected values come from numpy alone:
oracle.reproject_np.reproject_image_to_3d(d, Q, hm)[mask], img[..., ::-1][mask], sma.write_ply
(np.savetxt).  Vertices are compared bit for bit (NaNs position for position: the sign of a NaN that
0 * inf makes is the processor's own)."""
import functools
import io

import numpy as np
import pytest

import reproject_cases as C
import stereo_match_amd as sma
from oracle import reproject_np
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

# Q of disparity_calculation.py:293-298, and one whose principal point is x = 1 and whose X overflows
# float32 alone: d = 0 at x = 1 makes 0 * inf = NaN beside the +-inf of the other columns, and a
# small d > 0 makes X = inf with Y and Z finite
Q_CALC = np.float32([[1, 0, 0, -640], [0, -1, 0, 360], [0, 0, 0, -1164], [0, 0, 1, 0]])
Q_IN = np.float32([[1e38, 0, 0, -1e38], [0, -1, 0, 7], [0, 0, 0, -50], [0, 0, 1, 0]])

# k_cloud_count / k_ply_len make one total per 256 pixels / rows and k_scan_totals takes 1024
# totals a step: 520 x 510 = 265 200 pixels are 1036 totals, so the scan carries its running sum
# from one step into the next
BIG = (520, 510)
SHAPES = [(1, 1), (1, 3), (3, 1), (37, 53), (130, 150), BIG]


def savetxt_body(verts, colors) -> bytes:
    f = io.BytesIO()
    np.savetxt(f, np.hstack([verts, colors]), fmt='%f %f %f %d %d %d ')
    return f.getvalue()


@functools.lru_cache(maxsize=None)
def _map(H, W, kind):
    """Values (i * 37 % 97) * 4 - 16 in [-16, 368] (every value about equally often, neighbours far
    apart), every fifth pixel the invalid -16 (so that `d > d.min()` passes 4 in 5); the float32
    map is that / 16 with the two bounds of the float 'both' mask, as float32, put in: 15.7 rounds
    DOWN to float32, so `d < 15.7` differs between a float32 and a float64 comparison there."""
    i = np.arange(H * W, dtype=np.int64).reshape(H, W)
    d = ((i * 37 % 97) * 4 - 16).astype(np.int16)
    d[i % 5 == 0] = -16
    if kind == "f32":
        d = d.astype(np.float32) / np.float32(16.0)
        if d.size > 8:
            d.flat[5], d.flat[6], d.flat[7] = np.float32(15.7), np.float32(3.75), np.float32(3.3)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _image(H, W, seed=5):
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def numpy_mask(d, lo, hi):
    """The mask as the scripts write it, numpy's own comparison with Python scalars.  `d.min()` of
    a map with a NaN pixel is NaN and passes nothing: rule 2 of oracle/reproject_np.py."""
    m = np.ones(d.shape, bool)
    if isinstance(lo, str):
        m &= d > d.min()
    elif lo is not None:
        m &= d > lo
    if hi is not None:
        m &= d < hi
    return m


def expected(d, Q, img, lo, hi, hm=False, zero=False):
    m = numpy_mask(d, lo, hi)
    pts = reproject_np.reproject_image_to_3d(d, Q, hm)[m]
    if zero:
        pts[~np.isfinite(pts)] = 0
    return pts, img[..., ::-1][m], m


def assert_verts_equal(got, want):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn)
    assert np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])


def assert_cloud(got, pts, rgb):
    assert_verts_equal(got[0], pts)
    assert got[1].dtype == np.uint8 and np.array_equal(got[1], rgb)


def assert_fraction(m):
    """A range mask that passes nearly nothing or nearly everything would test nothing."""
    f = m.mean()
    assert 0.05 <= f <= 0.95, f"the mask passes {f:.3f} of the pixels"


# ---- shapes
@pytest.mark.parametrize("kind", ["s16", "f32"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_no_mask(H, W, kind):
    d, img = _map(H, W, kind), _image(H, W)
    pts, rgb, m = expected(d, Q_CALC, img, None, None)
    assert m.all()
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img), pts, rgb)


@pytest.mark.parametrize("kind,lo,hi", [("s16", 60, 252), ("f32", 3.75, 15.7)])
@pytest.mark.parametrize("H,W", SHAPES[1:])
def test_shapes_both_bounds(H, W, kind, lo, hi):
    """1x3 and 3x1: the values are -16, 132, 280 (-1, 8.25, 17.5): one of three passes."""
    d, img = _map(H, W, kind), _image(H, W)
    pts, rgb, m = expected(d, Q_CALC, img, lo, hi)
    assert_fraction(m)
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img, lo, hi), pts, rgb)


# ---- masks, at 37 x 53 and 130 x 150.  60 and 252 (3.75 and 15.7) are values of the map: strict.
RANGES = [(60, None), (None, 252), (60, 252), (60.5, 251.5), ("min", None), ("min", 252), (-1e30, 1e30)]
RANGES_F = [(3.75, None), (None, 15.7), (3.75, 15.7), (3.3, 15.7), ("min", None), ("min", 15.7),
            (float("-inf"), 15.7)]


@pytest.mark.parametrize("hm", [False, True])
@pytest.mark.parametrize("kind,lo,hi", [("s16", *r) for r in RANGES] + [("f32", *r) for r in RANGES_F])
@pytest.mark.parametrize("H,W", [(37, 53), (130, 150)])
def test_range_masks(H, W, kind, lo, hi, hm):
    d, img = _map(H, W, kind), _image(H, W)
    assert not np.isnan(d.astype(np.float64)).any()
    pts, rgb, m = expected(d, Q_CALC, img, lo, hi, hm)
    if (lo, hi) != (-1e30, 1e30):
        assert_fraction(m)
    else:
        assert m.all()
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img, lo, hi, handleMissingValues=hm), pts, rgb)


def test_float32_bound_is_rounded_like_numpy():
    """np.float32(15.7) < 15.7 as numbers, but numpy >= 2 rounds the Python scalar to float32 first:
    the pixel does not pass.  For an int16 map 251.5 stays 251.5."""
    d = _map(37, 53, "f32")
    assert d.flat[5] == np.float32(15.7) and float(d.flat[5]) < 15.7 and not (d < 15.7).flat[5]
    img = _image(37, 53)
    pts, rgb, m = expected(d, Q_CALC, img, None, 15.7)
    assert not m.flat[5]
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img, None, 15.7), pts, rgb)


def _special_map(which, H, W, kind):
    d = np.zeros((H, W), np.int16)
    if which == "first":
        d[0, 0] = 100
    elif which == "last":
        d[-1, -1] = 100
    elif which == "checker":
        yy, xx = np.mgrid[:H, :W]
        d[(yy + xx) % 2 == 1] = 100
    return d if kind == "s16" else d.astype(np.float32)


@pytest.mark.parametrize("kind", ["s16", "f32"])
@pytest.mark.parametrize("which,count", [("none", 0), ("first", 1), ("last", 1), ("checker", None)])
@pytest.mark.parametrize("H,W", [(37, 53), (130, 150)])
def test_special_masks(H, W, which, count, kind):
    d, img = _special_map(which, H, W, kind), _image(H, W)
    pts, rgb, m = expected(d, Q_CALC, img, 50, None)
    if count is None:
        assert_fraction(m)
    else:
        assert m.sum() == count
    got = sma.extract_point_cloud(d, Q_CALC, img, 50)
    assert got[0].shape == (m.sum(), 3) and got[1].shape == (m.sum(), 3)
    assert_cloud(got, pts, rgb)


@pytest.mark.parametrize("lo,hi", [(3.75, None), (None, 15.7), (3.75, 15.7), (None, None)])
def test_float_map_with_nan_pixels(lo, hi):
    d = _map(130, 150, "f32").copy()
    d[::7, ::3] = np.nan
    d[129, 149] = np.nan
    img = _image(130, 150)
    pts, rgb, m = expected(d, Q_CALC, img, lo, hi)
    nan = np.isnan(d)
    if lo is None and hi is None:
        assert m.all() and np.isnan(pts).any()  # without a bound the NaN pixels are points (of NaNs)
    else:
        assert_fraction(m)
        assert not m[nan].any()
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img, lo, hi), pts, rgb)


# ---- NaN pixels where a minimum is taken (the two rules of oracle/reproject_np.py).
# Neither may depend on the NaNs' sign or payload.
@functools.lru_cache(maxsize=None)
def _nan_map(sign, H=130, W=150, payloads=C.NAN_PAYLOADS):
    """_map's float32 map (minimum -1) with the float32 successor of the minimum at pixel 1 -- above
    the minimum, inside the FLT_EPSILON window -- and NaNs of one sign: the first pixel, the
    last, and every 23rd (lanes of every kind), their payloads cycling through `payloads`."""
    d = _map(H, W, "f32").copy()
    d.flat[1] = np.nextafter(np.float32(-1), np.float32(0))
    if sign:
        C.put_nans(d, [0, H * W - 1] + list(range(40, H * W, 23)), sign, payloads)
    d.setflags(write=False)
    return d


def _empty_header():
    return (sma.reproject.PLY_HEADER % dict(vert_num=0)).encode()


@pytest.mark.parametrize("hi", [None, 15.7])
@pytest.mark.parametrize("payloads", [C.NAN_PAYLOADS, C.QUIET_ONLY], ids=["payloads", "np.nan"])
@pytest.mark.parametrize("sign", [+1, -1])
def test_nan_map_lo_min_is_an_empty_cloud(sign, payloads, hi, tmp_path):
    """Rule 2: `d > d.min()` with a NaN pixel is `d > NaN`, for np.nan itself (0x7FC00000), its
    negative and every other payload."""
    import torch

    d, img = _nan_map(sign, payloads=payloads), _image(130, 150)
    pts, rgb, m = expected(d, Q_CALC, img, "min", hi)
    assert np.isnan(d.min()) and not m.any()
    got = sma.extract_point_cloud(d, Q_CALC, img, "min", hi)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    assert_cloud(got, pts, rgb)
    v, c = sma.extract_point_cloud(torch.from_numpy(d.copy()).cuda(), Q_CALC, torch.from_numpy(img.copy()).cuda(), "min", hi)
    assert v.shape == (0, 3) and c.shape == (0, 3)
    assert sma.write_point_cloud(str(tmp_path / "a.ply"), d, Q_CALC, img, "min", hi) == 0
    assert (tmp_path / "a.ply").read_bytes() == _empty_header()
    n = sma.write_point_cloud(str(tmp_path / "b.ply"), torch.from_numpy(d.copy()).cuda(), Q_CALC,
                              torch.from_numpy(img.copy()).cuda(), "min", hi)
    assert n == 0 and (tmp_path / "b.ply").read_bytes() == _empty_header()


@pytest.mark.parametrize("lo,hi", [(-1.5, None), (-1.5, 15.7), (None, 15.7), (None, None)])
def test_nan_map_handle_missing_follows_rule_1(lo, hi):
    """Rule 1, vertex for vertex: the NaNs take no part in the minimum, so the pixels at -1 and its
    successor get Z = 10000, whatever the NaNs' sign."""
    img = _image(130, 150)
    got = []
    for sign in (+1, -1):
        d = _nan_map(sign)
        pts, rgb, m = expected(d, Q_CALC, img, lo, hi, hm=True)
        n_marked = int((pts[:, 2] == 10000).sum())
        assert n_marked == int((d <= d.flat[1]).sum()) > 100 and (pts[:, 2] != 10000).any()
        if lo is None and hi is None:
            assert m.all() and np.isnan(pts).any()
        else:
            assert 0.05 <= m.mean() < 1 and not m[np.isnan(d)].any()
        got.append(sma.extract_point_cloud(d, Q_CALC, img, lo, hi, handleMissingValues=True))
        assert_cloud(got[-1], pts, rgb)
    assert_verts_equal(got[0][0], got[1][0])


@pytest.mark.parametrize("sign", [0, +1, -1])
def test_lo_min_with_handle_missing(sign):
    """Both at once need both facts of a map: rule 1's minimum for the 10000s and numpy's `d.min()`
    for the mask.  NaN-free (sign 0): the minimum's pixels fail `d > min`, its successor passes
    and is marked.  With NaNs: empty."""
    import torch

    d, img = _nan_map(sign), _image(130, 150)
    pts, rgb, m = expected(d, Q_CALC, img, "min", None, hm=True)
    if sign:
        assert not m.any()
    else:
        assert_fraction(m)
        assert (pts[:, 2] == 10000).sum() == 1 and m.flat[1]
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img, "min", handleMissingValues=True), pts, rgb)
    v, c = sma.extract_point_cloud(torch.from_numpy(d.copy()).cuda(), Q_CALC, torch.from_numpy(img.copy()).cuda(), "min",
                                   handleMissingValues=True)
    assert_cloud((v.cpu().numpy(), c.cpu().numpy()), pts, rgb)


@pytest.mark.parametrize("hm", [False, True])
@pytest.mark.parametrize("sign", [+1, -1])
def test_batch_device_only_one_map_has_a_nan(sign, hm):
    """lo = "min" on the batch entry point: map 1's cloud is empty, its neighbours' are not, and
    every map keeps its own minimum (-1, -1 with np.nan or its negative, 2.5)."""
    import torch

    H, W = 37, 53
    maps = np.stack([_nan_map(0, H, W), _nan_map(sign, H, W, C.QUIET_ONLY), np.maximum(_map(H, W, "f32"), np.float32(2.5))])
    imgs = np.stack([_image(H, W, 30 + i) for i in range(3)])
    exp = [expected(maps[i], Q_CALC, imgs[i], "min", None, hm=hm) for i in range(3)]
    want_counts = [int(e[2].sum()) for e in exp]
    assert want_counts[1] == 0 and want_counts[0] > 0 and want_counts[2] > 0 and want_counts[0] != want_counts[2]
    if hm:
        assert (exp[0][0][:, 2] == 10000).sum() == 1 and not (exp[2][0][:, 2] == 10000).any()
    v, c, counts = sma.extract_point_cloud(torch.from_numpy(maps).cuda(), Q_CALC, torch.from_numpy(imgs).cuda(), "min",
                                           handleMissingValues=hm)
    assert counts.tolist() == want_counts
    assert_cloud((v.cpu().numpy(), c.cpu().numpy()), np.concatenate([e[0] for e in exp]),
                 np.concatenate([e[1] for e in exp]))
    # a numeric bound with handleMissingValues: map 1 follows rule 1 beside its neighbours
    exp = [expected(maps[i], Q_CALC, imgs[i], -1.5, None, hm=True) for i in range(3)]
    assert all((e[0][:, 2] == 10000).any() for e in exp)
    v, c, counts = sma.extract_point_cloud(torch.from_numpy(maps).cuda(), Q_CALC, torch.from_numpy(imgs).cuda(), -1.5,
                                           handleMissingValues=True)
    assert counts.tolist() == [int(e[2].sum()) for e in exp]
    assert_cloud((v.cpu().numpy(), c.cpu().numpy()), np.concatenate([e[0] for e in exp]),
                 np.concatenate([e[1] for e in exp]))


# ---- zero_nonfinite, strides
@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_zero_nonfinite_is_per_component(kind):
    d = _map(37, 53, kind).copy()
    d[:, 1] = 0  # x = 1 is Q_IN's principal point: X = 0 * inf
    d[::3, ::4] = 0
    img = _image(37, 53)
    raw, _, m = expected(d, Q_IN, img, -0.5, None)
    assert np.isnan(raw).any() and np.isposinf(raw).any() and np.isneginf(raw).any()
    rows = ~np.isfinite(raw).all(1)
    assert np.isfinite(raw[rows]).any()  # rows that are only partly non-finite: per component
    assert_fraction(m)
    pts, rgb, _ = expected(d, Q_IN, img, -0.5, None, zero=True)
    assert np.isfinite(pts).all()
    assert_cloud(sma.extract_point_cloud(d, Q_IN, img, -0.5, zero_nonfinite=True), pts, rgb)
    assert_cloud(sma.extract_point_cloud(d, Q_IN, img, -0.5), raw, rgb)


def test_strided_bgr_image():
    import torch

    H, W = 37, 53
    big = np.random.default_rng(9).integers(0, 256, (H, W + 5, 3), dtype=np.uint8)
    img = big[:, 2:2 + W]
    assert img.strides[0] == 3 * (W + 5) and not img.flags.c_contiguous
    d = _map(H, W, "s16")
    pts, rgb, m = expected(d, Q_CALC, img, 60, 252)
    assert_fraction(m)
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img, 60, 252), pts, rgb)
    tb = torch.from_numpy(big).cuda()
    v, c = sma.extract_point_cloud(torch.from_numpy(d.copy()).cuda(), Q_CALC, tb[:, 2:2 + W], 60, 252)
    assert v.is_cuda and c.is_cuda
    assert_cloud((v.cpu().numpy(), c.cpu().numpy()), pts, rgb)
    # reversed channels: not readable in place, packed first
    assert_cloud(sma.extract_point_cloud(d, Q_CALC, img[..., ::-1], 60, 252), pts, rgb[:, ::-1])


# ---- batch-device form
@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_batch_device_three_maps(kind):
    import torch

    H, W = 37, 53
    base = _map(H, W, kind)
    maps = np.stack([base, np.full_like(base, -1), np.roll(base, 11, 1)[::-1].copy()])
    maps[2, :5] = -1
    imgs = np.stack([_image(H, W, 20 + i) for i in range(3)])
    lo = 60 if kind == "s16" else 3.75
    exp = [expected(maps[i], Q_CALC, imgs[i], lo, None, hm=True) for i in range(3)]
    want_counts = [int(e[2].sum()) for e in exp]
    assert want_counts[1] == 0 and want_counts[0] != want_counts[2] and min(want_counts[0], want_counts[2]) > 0
    v, c, counts = sma.extract_point_cloud(torch.from_numpy(maps).cuda(), Q_CALC, torch.from_numpy(imgs).cuda(), lo,
                                           handleMissingValues=True)
    assert counts.tolist() == want_counts and v.shape[0] == sum(want_counts)
    assert_cloud((v.cpu().numpy(), c.cpu().numpy()), np.concatenate([e[0] for e in exp]),
                 np.concatenate([e[1] for e in exp]))
    # lo = "min" is every map's own minimum
    exp = [expected(maps[i], Q_CALC, imgs[i], "min", None) for i in range(3)]
    v, c, counts = sma.extract_point_cloud(torch.from_numpy(maps).cuda(), Q_CALC, torch.from_numpy(imgs).cuda(), "min")
    assert counts.tolist() == [int(e[2].sum()) for e in exp] and counts[1] == 0
    assert_cloud((v.cpu().numpy(), c.cpu().numpy()), np.concatenate([e[0] for e in exp]),
                 np.concatenate([e[1] for e in exp]))


def test_device_capacity_is_never_exceeded():
    """sm_cloud_extract_batch_device with room for fewer rows than pass: the counts are the true
    ones and nothing is written behind the capacity."""
    import torch

    H, W = 37, 53
    d, img = _map(H, W, "s16"), _image(H, W)
    pts, rgb, m = expected(d, Q_CALC, img, 60, None)
    n, cap = int(m.sum()), int(m.sum()) // 2
    eng = _lib.engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    td, ti = torch.from_numpy(d.copy()).cuda(), torch.from_numpy(img.copy()).cuda()
    v = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")
    c = torch.full((n, 3), 77, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    prm = _lib.SmCloudParams(lo=60.0, lo_mode=_lib.SM_CLOUD_LO_VALUE)
    eng.cloud_extract_batch_device(td.data_ptr(), 0, ti.data_ptr(), 0, 3 * W, 1, H, W, Q_CALC, prm, cap, v.data_ptr(),
                                   c.data_ptr(), counts.data_ptr())
    assert int(counts.cpu()[0]) == n
    v, c = v.cpu().numpy(), c.cpu().numpy()
    assert_cloud((v[:cap], c[:cap]), pts[:cap], rgb[:cap])
    assert (v[cap:] == -7.0).all() and (c[cap:] == 77).all()
    # the PLY body likewise: rows that would end behind the capacity are left out
    body = savetxt_body(pts, rgb)
    capb = len(body) // 2
    out = torch.full((len(body),), 0xAB, dtype=torch.uint8, device="cuda")
    nb = torch.zeros(1, dtype=torch.int64, device="cuda")
    tv, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
    eng.ply_format_device(tv.data_ptr(), tc.data_ptr(), n, capb, out.data_ptr(), nb.data_ptr())
    assert int(nb.cpu()[0]) == len(body)
    out = out.cpu().numpy().tobytes()
    whole = body[:capb].rfind(b"\n") + 1
    assert out[:whole] == body[:whole] and out[whole:] == b"\xAB" * (len(body) - whole)
    eng.set_stream(None)


# ---- device formatter
def _special_rows():
    from test_ply_format_host import rows_of, special_values

    return rows_of(special_values())


def test_device_formatter_special_values():
    import torch

    v, c = _special_rows()
    got = sma.format_ply(torch.from_numpy(v).cuda(), torch.from_numpy(c).cuda())
    assert got.is_cuda and got.dtype == torch.uint8
    assert got.cpu().numpy().tobytes() == savetxt_body(v, c) == sma.format_ply(v, c)
    e = sma.format_ply(torch.empty((0, 3), dtype=torch.float32, device="cuda"),
                       torch.empty((0, 3), dtype=torch.uint8, device="cuda"))
    assert e.numel() == 0


def test_device_formatter_random_bit_patterns():
    """300 000 rows (900 000 bit patterns; 1172 block totals, more than one step of the scan) against
    the host formatter's bytes, and a 20 000-row subset against np.savetxt."""
    import torch

    rng = np.random.default_rng(31)
    v = rng.integers(0, 1 << 32, (300_000, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    c = rng.integers(0, 256, (300_000, 3), dtype=np.uint8)
    got = sma.format_ply(torch.from_numpy(v).cuda(), torch.from_numpy(c).cuda()).cpu().numpy().tobytes()
    assert got == sma.format_ply(v, c)
    sub = slice(140_000, 160_000)
    got = sma.format_ply(torch.from_numpy(v[sub]).cuda(), torch.from_numpy(c[sub]).cuda()).cpu().numpy().tobytes()
    assert got == savetxt_body(v[sub], c[sub])


@pytest.mark.parametrize("stage", [1, -1])
def test_both_write_passes_give_the_same_bytes(stage):
    """SM_TUNE_PLY_STAGE 1 (the default: a block's rows staged in LDS, 16-byte stores) and -1 (every
    row straight to global memory): every alignment of the
    output, blocks of one and two rows, and a capacity that cuts a block (row-by-row fallback)."""
    import torch

    rng = np.random.default_rng(32)
    v = rng.integers(0, 1 << 32, (5000, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    v[:256] = -np.finfo(np.float32).max  # a block of the longest rows: all of the LDS tile
    c = rng.integers(0, 256, (5000, 3), dtype=np.uint8)
    c[:256] = 255
    want = sma.format_ply(v, c)
    tv, tc = torch.from_numpy(v).cuda(), torch.from_numpy(c).cuda()
    eng = _lib.engine(0)
    eng.set_tuning(eng.TUNE_PLY_STAGE, stage)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        for k in range(17):
            out = torch.full((len(want) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
            eng.ply_format_device(tv.data_ptr(), tc.data_ptr(), len(v), len(want), out.data_ptr() + k, 0)
            got = out.cpu().numpy().tobytes()
            assert got[:k] == b"\xAB" * k and got[k:k + len(want)] == want and got[k + len(want):] == b"\xAB" * (64 - k)
        for n in (1, 2):
            out = torch.full((256,), 0xAB, dtype=torch.uint8, device="cuda")
            w = sma.format_ply(np.zeros((n, 3), np.float32), c[300:300 + n])
            z = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            eng.ply_format_device(z.data_ptr(), tc.data_ptr() + 900, n, len(w), out.data_ptr() + 3, 0)
            assert out.cpu().numpy().tobytes()[3:3 + len(w)] == w
        cap = len(want) // 2
        out = torch.full((len(want),), 0xAB, dtype=torch.uint8, device="cuda")
        eng.ply_format_device(tv.data_ptr(), tc.data_ptr(), len(v), cap, out.data_ptr(), 0)
        got = out.cpu().numpy().tobytes()
        whole = want[:cap].rfind(b"\n") + 1
        assert got[:whole] == want[:whole] and got[whole:] == b"\xAB" * (len(want) - whole)
        assert sma.format_ply(tv, tc).cpu().numpy().tobytes() == want
    finally:
        eng.set_tuning(eng.TUNE_PLY_STAGE, 0)
        eng.set_stream(None)


# ---- the three script tails, on a synthetic 96 x 160 map with invalid pixels at -16
def _tail_case(name):
    H, W = 96, 160
    rng = np.random.default_rng(41)
    d16 = rng.integers(0, 40, (H, W)).astype(np.int16)
    d16[rng.random((H, W)) < 0.1] = -16
    d16[5, 7] = 0
    img = _image(H, W, 43)
    if name == "disparity_calculation":  # :293-320: the raw int16 x16 map, 10 < disp < 20, non-finite zeroed
        return d16, Q_CALC, img, 10, 20, True
    d = d16.astype(np.float32) * 8 / np.float32(16.0)
    if name == "disparity_test":  # :225-265: float32 / 16, Tx = -22, disp > 2, non-finite zeroed
        Q = np.float32([[1, 0, 0, -360], [0, -1, 0, 640], [0, 0, 0, -1164], [0, 0, -1 / -22, 0]])
        return d, Q, img, 2, None, True
    # try_try.py:80-96: f = 0.8 w, disp > disp.min(), nothing zeroed
    Q = np.float32([[1, 0, 0, -0.5 * W], [0, -1, 0, 0.5 * H], [0, 0, 0, -0.8 * W], [0, 0, 1, 0]])
    return d, Q, img, "min", None, False


@pytest.mark.parametrize("name", ["disparity_calculation", "disparity_test", "try_try"])
def test_script_tails_write_the_same_file(name, tmp_path):
    import torch

    d, Q, img, lo, hi, zero = _tail_case(name)
    # the script's tail, line for line
    points = reproject_np.reproject_image_to_3d(d, Q)
    colors = img[..., ::-1]
    mask = numpy_mask(d, lo, hi)
    assert_fraction(mask)
    out_points, out_colors = points[mask], colors[mask]
    if name == "try_try":
        assert not np.isfinite(out_points).all()  # the d = 0 pixel stays in, as inf
    if zero:
        out_points[np.isnan(out_points)] = 0
        out_points[np.isinf(out_points)] = 0
    sma.write_ply(str(tmp_path / "ref.ply"), out_points, out_colors)
    want = (tmp_path / "ref.ply").read_bytes()
    n = sma.write_point_cloud(str(tmp_path / "a.ply"), d, Q, img, lo, hi, zero_nonfinite=zero)
    assert n == int(mask.sum())
    assert (tmp_path / "a.ply").read_bytes() == want
    n = sma.write_point_cloud(str(tmp_path / "b.ply"), torch.from_numpy(d).cuda(), Q, torch.from_numpy(img.copy()).cuda(),
                              lo, hi, zero_nonfinite=zero)
    assert n == int(mask.sum())
    assert (tmp_path / "b.ply").read_bytes() == want


def test_write_point_cloud_big_and_empty(tmp_path):
    """The scan of the byte totals over more than one step (265 200 rows), and N = 0."""
    H, W = BIG
    d, img = _map(H, W, "s16"), _image(H, W)
    pts, rgb, _ = expected(d, Q_CALC, img, None, None)
    n = sma.write_point_cloud(str(tmp_path / "big.ply"), d, Q_CALC, img)
    assert n == H * W
    got = (tmp_path / "big.ply").read_bytes()
    head = (sma.reproject.PLY_HEADER % dict(vert_num=n)).encode()
    assert got[:len(head)] == head and got[len(head):] == sma.format_ply(pts, np.ascontiguousarray(rgb))
    n = sma.write_point_cloud(str(tmp_path / "none.ply"), d, Q_CALC, img, 1000)
    assert n == 0 and (tmp_path / "none.ply").read_bytes() == (sma.reproject.PLY_HEADER % dict(vert_num=0)).encode()


# ---- matcher -> extraction -> formatter without a host copy in between
def test_on_device_chain(tmp_path):
    import torch

    H, W, D = 64, 128, 16
    left, right, _ = synthetic.random_dot_pair(H, W, D, seed=3)
    bgr = np.stack([left, right, 255 - left], -1)
    m = sma.StereoSGBM_create(numDisparities=D, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
                              preFilterCap=63)
    t = m.compute(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda())
    assert t.is_cuda and t.dtype == torch.int16
    v, c = sma.extract_point_cloud(t, Q_CALC, torch.from_numpy(bgr).cuda(), 0, zero_nonfinite=True)
    body = sma.format_ply(v, c)
    assert v.is_cuda and c.is_cuda and body.is_cuda
    # the host path of the parent commit
    d = m.compute(left, right)
    mask = d > 0
    assert_fraction(mask)
    pts = sma.reprojectImageTo3D(d, Q_CALC)[mask]
    pts[~np.isfinite(pts)] = 0
    sma.write_ply(str(tmp_path / "h.ply"), pts, bgr[..., ::-1][mask])
    want = (tmp_path / "h.ply").read_bytes()
    head = (sma.reproject.PLY_HEADER % dict(vert_num=int(mask.sum()))).encode()
    assert head + body.cpu().numpy().tobytes() == want


# ---- argument errors
def test_argument_errors():
    import torch

    d, img = _map(37, 53, "s16"), _image(37, 53)
    with pytest.raises(ValueError, match="shape"):
        sma.extract_point_cloud(d, Q_CALC, _image(37, 54))
    with pytest.raises(ValueError, match="shape"):
        sma.extract_point_cloud(torch.from_numpy(d.copy()).cuda(), Q_CALC, torch.from_numpy(_image(36, 53).copy()).cuda())
    with pytest.raises(ValueError, match="int16 or float32"):
        sma.extract_point_cloud(d.astype(np.float64), Q_CALC, img)
    with pytest.raises(ValueError, match="int16 or float32"):
        sma.extract_point_cloud(torch.from_numpy(d.astype(np.int32)).cuda(), Q_CALC, torch.from_numpy(img.copy()).cuda())
    with pytest.raises(ValueError, match="uint8"):
        sma.extract_point_cloud(d, Q_CALC, img.astype(np.int16))
    with pytest.raises(ValueError, match="uint8"):
        sma.extract_point_cloud(d, Q_CALC, img[..., 0])
    for kw in (dict(lo=float("nan")), dict(hi=float("nan")), dict(lo=1, hi=np.float32("nan"))):
        with pytest.raises(ValueError, match="NaN"):
            sma.extract_point_cloud(d, Q_CALC, img, **kw)
        with pytest.raises(ValueError, match="NaN"):
            sma.write_point_cloud("unused.ply", d, Q_CALC, img, **kw)
    with pytest.raises(ValueError, match="'min'"):
        sma.extract_point_cloud(d, Q_CALC, img, "max")
    # the C-ABI refuses a NaN bound itself
    eng = _lib.engine(0)
    prm = _lib.SmCloudParams(hi=float("nan"), has_hi=1)
    with pytest.raises(ValueError, match="NaN"):
        eng.cloud_extract(d, 0, img, Q_CALC, prm)
    v = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    c = torch.zeros((4, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="write_ply"):
        sma.format_ply(v, c)
    with pytest.raises(ValueError, match="write_ply"):
        sma.format_ply(v.float(), c.int())
    with pytest.raises(ValueError):
        sma.format_ply(v.float(), c.cpu().numpy())
