"""The PNG encoder on the device (k_png_filter, k_png_deflate, k_png_assemble, k_png_scatter): its
bytes against the CPU twin's, byte for byte, and through the validator of tests/png_np.py."""
import ctypes

import numpy as np
import pytest

import png_np
import stereo_match_amd as sma
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

SEG = png_np.SEG


def same_as_host(img, px=None, validate=True, **opts):
    """Device bytes == host-twin bytes; the device bytes through the validator."""
    dev = sma.imencode_png(img, **opts)
    host = sma.imencode_png_host(img, **opts)
    if dev != host:
        a, b = np.frombuffer(dev, np.uint8), np.frombuffer(host, np.uint8)
        n = min(len(a), len(b))
        d = np.flatnonzero(a[:n] != b[:n])
        raise AssertionError(f"device file ({len(a)} bytes) != host file ({len(b)} bytes), first difference at byte "
                             f"{int(d[0]) if len(d) else n}")
    if validate:
        px = png_np.pixels_of(img, keep_channel_order=opts.get("keep_channel_order", False)) if px is None else px
        png_np.validate(dev, px, -1 if opts.get("filter") is None else opts["filter"])
    return dev


@pytest.mark.parametrize("name,kind,H,W", png_np.SHAPES, ids=[f"{s[0]}-{s[1]}" for s in png_np.SHAPES])
def test_shapes(name, kind, H, W):
    for random in (False, True):
        same_as_host(png_np.shape_image(kind, H, W, seed=H * 131 + W, random=random))


def test_keep_channel_order_and_fixed_filters():
    img = png_np.shape_image("bgr", 37, 67, seed=5)
    same_as_host(img, keep_channel_order=True)
    for kind in ("gray", "bgr", "u16"):
        for f in range(5):
            same_as_host(png_np.shape_image(kind, 37, 67, seed=9), filter=f)


def test_filter_ties():
    same_as_host(np.full((1, 50), 90, np.uint8))
    same_as_host(np.zeros((3, 20), np.uint8))
    row = png_np.shape_image("gray", 1, 40, seed=8, random=True)
    same_as_host(np.vstack([row, row]))


@pytest.mark.parametrize("R", [2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 519])
def test_repeat_block(R):
    same_as_host(png_np.repeat_blocks([R, 5, R, 1, R]), filter=0)
    same_as_host(png_np.repeat_blocks([R]), filter=0)


def test_runs_and_segments():
    same_as_host(png_np.repeat_blocks([2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 519] * 3, seed=3), filter=0)
    same_as_host(png_np.one_row(np.full(40000, 7)), filter=0)  # a run across the segment boundary
    for k in (SEG - 2, SEG - 1, SEG, SEG + 1):
        same_as_host(png_np.one_row(np.concatenate([np.full(k - 1, 9), np.full(3000, 200)])), filter=0)
    same_as_host(png_np.one_row(np.zeros(SEG - 1)), filter=0)  # a segment of one byte value
    # runs that begin, end and continue at the boundaries of the threads' 128 positions
    row = np.zeros(SEG - 1, np.uint8)
    row[126:130] = 5
    row[255:257] = 6
    row[383] = 7
    row[511:1030] = 8
    same_as_host(png_np.one_row(row), filter=0)


def test_no_match_and_length_limit():
    counts = np.maximum(1, (6000 * 0.8 ** np.arange(40)).astype(int))
    counts[0] += SEG - 1 - counts.sum()
    same_as_host(png_np.skewed_no_neighbours(list(counts)), filter=0)  # literals only: zero-length distance code
    img = png_np.skewed_no_neighbours(png_np.deep_tree_counts())  # every Huffman tree deeper than 15
    same_as_host(img, filter=0)
    same_as_host(np.tile(img, (4, 1)), filter=0)
    same_as_host(np.tile(img, (3, 1)))


def test_incompressible_and_constant():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (96, 1021), dtype=np.uint8)
    png = same_as_host(img)
    assert len(png) <= png_np.all_stored_size(96 * 1022) == _lib.load().sm_png_bound(96, 1021, 1, 8)
    png = same_as_host(np.full((16, 8191), 113, np.uint8))
    assert len(png) < 131072 / 100


def test_host_pointer_entry_point_capacity():
    img = png_np.shape_image("bgr", 37, 67, seed=10)
    want = sma.imencode_png_host(img)
    eng = _lib.engine(0)
    prm = _lib.SmPngParams(src_kind=_lib.SM_PNG_SRC_U8, channels=3, filter=-1)
    nb = ctypes.c_uint64()
    buf = np.full(len(want) + 64, 0xAB, np.uint8)
    rc = eng._lib.sm_png_encode(eng.ctx, img.ctypes.data, img.strides[0], 37, 67, ctypes.byref(prm), len(want) - 1,
                                buf.ctypes.data, ctypes.byref(nb))
    assert rc == _lib.SM_E_ARG and nb.value == len(want) and (buf == 0xAB).all()
    rc = eng._lib.sm_png_encode(eng.ctx, img.ctypes.data, img.strides[0], 37, 67, ctypes.byref(prm), len(want),
                                buf.ctypes.data, ctypes.byref(nb))
    assert rc == _lib.SM_OK and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()


@pytest.mark.parametrize("kind", ["gray", "bgr"])
def test_batch_of_three(kind):
    """Every file equals the image's own encoding, d_nbytes is right, and nothing is written past
    capacity_bytes of any slot, neither with room for the files nor without."""
    import torch

    imgs = np.stack([png_np.shape_image(kind, 37, 67, seed=20), png_np.shape_image(kind, 37, 67, seed=21, random=True),
                     np.full_like(png_np.shape_image(kind, 37, 67), 200)])
    singles = [sma.imencode_png_host(x) for x in imgs]
    assert len(set(singles)) == 3
    t = torch.from_numpy(imgs).cuda()
    assert sma.imencode_png_batch(t) == singles
    eng = _lib.engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    prm = _lib.SmPngParams(src_kind=_lib.SM_PNG_SRC_U8, channels=3 if kind == "bgr" else 1, filter=-1)
    row = t.stride(1) * t.element_size()
    for cap in (max(len(s) for s in singles) + 5, min(len(s) for s in singles) - 7, 40):
        out = torch.full((3 * cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        nb = torch.zeros(3, dtype=torch.int64, device="cuda")
        eng.png_encode_batch_device(t.data_ptr(), t.stride(0), row, 3, 37, 67, prm, cap, out.data_ptr(), nb.data_ptr())
        torch.cuda.synchronize()
        assert nb.cpu().tolist() == [len(s) for s in singles]
        o = out.cpu().numpy()
        assert (o[3 * cap:] == 0xAB).all()
        for i, s in enumerate(singles):
            slot = o[i * cap:(i + 1) * cap]
            k = min(cap, len(s))
            assert slot[:k].tobytes() == s[:k]
            assert (slot[k:] == 0xAB).all()
    # sizes only
    nb = torch.zeros(3, dtype=torch.int64, device="cuda")
    eng.png_encode_batch_device(t.data_ptr(), t.stride(0), row, 3, 37, 67, prm, 0, 0, nb.data_ptr())
    torch.cuda.synchronize()
    assert nb.cpu().tolist() == [len(s) for s in singles]


def test_torch_input_on_another_stream():
    import torch

    for kind in ("gray", "bgr", "u16"):
        img = png_np.shape_image(kind, 41, 53, seed=30)
        want = sma.imencode_png(img)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            if kind == "u16":
                t = torch.from_numpy(img.view(np.int16)).cuda().view(torch.uint16)
            else:
                t = torch.from_numpy(img).cuda()
            got = sma.imencode_png(t)
        assert got == want
    # a view with its own row stride is read in place
    big = torch.from_numpy(png_np.shape_image("gray", 41, 80, seed=6)).cuda()
    view = big[:, 3:56]
    assert sma.imencode_png(view) == sma.imencode_png_host(view.cpu().numpy())


def test_imwrite(tmp_path):
    import torch

    img = png_np.shape_image("bgr", 37, 67, seed=31)
    assert sma.imwrite(str(tmp_path / "a.png"), torch.from_numpy(img).cuda()) is True
    assert (tmp_path / "a.png").read_bytes() == sma.imencode_png_host(img)
    png_np.check_pillow((tmp_path / "a.png").read_bytes(), png_np.pixels_of(img))


def test_disparity_conversions_on_the_device():
    d = np.array([[-16, -1, 0, 1, 15, 16, 4095, 4096, 32767, -32768]], np.int16)
    dev = sma.encode_disparity_png(d, "kitti")
    assert dev == sma.encode_disparity_png(d, "kitti", host=True)
    png_np.validate(dev, png_np.pixels_of(d, disp="kitti"))
    f = np.array([[np.nan, np.inf, -np.inf, -0.0, 0.0, 0.00195, 0.001953125, 0.005859375, 255.998, 256.0, 1e30, -3.5, 1.0,
                   0.5 / 256 + 1.0, 1.5 / 256 + 1.0]], np.float32)
    dev = sma.encode_disparity_png(f, "kitti")
    assert dev == sma.encode_disparity_png(f, "kitti", host=True)
    png_np.validate(dev, png_np.pixels_of(f, disp="kitti"))
    t = np.arange(-3, 515, dtype=np.int16).reshape(1, -1)
    dev = sma.encode_disparity_png(t, "u8", 0, 510)
    png_np.validate(dev, png_np.pixels_of(t, disp="u8", lo=0, hi=510))
    flat = np.full((5, 7), 123, np.int16)
    png_np.validate(sma.encode_disparity_png(flat, "u8"), np.zeros((5, 7), np.uint8))


def test_write_disparity_png_of_a_golden_pair(golden_cases, tmp_path):
    """The GPU disparity of sgbm5_d16_settings, from device memory to the two files."""
    import torch

    name, left, right, params, expected, _ = next(c for c in golden_cases if c[0] == "sgbm5_d16_settings")
    eng = _lib.engine(0)
    eng.set_stream(None)
    d = eng.compute(left, right, synthetic.to_sm_params(params))
    assert np.array_equal(d, expected) and (d < 0).any() and (d > 0).any()
    t = torch.from_numpy(d).cuda()
    assert sma.write_disparity_png(str(tmp_path / "k.png"), t, "kitti") is True
    kitti = (tmp_path / "k.png").read_bytes()
    want = np.where(d < 0, 0, d.astype(np.int32) << 4).astype(np.uint16)
    png_np.validate(kitti, want)
    png_np.check_pillow(kitti, want)
    assert kitti == sma.encode_disparity_png(d, "kitti", host=True)
    sma.write_disparity_png(str(tmp_path / "u.png"), t, "u8")  # the map's min and max found on the device
    u8 = (tmp_path / "u.png").read_bytes()
    png_np.validate(u8, png_np.linear_u8(d))
    assert u8 == sma.encode_disparity_png(d, "u8", host=True)
    # the float32 map of the same disparities
    f = torch.from_numpy(d.astype(np.float32) / 16).cuda()
    assert sma.encode_disparity_png(f, "kitti") == kitti


@pytest.mark.slow
def test_full_size_kitti_map():
    rng = np.random.default_rng(40)
    H, W = 375, 1242
    base = (np.linspace(40, 900, W)[None, :] + np.linspace(0, 300, H)[:, None]).astype(np.int16)
    d = (base + rng.integers(-3, 4, (H, W))).astype(np.int16)
    d[rng.random((H, W)) < 0.1] = -16
    dev = sma.encode_disparity_png(d, "kitti")
    assert dev == sma.encode_disparity_png(d, "kitti", host=True)
    png_np.validate(dev, png_np.pixels_of(d, disp="kitti"))


@pytest.mark.slow
def test_full_size_bgr_frame():
    left, _, _ = synthetic.random_dot_pair(720, 1280, 64, seed=2)
    rng = np.random.default_rng(41)
    yy, xx = np.mgrid[0:720, 0:1280]
    img = np.stack([(xx // 5) % 256, (yy // 3) % 256, left], -1).astype(np.uint8)
    img[200:400] += rng.integers(0, 3, (200, 1280, 3)).astype(np.uint8)
    dev = same_as_host(img, validate=False)
    png_np.validate(dev, png_np.pixels_of(img))
