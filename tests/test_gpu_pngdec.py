"""The PNG decoder on the device (sm_pngdec.hpp: k_pngdec_parse, _crc, _inflate, _place, _compact,
_gather, _inflate_serial, _adler, _verify, _unfilter): its pixels, status and inflate path against
the CPU twin's and against the judge (zlib.decompress + png_np.unfilter_stream)."""
import os
import zlib

import numpy as np
import pytest

import png_np
import pngdec_np as P
import stereo_match_amd as sm
from stereo_match_amd import _lib

pytestmark = pytest.mark.gpu

PATHS = {"parallel": (1, 0), "serial": (0, 1)}


def check(png, path=None, flags=(-1,), judge=True):
    """device == host twin == judge, for every flag; the device's path."""
    want = P.judge(png) if judge else None
    for fl in flags:
        host = sm.imdecode_host(png, fl)
        host_path = _lib.png_decode_stats(None)
        dev = sm.imdecode(png, fl)
        assert dev.dtype == host.dtype and dev.shape == host.shape
        assert np.array_equal(dev, host), f"flags {fl}: device != host twin"
        got = _lib.engine(0).png_decode_stats()
        assert got == host_path, (got, host_path)
        if path:
            assert got == PATHS[path], (path, got)
        if judge:
            assert np.array_equal(dev, P.expected(want, fl)), f"flags {fl}: device != judge"


def rejects(png, text):
    with pytest.raises(sm.SmError) as host:
        sm.imdecode_host(png, -1)
    with pytest.raises(sm.SmError) as dev:
        sm.imdecode(png, -1)
    assert text in str(dev.value) and dev.value.code == host.value.code, (str(dev.value), str(host.value))
    assert str(dev.value) == str(host.value)


# ---- unfilter geometry ------------------------------------------------------------------------------
def image(bpp, H, W, seed):
    rng = np.random.default_rng(seed)
    if bpp == 2:
        return png_np.runny(seed, (H, W), np.uint16)
    shape = (H, W) if bpp == 1 else (H, W, bpp)
    smooth = np.cumsum(rng.integers(-3, 4, shape), axis=1).astype(np.uint8)  # every filter type wins somewhere
    return smooth


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_unfilter_geometry(bpp):
    for H in (1, 2, 63, 64, 65, 129, 130):
        for W in (1, 2, 63, 64, 65):
            px = image(bpp, H, W, H * 100 + W)
            check(P.write_png(px, filters=-1, level=1), flags=(-1,))


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_each_fixed_filter_and_a_type_per_row(bpp):
    px = image(bpp, 130, 65, 7)
    for t in range(5):
        check(P.write_png(px, filters=t, level=1))
    check(P.write_png(px, filters=[(3 * y + y // 64) % 5 for y in range(130)], level=1))


def test_long_rows():
    check(P.write_png(image(3, 3, 5000, 1), filters=[4, 3, 4], level=1), flags=(-1, 1, 0))
    check(P.write_png(image(1, 1, 16384, 2), filters=[1], level=1))
    check(P.write_png(image(1, 2, 16384, 3), filters=[3, 4], level=1))


# ---- the host tests' streams ----------------------------------------------------------------------
FOREIGN = P.foreign_cases()
HANDMADE = P.handmade_cases()
PATHCASES = P.path_cases()


@pytest.mark.parametrize("name", sorted(FOREIGN))
def test_foreign_streams(name):
    png, path = FOREIGN[name]
    check(png, path, flags=(1, 0, -1))


@pytest.mark.parametrize("name", sorted(HANDMADE))
def test_handmade_streams(name):
    png, path = HANDMADE[name]
    check(png, path)


@pytest.mark.parametrize("name", sorted(PATHCASES))
def test_path_selection(name):
    png, path = PATHCASES[name]
    check(png, path)


def test_own_files():
    check(sm.imencode_png_host(png_np.runny(9, (3, 40000))), "parallel")
    check(sm.imencode_png_host(P.own_literal_only(), filter=0), "parallel")
    deep = png_np.skewed_no_neighbours(png_np.deep_tree_counts())
    check(sm.imencode_png_host(np.tile(deep, (4, 1)), filter=0), "parallel")
    for kind in ("gray", "bgr", "u16"):
        for name, k, H, W in png_np.SHAPES:
            if k == kind and name in ("1x1", "cuts_mid_row", "one_segment_plus_1", "41x53"):
                check(sm.imencode_png_host(png_np.shape_image(kind, H, W, seed=3)), "parallel")


# ---- batch ------------------------------------------------------------------------------------------
def test_batch_with_a_foreign_and_a_corrupt_file():
    import torch

    imgs = [png_np.shape_image("bgr", 70, 90, seed=s) for s in range(5)]
    files = [sm.imencode_png_host(im) for im in imgs]
    files[2] = P.write_png(np.ascontiguousarray(imgs[2][:, :, ::-1]), level=6, idat_split=700)
    good = sm.imdecode_batch(files, 1)
    assert good.is_cuda and tuple(good.shape) == (5, 70, 90, 3)
    assert _lib.engine(0).png_decode_stats() == (4, 1)
    for i in range(5):
        assert np.array_equal(good[i].cpu().numpy(), imgs[i])
    bad = bytearray(files[3])
    bad[-30] ^= 1  # inside the last IDAT chunk: its CRC no longer holds
    files[3] = bytes(bad)
    with pytest.raises(sm.SmError) as e:
        sm.imdecode_batch(files, 1)
    assert "image 3" in str(e.value) and "CRC" in str(e.value)
    # the statuses and the four good images through the C-ABI
    blob = np.concatenate([np.frombuffer(f, np.uint8) for f in files])
    sizes = np.array([len(f) for f in files], np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    d_blob = torch.from_numpy(blob.copy()).cuda()
    d_tab = torch.from_numpy(np.stack([offs, sizes]).astype(np.int64)).cuda()
    out = torch.zeros((5, 70, 90, 3), dtype=torch.uint8, device="cuda")
    status = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    prm = _lib.SmPngDecParams()
    prm.out_kind, prm.flags, prm.file_channels, prm.file_depth = _lib.SM_PNGDEC_U8, 1, 3, 8
    prm.max_chunks, prm.max_file_bytes = int(sizes.max()) // 12 + 1, int(sizes.max())
    eng = _lib.engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.png_decode_batch_device(d_blob.data_ptr(), d_tab[0].data_ptr(), d_tab[1].data_ptr(), 5, 70, 90, prm, out.data_ptr(),
                                out.stride(0), out.stride(1), status.data_ptr())
    st = status.cpu().tolist()
    assert [s != 0 for s in st] == [False, False, False, True, False], st
    assert b"CRC" in _lib.load().sm_pngdec_status_message(st[3])
    for i in (0, 1, 2, 4):
        assert np.array_equal(out[i].cpu().numpy(), imgs[i])


# ---- rejections: one of each kind, all passed by the host test and the sanitizer program ------------
def test_rejections_on_the_device():
    px = png_np.runny(2, (12, 20))
    png = P.write_png(px, level=6)
    rejects(b"\x89PNG\r\n\x1a\x0b" + png[8:], "bad signature")
    rejects(png[:len(png) - 12], "truncated")
    rejects(png[:60], "truncated")
    bad = bytearray(png)
    bad[8 + 8 + 13 + 2] ^= 0x10
    rejects(bytes(bad), "CRC mismatch")
    z = bytearray(zlib.compress(P.filtered(px)))
    z[-1] ^= 1
    rejects(P.assemble(px, [bytes(z)]), "Adler-32 mismatch")
    st = P.filtered(px, 0)
    rejects(P.assemble(px, [zlib.compress(st[:-21])]), "shorter")
    rejects(P.assemble(px, [zlib.compress(st + st[-21:])]), "longer")
    s5 = bytearray(st)
    s5[21 * 7] = 5
    rejects(P.assemble(px, [zlib.compress(bytes(s5))]), "filter type above 4")
    data = bytes([0, 1, 2, 3, 1, 2, 3, 1])
    one = np.zeros((1, 7), np.uint8)
    b = P.Bits()
    P.fixed_block(b, [0, 1, 2, 3, (4, 5)])
    rejects(P.assemble(one, [P.zlib_wrap(b.bytes(), data)]), "distance beyond the start")
    rejects(P.assemble(one, [P.zlib_wrap(bytes([0b111]), data)]), "block type 3")
    rejects(P.assemble(one, [P.zlib_wrap(bytes([1, 8, 0, 0xF6, 0xFF]) + data, data)]), "LEN / NLEN")
    b = P.Bits()
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(0, 4)
    for _ in range(3):
        b.put(1, 3)
    b.put(0, 3)
    rejects(P.assemble(one, [P.zlib_wrap(b.bytes() + bytes(8), data)]), "over-subscribed or incomplete")
    with pytest.raises(sm.SmError) as e:
        sm.imdecode(P.assemble(px, [zlib.compress(st)], head=P.ihdr(px, interlace=1)), 1)
    assert e.value.code == _lib.SM_E_UNSUPPORTED and "interlace" in str(e.value)


# ---- flags, strides, tensors --------------------------------------------------------------------------
def test_flags_on_every_file_kind():
    rng = np.random.default_rng(5)
    rgb = png_np.shape_image("bgr", 33, 47, seed=1)
    files = [P.write_png(rgb[:, :, 0].copy()), P.write_png(png_np.shape_image("u16", 33, 47, seed=2)), P.write_png(rgb),
             P.write_png(np.dstack([rgb, rng.integers(0, 256, (33, 47), dtype=np.uint8)]))]
    for f in files:
        check(f, flags=(1, 0, -1))
    keep = sm.imdecode(files[2], 1, keep_channel_order=True)
    assert np.array_equal(keep, rgb)


def test_strided_output():
    import torch

    img = png_np.shape_image("bgr", 41, 53, seed=4)
    f = np.frombuffer(sm.imencode_png_host(img), np.uint8)
    d_f = torch.from_numpy(f.copy()).cuda()
    tab = torch.tensor([0, f.size], dtype=torch.int64).cuda()
    out = torch.full((41, 53 * 3 + 29), 0xAB, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    prm = _lib.SmPngDecParams()
    prm.out_kind, prm.flags, prm.file_channels, prm.file_depth = _lib.SM_PNGDEC_U8, 1, 3, 8
    eng = _lib.engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.png_decode_batch_device(d_f.data_ptr(), tab[0:].data_ptr(), tab[1:].data_ptr(), 1, 41, 53, prm, out.data_ptr(), 0,
                                out.stride(0), status.data_ptr())
    assert status.cpu().tolist() == [0]
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :159].reshape(41, 53, 3), img)
    assert (o[:, 159:] == 0xAB).all()


def test_imread_denoise_and_match_on_tensors(tmp_path, golden_cases):
    import torch

    name, left, right, params, expected, raw = next(c for c in golden_cases if c[0] == "sgbm5_d16_settings")
    pl, pr = str(tmp_path / "l.png"), str(tmp_path / "r.png")
    assert sm.imwrite(pl, left) and sm.imwrite(pr, right)
    tl, tr = sm.imread(pl, 0, as_tensor=True), sm.imread(pr, 0, as_tensor=True)
    assert tl.is_cuda and tl.dtype == torch.uint8
    assert np.array_equal(tl.cpu().numpy(), left)
    m = sm.StereoSGBM_create(minDisparity=0, numDisparities=16, blockSize=5)
    dt = m.compute(sm.fastNlMeansDenoising(tl), sm.fastNlMeansDenoising(tr))
    dn = m.compute(sm.fastNlMeansDenoising(sm.imread(pl, 0)), sm.fastNlMeansDenoising(sm.imread(pr, 0)))
    assert dt.is_cuda and np.array_equal(dt.cpu().numpy(), dn)


def test_disparity_png_round_trip_of_the_golden_map(tmp_path, golden_cases):
    name, left, right, params, expected, raw = next(c for c in golden_cases if c[0] == "sgbm5_d16_settings")
    d = np.ascontiguousarray(raw).astype(np.int16)
    path = str(tmp_path / "d.png")
    sm.write_disparity_png(path, d, "kitti")
    back = sm.read_disparity_png(path, "kitti", np.int16, invalid=-16)
    assert np.array_equal(back, np.where(d > 0, d, -16))
    f = sm.read_disparity_png(path, "kitti", np.float32, as_tensor=True)
    assert f.is_cuda and np.array_equal(f.cpu().numpy(), np.where(d > 0, d.astype(np.float32) / 16, np.float32(-1)))
    host = sm.decode_disparity_png(open(path, "rb").read(), host=True, invalid=-16)
    assert np.array_equal(host, back)


@pytest.mark.slow
def test_full_size_round_trip_and_level_6():
    img = png_np.shape_image("bgr", 720, 1280, seed=1)
    own = sm.imencode_png_host(img)
    got = sm.imdecode(own, 1)
    assert np.array_equal(got, img) and _lib.engine(0).png_decode_stats() == (1, 0)
    l6 = P.write_png(np.ascontiguousarray(img[:, :, ::-1]), filters=1, level=6)
    got = sm.imdecode(l6, 1)
    assert np.array_equal(got, img) and _lib.engine(0).png_decode_stats() == (0, 1)
