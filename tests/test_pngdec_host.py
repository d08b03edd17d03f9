"""PNG input on the CPU twin (sm_png_decode_host): the functions the GPU kernels
run, called in loops.  The judge is zlib.decompress + png_np.unfilter_stream (and Pillow where it
is installed), never the code under test."""
import os
import struct
import zlib

import numpy as np
import pytest

import png_np
import pngdec_np as P
import stereo_match_amd as sm
from stereo_match_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_PNG = os.path.join(HERE, "golden", "png")
PATHS = {"parallel": (1, 0), "serial": (0, 1)}


def check(png, path=None, flags=(1, 0, -1)):
    want = P.judge(png)
    for fl in flags:
        got = sm.imdecode_host(png, fl)
        exp = P.expected(want, fl)
        assert got.dtype == exp.dtype and got.shape == exp.shape, (fl, got.shape, exp.shape)
        assert np.array_equal(got, exp), f"flags {fl}"
        if path:
            assert _lib.png_decode_stats(None) == PATHS[path], (path, _lib.png_decode_stats(None))
    return want


def rejects(png, text, code=_lib.SM_E_DATA):
    with pytest.raises(sm.SmError) as e:
        sm.imdecode_host(png, -1)
    assert e.value.code == code and text in str(e.value), str(e.value)


# ---- round trip -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,H,W", png_np.SHAPES, ids=[f"{s[0]}-{s[1]}" for s in png_np.SHAPES])
def test_round_trip_of_our_own_files(name, kind, H, W):
    img = png_np.shape_image(kind, H, W, seed=H + W)
    for flt in (None, 0, 1, 2, 3, 4):
        png = sm.imencode_png_host(img, filter=flt)
        got = sm.imdecode_host(png, -1)
        assert got.dtype == img.dtype and np.array_equal(got, img), (kind, flt)
        assert _lib.png_decode_stats(None) == (1, 0)  # every file of ours inflates chunk-parallel


def test_round_trip_against_the_judge_and_pillow():
    for kind in ("gray", "bgr", "u16"):
        png = sm.imencode_png_host(png_np.shape_image(kind, 37, 67, seed=1))
        px = check(png, "parallel")
        pil = P.pillow_pixels(png)
        assert np.array_equal(pil.astype(np.int64), px.astype(np.int64))


# ---- foreign streams ------------------------------------------------------------------------------
FOREIGN = P.foreign_cases()
HANDMADE = P.handmade_cases()
PATHCASES = P.path_cases()


@pytest.mark.parametrize("name", sorted(FOREIGN))
def test_foreign_streams(name):
    png, path = FOREIGN[name]
    check(png, path)


def test_rgba_drops_alpha_and_pillow_agrees():
    png, _ = FOREIGN["rgba"]
    got = sm.imdecode_host(png, -1)
    assert got.shape[2] == 3
    assert np.array_equal(got[:, :, ::-1], P.pillow_pixels(png)[:, :, :3])


# ---- hand-made streams ----------------------------------------------------------------------------
def test_zlib_never_reaches_distance_32768():
    """Why the stream is hand-made: data of period 32768 does not compress at level 9 (zlib's
    matcher stops at 32768 - 262)."""
    rng = np.random.default_rng(0)
    row = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    assert len(zlib.compress(row + row, 9)) > 2 * 32768
    png, _ = HANDMADE["distance_32768"]
    assert len(png) < 32768 * 9 // 8 + 1000  # the first row in 8- and 9-bit literals, the second almost free


@pytest.mark.parametrize("name", sorted(HANDMADE))
def test_handmade_streams(name):
    png, path = HANDMADE[name]
    check(png, path, flags=(-1,))


def test_literal_only_dynamic_block_with_the_zero_length_distance_tree():
    img = P.own_literal_only()
    png = sm.imencode_png_host(img, filter=0)
    idat = [d for t, d in png_np.parse_chunks(png) if t == b"IDAT"]
    assert len(idat) == 1 and (idat[0][2] >> 1) & 3 == 2  # one dynamic block
    assert np.array_equal(sm.imdecode_host(png, -1), img)


def test_codes_of_15_bits():
    img = png_np.skewed_no_neighbours(png_np.deep_tree_counts())
    for im in (img, np.tile(img, (4, 1))):
        png = sm.imencode_png_host(im, filter=0)
        assert np.array_equal(sm.imdecode_host(png, -1), im)
        check(png, "parallel", flags=(-1,))


# ---- path selection -------------------------------------------------------------------------------
def test_own_multi_segment_file_takes_the_parallel_path():
    img = png_np.runny(9, (3, 40000))
    png = sm.imencode_png_host(img)
    assert png_np.stream_len(img) > P.SEG
    check(png, "parallel", flags=(-1,))


def test_sync_flush_pieces_reference_back():
    """Checked here: pieces 2.. of the Z_SYNC_FLUSH file fail a fresh raw inflater (distance too
    far back) while the joined stream inflates; the Z_FULL_FLUSH pieces all inflate alone."""
    def alone(png):
        idat = [d for t, d in png_np.parse_chunks(png) if t == b"IDAT"]
        idat[0], idat[-1] = idat[0][2:], idat[-1][:-4]
        res = []
        for d in idat:
            o = zlib.decompressobj(-15)
            try:
                res.append(len(o.decompress(d)))
            except zlib.error as e:
                res.append(str(e))
        return res

    sync = alone(PATHCASES["sync_flush_pieces"][0])
    assert sync[0] == 1000 and any(isinstance(r, str) and "too far back" in r for r in sync[1:]), sync
    assert alone(PATHCASES["full_flush_pieces"][0]) == [1000, 5, 3000]
    above = alone(PATHCASES["full_flush_piece_above_cap"][0])
    assert above[:2] == [1000, 5] and above[2] > P.CAP


@pytest.mark.parametrize("name", sorted(PATHCASES))
def test_path_selection(name):
    png, path = PATHCASES[name]
    check(png, path, flags=(-1,))


def test_split_8192_of_a_level_6_file_is_serial():
    png, path = FOREIGN["split_8192"]
    assert path == "serial"
    check(png, path, flags=(-1,))


# ---- rejections -----------------------------------------------------------------------------------
def small_file():
    return P.write_png(png_np.runny(2, (12, 20)), level=6)


def with_idat(px, z):
    return P.assemble(px, [z])


def test_bad_signature_and_truncation():
    png = small_file()
    rejects(b"", "bad signature")
    rejects(b"\x89PNG\r\n\x1a\x0b" + png[8:], "bad signature")
    chunks, pos = [], 8
    while pos < len(png):
        chunks.append(pos)
        pos += 12 + struct.unpack(">I", png[pos:pos + 4])[0]
    for cut in chunks[1:] + [chunks[1] + 5, chunks[1] + 14, len(png) - 1, 20]:
        rejects(png[:cut], "truncated")


def test_flipped_crc_and_wrong_adler():
    png = bytearray(small_file())
    png[8 + 8 + 13 + 2] ^= 0x10  # IHDR's CRC
    rejects(bytes(png), "CRC mismatch")
    px = png_np.runny(2, (12, 20))
    z = bytearray(P.deflate_pieces(P.filtered(px))[0])
    z[-1] ^= 1
    rejects(with_idat(px, bytes(z)), "Adler-32 mismatch")


def test_stream_one_row_short_and_long():
    px = png_np.runny(2, (12, 20))
    st = P.filtered(px, 0)
    rejects(with_idat(px, zlib.compress(st[:-21])), "shorter")
    rejects(with_idat(px, zlib.compress(st + st[-21:])), "longer")


def test_filter_byte_5():
    px = png_np.runny(2, (12, 20))
    st = bytearray(P.filtered(px, 0))
    st[21 * 7] = 5
    rejects(with_idat(px, zlib.compress(bytes(st))), "filter type above 4")


def _raw_file(raw, data, W):
    """A gray file of width W around a raw deflate stream said to inflate to `data`."""
    px = np.zeros((max(1, len(data) // (W + 1)), W), np.uint8)
    return P.assemble(px, [P.zlib_wrap(raw, data)])


def test_deflate_faults():
    data = bytes([0, 1, 2, 3, 1, 2, 3, 1])
    b = P.Bits()
    P.fixed_block(b, [0, 1, 2, 3, (4, 5)])  # distance 5 with four bytes made
    rejects(_raw_file(b.bytes(), data, 7), "distance beyond the start")
    rejects(_raw_file(bytes([0b111]), data, 7), "block type 3")
    rejects(_raw_file(bytes([1, 8, 0, 0xF6, 0xFF]) + data, data, 7), "LEN / NLEN")
    # a dynamic block whose code-length code has three codes of length 1
    b = P.Bits()
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(0, 4)
    for _ in range(3):
        b.put(1, 3)
    b.put(0, 3)
    rejects(_raw_file(b.bytes() + bytes(8), data, 7), "over-subscribed or incomplete")
    z = bytearray(zlib.compress(data))
    z[0] = 0x79  # CM = 9
    rejects(_raw_file(b"", data, 7)[:0] + P.assemble(np.zeros((1, 7), np.uint8), [bytes(z)]), "zlib header")


@pytest.mark.parametrize("field,head,text", [
    ("interlace", dict(interlace=1), "interlace"),
    ("palette", dict(ctype=3), "palette"),
    ("depth1", dict(depth=1), "bit depth 1, 2 or 4"),
    ("depth2", dict(depth=2), "bit depth 1, 2 or 4"),
    ("depth4", dict(depth=4), "bit depth 1, 2 or 4"),
    ("rgb16", dict(depth=16, ctype=2), "16-bit colour"),
    ("rgba16", dict(depth=16, ctype=6), "16-bit colour"),
    ("gray_alpha", dict(ctype=4), "gray + alpha"),
])
def test_unsupported_ihdr(field, head, text):
    px = png_np.runny(2, (12, 20))
    png = P.assemble(px, [zlib.compress(P.filtered(px))], head=P.ihdr(px, **head))
    rejects(png, text, _lib.SM_E_UNSUPPORTED)
    with pytest.raises(sm.SmError):
        _lib.png_info(png)


def test_imread_of_a_missing_file_is_none(tmp_path):
    assert sm.imread(str(tmp_path / "nothing.png")) is None


# ---- mutation sweep -------------------------------------------------------------------------------
def test_mutation_sweep_agrees_with_zlib():
    """2000 single-byte mutations of a small file's IDAT data (CRCs recomputed): zlib.error, a
    wrong length or (inside zlib) a wrong Adler <=> SmError; else the same pixels."""
    px = png_np.runny(6, (24, 31))
    z = zlib.compress(P.filtered(px), 6)
    n = px.shape[0] * (px.shape[1] + 1)
    rng = np.random.default_rng(2024)
    bad = good = 0
    for _ in range(2000):
        m = bytearray(z)
        m[int(rng.integers(0, len(m)))] ^= int(rng.integers(1, 256))
        png = P.assemble(px, [bytes(m[:17]), bytes(m[17:])])
        try:
            st = zlib.decompress(bytes(m))
            ok = len(st) == n and max(st[::px.shape[1] + 1]) <= 4
        except zlib.error:
            ok = False
        if ok:
            good += 1
            want = png_np.unfilter_stream(st, px.shape[0], px.shape[1], 1)
            assert np.array_equal(sm.imdecode_host(png, -1), want)
        else:
            bad += 1
            with pytest.raises(sm.SmError):
                sm.imdecode_host(png, -1)
    assert bad > 1500 and good + bad == 2000


# ---- disparity ------------------------------------------------------------------------------------
def test_kitti_disparity_round_trip():
    d = np.arange(-16, 4096, dtype=np.int16).reshape(8, 514)
    png = sm.encode_disparity_png(d, "kitti", host=True)
    back = sm.decode_disparity_png(png, "kitti", np.int16, invalid=-7, host=True)
    assert back.dtype == np.int16
    assert np.array_equal(back, np.where(d > 0, d, -7))
    f = sm.decode_disparity_png(png, "kitti", np.float32, invalid=-3.5, host=True)
    assert f.dtype == np.float32
    assert np.array_equal(f, np.where(d > 0, d.astype(np.float32) / 16, np.float32(-3.5)))
    fm = np.float32([[0.0, 0.00390625, 1.5, 255.99609375, -2.0]])
    back = sm.decode_disparity_png(sm.encode_disparity_png(fm, "kitti", host=True), dtype=np.float32, host=True)
    assert np.array_equal(back, np.float32([[-1.0, 0.00390625, 1.5, 255.99609375, -1.0]]))


def test_committed_16_bit_file_written_by_pillow():
    path = os.path.join(GOLDEN_PNG, "pillow_gray16.png")
    with open(path, "rb") as f:
        png = f.read()
    want = np.load(os.path.join(GOLDEN_PNG, "pillow_gray16.npz"))["pixels"]
    assert np.array_equal(P.judge(png), want)
    assert np.array_equal(sm.imdecode_host(png, -1), want)
    assert np.array_equal(sm.imdecode_host(png, 0), (want >> 8).astype(np.uint8))
    f = sm.decode_disparity_png(png, dtype=np.float32, host=True)
    assert np.array_equal(f, np.where(want > 0, want.astype(np.float32) / 256, np.float32(-1)))
