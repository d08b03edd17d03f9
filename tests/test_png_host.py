"""The PNG encoder's CPU twin (sm_png_encode_host: the functions the GPU kernels run, on the CPU,
no context and no device) through the validator of tests/png_np.py: chunk CRCs, chunk order, IHDR,
zlib's own inflate of the IDAT data (deflate validity, Adler-32), every segment inflated on its
own, the stream byte for byte against the numpy model of conversion + adaptive filtering, and the
pixels after unfiltering.  Where Pillow is installed it must read the same pixels."""
import ctypes
import heapq
import zlib

import numpy as np
import pytest

import png_np
import stereo_match_amd as sma
from stereo_match_amd import _lib

SEG = png_np.SEG


def idat_chunks(png):
    return [d for t, d in png_np.parse_chunks(bytes(png)) if t == b"IDAT"]


def block_type(chunk, first):
    """BTYPE of the chunk's first block: 0 stored, 2 dynamic."""
    return (chunk[2 if first else 0] >> 1) & 3


def roundtrip(img, **opts):
    png = sma.imencode_png_host(img, **opts)
    px = png_np.pixels_of(img, keep_channel_order=opts.get("keep_channel_order", False))
    png_np.validate(png, px, -1 if opts.get("filter") is None else opts["filter"])
    return png, px


@pytest.mark.parametrize("name,kind,H,W", png_np.SHAPES, ids=[f"{s[0]}-{s[1]}" for s in png_np.SHAPES])
def test_shapes(name, kind, H, W):
    for random in (False, True):
        img = png_np.shape_image(kind, H, W, seed=H * 131 + W, random=random)
        png, px = roundtrip(img)
        png_np.check_pillow(png, px)
        assert len(png) <= _lib.load().sm_png_bound(H, W, 3 if kind == "bgr" else 1, 16 if kind == "u16" else 8)


def test_keep_channel_order():
    img = png_np.shape_image("bgr", 37, 67, seed=5)
    png, px = roundtrip(img, keep_channel_order=True)
    assert np.array_equal(px, img)
    assert png != sma.imencode_png_host(img)


def test_strided_rows_are_read_in_place():
    big = png_np.shape_image("gray", 41, 80, seed=6)
    view = big[:, 3:56]
    assert not view.flags.c_contiguous
    assert sma.imencode_png_host(view) == sma.imencode_png_host(np.ascontiguousarray(view))


# ---- run arithmetic: one-row images with filter 0, so the stream is a 0 and then the row ------
@pytest.mark.parametrize("R", [2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 519])
def test_repeat_block(R):
    """R repeating positions between literals: R / 258 matches of 258, a remainder >= 3 as one more
    match, 1 or 2 as literals."""
    img = png_np.repeat_blocks([R, 5, R, 1, R])
    roundtrip(img, filter=0)
    # alone in its segment too: the block at the very end of the stream
    roundtrip(png_np.repeat_blocks([R]), filter=0)


def test_all_repeat_blocks_in_one_row():
    roundtrip(png_np.repeat_blocks([2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 519] * 3, seed=3), filter=0)


def test_run_crossing_a_segment_boundary_is_cut_there():
    """40000 equal bytes: the validator inflates every chunk with a fresh inflater, which fails on
    a match that reaches before the chunk."""
    img = png_np.one_row(np.full(40000, 7))
    png, _ = roundtrip(img, filter=0)
    c = idat_chunks(png)
    assert len(c) == 2 and block_type(c[0], True) == 2 and block_type(c[1], False) == 2
    # runs that end and begin exactly at the cut, and one byte either side of it
    for k in (SEG - 2, SEG - 1, SEG, SEG + 1):
        row = np.concatenate([np.full(k - 1, 9), np.full(3000, 200)])  # stream position k begins the second run
        roundtrip(png_np.one_row(row), filter=0)


def test_segment_of_a_single_byte_value():
    img = png_np.one_row(np.zeros(SEG - 1))  # with the filter byte: 32768 zeros
    png, _ = roundtrip(img, filter=0)
    c = idat_chunks(png)
    assert len(c) == 1 and block_type(c[0], True) == 2
    assert len(c[0]) < 64  # 127 matches of 258 and one of 2 ... as a handful of bytes


def test_segment_without_a_match_uses_the_zero_length_distance_code():
    """32768 bytes, no two neighbours equal, a skewed distribution: a dynamic block with literals
    only.  Its distance code is the single zero-length code (RFC 1951 §3.2.7), which zlib accepts
    only because no distance is used."""
    counts = np.maximum(1, (6000 * 0.8 ** np.arange(40)).astype(int))
    counts[0] += SEG - 1 - counts.sum()
    img = png_np.skewed_no_neighbours(list(counts))
    assert img.size == SEG - 1 and img[0, 0] != 0
    png, _ = roundtrip(img, filter=0)
    c = idat_chunks(png)
    assert len(c) == 1 and block_type(c[0], True) == 2


# ---- length limiting --------------------------------------------------------------------------
def huffman_depth(counts):
    """Depth of the unlimited Huffman tree of these counts."""
    h = [(c, 0) for c in counts]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def test_fibonacci_counts_need_the_length_limit():
    """One segment whose byte counts grow like the Fibonacci sequence over 24 values
    (png_np.deep_tree_counts): every Huffman tree of them is deeper than 15, so the lengths have to
    be limited; zlib inflates the block only if the limited code is complete and not
    over-subscribed."""
    counts = png_np.deep_tree_counts()
    assert len(counts) >= 24 and sum(counts) < SEG
    assert huffman_depth(counts + [1, 1]) > 15
    r = [counts[k + 1] / counts[k] for k in range(12, len(counts) - 1)]
    assert all(1.5 < x < 1.75 for x in r)  # the golden ratio, as Fibonacci's
    img = png_np.skewed_no_neighbours(counts)
    png, _ = roundtrip(img, filter=0)
    c = idat_chunks(png)
    assert len(c) == 1 and block_type(c[0], True) == 2
    # the same counts over several segments and with runs in
    roundtrip(np.tile(img, (4, 1)), filter=0)
    roundtrip(np.tile(img, (3, 1)))


def test_code_length_code_is_limited_to_7_bits():
    """Many different code lengths with Fibonacci-like frequencies among the lengths themselves."""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    counts = []
    for k, f in enumerate(fib[:14]):  # 2^k symbols would be too many: a few symbols per depth
        counts += [f] * min(1 + k, 12)
    counts = [c for c in counts if c > 0][:200]
    scale = (SEG - 2) // (2 * sum(counts)) or 1
    img = png_np.skewed_no_neighbours([c * scale for c in counts])
    roundtrip(img, filter=0)


# ---- sizes ------------------------------------------------------------------------------------
def test_incompressible_input_stays_within_the_all_stored_bound():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (96, 1021), dtype=np.uint8)
    png, px = roundtrip(img)
    n = png_np.stream_len(px)
    assert n > 2 * SEG
    assert len(png) <= png_np.all_stored_size(n)
    assert png_np.all_stored_size(n) == _lib.load().sm_png_bound(96, 1021, 1, 8)
    assert len(png) <= _lib.load().sm_png_bound(96, 1021, 1, 8)
    assert all(block_type(c, k == 0) == 0 for k, c in enumerate(idat_chunks(png)))


def test_runs_pay():
    """A constant 16 x 8191 image: a stream of 131072 bytes.  A coder without runs cannot go below
    one bit a byte (1/8); with them the file is below 1/100."""
    img = np.full((16, 8191), 113, np.uint8)
    png, px = roundtrip(img)
    assert png_np.stream_len(px) == 131072
    print("runs pay: file of", len(png), "bytes for a stream of 131072")
    assert len(png) < 131072 / 100


# ---- disparity maps ---------------------------------------------------------------------------
def test_kitti_int16():
    d = np.array([[-16, -1, 0, 1, 15, 16, 4095, 4096, 32767, -32768]], np.int16)
    want = png_np.pixels_of(d, disp="kitti")
    # 32767 << 4 = 524272 does not fit uint16: above d = 4095 (disparity 255.9375) the value is
    # 65535, as for a float32 map
    assert want.tolist() == [[0, 0, 0, 16, 240, 256, 65520, 65535, 65535, 0]]
    png = sma.encode_disparity_png(d, "kitti", host=True)
    png_np.validate(png, want)
    png_np.check_pillow(png, want)
    d = png_np.runny(3, (41, 53), np.uint16).astype(np.int16)
    png_np.validate(sma.encode_disparity_png(d, "kitti", host=True), png_np.pixels_of(d, disp="kitti"))


def test_kitti_float32():
    d = np.array([[np.nan, np.inf, -np.inf, -0.0, 0.0, 0.00195, 0.001953125, 0.005859375, 255.998, 256.0, 1e30, -3.5,
                   1.0, 0.5 / 256 + 1.0, 1.5 / 256 + 1.0]], np.float32)
    want = png_np.pixels_of(d, disp="kitti")
    #            nan inf -inf -0 0  <half  half->even(0)  1.5->2  clamp  clamp  clamp  neg  256  tie->256  tie->258
    assert want.tolist() == [[0, 0, 0, 0, 0, 0, 0, 2, 65535, 65535, 65535, 0, 256, 256, 258]]
    png = sma.encode_disparity_png(d, "kitti", host=True)
    png_np.validate(png, want)
    rng = np.random.default_rng(2)
    d = (rng.standard_normal((37, 67)) * 80).astype(np.float32)
    d[rng.random(d.shape) < 0.05] = np.nan
    png_np.validate(sma.encode_disparity_png(d, "kitti", host=True), png_np.pixels_of(d, disp="kitti"))


def test_linear_u8():
    # lo 0, hi 510: v = (d + 1) // 2, every odd d a tie at exactly half, rounded up
    d = np.arange(-3, 515, dtype=np.int16).reshape(1, -1)
    want = png_np.pixels_of(d, disp="u8", lo=0, hi=510)
    assert want[0, 3:9].tolist() == [0, 1, 1, 2, 2, 3] and want.max() == 255 and want.min() == 0
    png_np.validate(sma.encode_disparity_png(d, "u8", 0, 510, host=True), want)
    # derived bounds are the map's own minimum and maximum
    rng = np.random.default_rng(4)
    d = rng.integers(-16, 1400, (37, 67)).astype(np.int16)
    derived = sma.encode_disparity_png(d, "u8", host=True)
    png_np.validate(derived, png_np.pixels_of(d, disp="u8"))
    assert derived == sma.encode_disparity_png(d, "u8", int(d.min()), int(d.max()), host=True)
    # hi == lo: 0 everywhere
    flat = np.full((5, 7), 123, np.int16)
    png_np.validate(sma.encode_disparity_png(flat, "u8", host=True), np.zeros((5, 7), np.uint8))
    png_np.validate(sma.encode_disparity_png(d, "u8", 50, 50, host=True), np.zeros(d.shape, np.uint8))
    with pytest.raises(ValueError, match="hi"):
        sma.encode_disparity_png(d, "u8", 10, 9, host=True)
    with pytest.raises(sma.SmError):
        sma.encode_disparity_png(d.astype(np.float32), "u8", host=True)


# ---- filters ----------------------------------------------------------------------------------
def test_filter_ties_go_to_the_lowest_type():
    # a constant first row: Sub (1) and Paeth (4) both leave one byte, None / Up / Average more
    img = np.full((1, 50), 90, np.uint8)
    png, px = roundtrip(img)
    assert zlib.decompress(b"".join(idat_chunks(png)))[0] == 1
    # all zeros: all five tie at 0
    png, px = roundtrip(np.zeros((3, 20), np.uint8))
    s = zlib.decompress(b"".join(idat_chunks(png)))
    assert [s[0], s[21], s[42]] == [0, 0, 0]
    # a second row equal to the first: Up (2), Paeth (4) ... tie at 0, Up is the lowest of them
    row = png_np.shape_image("gray", 1, 40, seed=8, random=True)
    png, px = roundtrip(np.vstack([row, row]))
    assert zlib.decompress(b"".join(idat_chunks(png)))[41] == 2


@pytest.mark.parametrize("f", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["gray", "bgr", "u16"])
def test_fixed_filter(kind, f):
    img = png_np.shape_image(kind, 37, 67, seed=9)
    png, px = roundtrip(img, filter=f)
    s = zlib.decompress(b"".join(idat_chunks(png)))
    n = png_np.stream_len(px) // 37
    assert set(s[::n]) == {f}
    png_np.check_pillow(png, px)


# ---- the C-ABI's sizes and errors -----------------------------------------------------------
def test_capacity_too_small_is_reported_and_nothing_written():
    img = png_np.shape_image("bgr", 37, 67, seed=10)
    want = sma.imencode_png_host(img)
    lib = _lib.load()
    prm = _lib.SmPngParams(src_kind=_lib.SM_PNG_SRC_U8, channels=3, filter=-1)
    nb = ctypes.c_uint64()
    for cap in (0, 1, len(want) // 2, len(want) - 1):
        buf = np.full(len(want) + 64, 0xAB, np.uint8)
        rc = lib.sm_png_encode_host(img.ctypes.data, img.strides[0], 37, 67, ctypes.byref(prm), cap, buf.ctypes.data,
                                    ctypes.byref(nb))
        assert rc == _lib.SM_E_ARG and nb.value == len(want)
        assert (buf == 0xAB).all()
        with pytest.raises(ValueError, match="capacity"):
            _lib.png_encode_host(img, prm, capacity=cap)
    # the size query
    rc = lib.sm_png_encode_host(img.ctypes.data, img.strides[0], 37, 67, ctypes.byref(prm), 0, None, ctypes.byref(nb))
    assert rc == _lib.SM_E_ARG and nb.value == len(want)
    # the exact capacity fits, and the bytes behind it stay untouched
    buf = np.full(len(want) + 64, 0xAB, np.uint8)
    rc = lib.sm_png_encode_host(img.ctypes.data, img.strides[0], 37, 67, ctypes.byref(prm), len(want), buf.ctypes.data,
                                ctypes.byref(nb))
    assert rc == _lib.SM_OK and nb.value == len(want)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()


def test_bound():
    lib = _lib.load()
    assert lib.sm_png_bound(1, 1, 1, 8) == 2 + 17 + 6 + 57
    assert lib.sm_png_bound(375, 1242, 1, 16) == png_np.all_stored_size(375 * (2 * 1242 + 1))
    assert lib.sm_png_bound(0, 5, 1, 8) == 0 and lib.sm_png_bound(5, 5, 2, 8) == 0 and lib.sm_png_bound(5, 5, 3, 16) == 0
    assert lib.sm_png_bound(32768, 65536, 1, 8) == 0  # a stream of 2^31 bytes and more


def test_bad_arguments():
    lib = _lib.load()
    img = np.zeros((4, 6), np.uint8)
    nb = ctypes.c_uint64()
    buf = np.zeros(4096, np.uint8)

    def call(prm, H=4, W=6, stride=6, ptr=img.ctypes.data):
        return lib.sm_png_encode_host(ptr, stride, H, W, ctypes.byref(prm), buf.size, buf.ctypes.data, ctypes.byref(nb))

    ok = dict(src_kind=_lib.SM_PNG_SRC_U8, channels=1, filter=-1)
    assert call(_lib.SmPngParams(**ok)) == _lib.SM_OK
    assert call(_lib.SmPngParams(**ok), H=0) == _lib.SM_E_ARG
    assert call(_lib.SmPngParams(**ok), ptr=None) == _lib.SM_E_ARG
    assert call(_lib.SmPngParams(**ok), stride=5) == _lib.SM_E_ARG
    assert call(_lib.SmPngParams(**{**ok, "channels": 2})) == _lib.SM_E_ARG
    assert call(_lib.SmPngParams(**{**ok, "filter": 5})) == _lib.SM_E_ARG
    assert call(_lib.SmPngParams(**{**ok, "src_kind": 9})) == _lib.SM_E_ARG
    assert call(_lib.SmPngParams(src_kind=_lib.SM_PNG_SRC_U16, channels=3, filter=-1)) == _lib.SM_E_ARG
    assert call(_lib.SmPngParams(src_kind=_lib.SM_PNG_SRC_DISP_I16, channels=1, filter=-1,
                                 disp_mode=_lib.SM_PNG_DISP_LINEAR_U8, has_bounds=1, lo=5, hi=4), W=3) == _lib.SM_E_ARG
    # nothing is read before the size check: a stream of 2^31 bytes and more
    assert call(_lib.SmPngParams(**ok), H=32768, W=65536, stride=65536) == _lib.SM_E_UNSUPPORTED


def test_python_surface_refuses_other_inputs(tmp_path):
    with pytest.raises(sma.SmError):
        sma.imencode_png_host(np.zeros((4, 4), np.float32))
    with pytest.raises(sma.SmError):
        sma.imencode_png_host(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(sma.SmError):
        sma.imencode_png_host(np.zeros((4, 4, 3), np.uint16))
    with pytest.raises(sma.SmError):
        sma.imwrite(str(tmp_path / "x.jpg"), np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        sma.encode_disparity_png(np.zeros((4, 4), np.int16), "png16", host=True)
