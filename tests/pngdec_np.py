"""Helpers of the PNG input tests: a PNG writer with a chosen filter per row,
zlib level / strategy / flush mode, IDAT split and extra chunks; a fixed-Huffman token writer for
deflate streams zlib's compressor never emits; the judge (zlib.decompress + png_np.unfilter_stream,
never the code under test); and the shared lists of stream cases the host and the GPU tests run.
No test functions here."""
import struct
import zlib

import numpy as np

import png_np

CAP = 32768  # SM_PNGDEC_CAP
SEG = png_np.SEG


# ---- the writer ---------------------------------------------------------------------------------
def chunk(typ: bytes, data: bytes = b"") -> bytes:
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data))


def file_geometry(px):
    """(depth, colour type, bpp) of the file that holds px: uint8 [H, W], [H, W, 3] (RGB), [H, W, 4]
    (RGBA) or uint16 [H, W]."""
    if px.dtype == np.uint16:
        return 16, 0, 2
    if px.ndim == 2:
        return 8, 0, 1
    return (8, 2, 3) if px.shape[2] == 3 else (8, 6, 4)


def raw_rows(px):
    H = px.shape[0]
    if px.dtype == np.uint16:
        return px.astype(">u2").view(np.uint8).reshape(H, -1)
    return np.ascontiguousarray(px).reshape(H, -1)


def filtered(px, filters=-1):
    """The filtered stream of px: filters an int (-1 adaptive, 0..4 for every row) or a type per row."""
    rows = raw_rows(px)
    bpp = file_geometry(px)[2]
    if isinstance(filters, int):
        return png_np.filter_stream(rows, bpp, filters).tobytes()
    H, n = rows.shape
    by_type = {t: png_np.filter_stream(rows, bpp, t).reshape(H, n + 1) for t in set(filters)}
    return b"".join(by_type[t][y].tobytes() for y, t in enumerate(filters))


def deflate_pieces(stream: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, pieces=None, flush=zlib.Z_FULL_FLUSH):
    """The zlib stream of `stream` as a list of byte strings: one, or one per entry of `pieces`
    (bytes of input each, the rest in a last one), every piece but the last closed by `flush`."""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if not pieces:
        return [c.compress(stream) + c.flush()]
    out, at = [], 0
    for n in pieces:
        out.append(c.compress(stream[at:at + n]) + c.flush(flush))
        at += n
    out.append(c.compress(stream[at:]) + c.flush())
    return out


def split(data: bytes, n):
    return [data[i:i + n] for i in range(0, len(data), n)] if n else [data]


def ihdr(px, interlace=0, depth=None, ctype=None):
    d, c, _ = file_geometry(px)
    return struct.pack(">IIBBBBB", px.shape[1], px.shape[0], d if depth is None else depth, c if ctype is None else ctype,
                       0, 0, interlace)


def assemble(px, idat, before=(), between=(), head=None):
    """A file: IHDR, `before` chunks, the IDAT data strings (the `between` chunks behind the first
    one), IEND."""
    out = png_np.SIG + chunk(b"IHDR", head if head is not None else ihdr(px))
    for t, d in before:
        out += chunk(t, d)
    for k, d in enumerate(idat):
        out += chunk(b"IDAT", d)
        if k == 0:
            for t, dd in between:
                out += chunk(t, dd)
    return out + chunk(b"IEND")


def write_png(px, filters=-1, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, idat_split=None, pieces=None,
              flush=zlib.Z_FULL_FLUSH, before=(), between=()):
    z = deflate_pieces(filtered(px, filters), level, strategy, pieces, flush)
    idat = z if pieces else split(z[0], idat_split)
    return assemble(px, idat, before, between)


# ---- fixed-Huffman token writer -------------------------------------------------------------------
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    """LSB-first bit string."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):  # a Huffman code: most significant bit first
        self.put(int(format(c, f"0{k}b")[::-1], 2), k)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def _fixed_sym(b: Bits, s):
    if s < 144:
        b.code(0x30 + s, 8)
    elif s < 256:
        b.code(0x190 + s - 144, 9)
    elif s < 280:
        b.code(s - 256, 7)
    else:
        b.code(0xC0 + s - 280, 8)


def fixed_block(b: Bits, tokens, final=True):
    """One fixed-Huffman block: tokens are ints (literals) or (length, distance) pairs."""
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_sym(b, t)
            continue
        length, dist = t
        ls = max(k for k in range(29) if _LBASE[k] <= length) if length != 258 else 28
        _fixed_sym(b, 257 + ls)
        b.put(length - _LBASE[ls], _LEXT[ls])
        ds = max(k for k in range(30) if _DBASE[k] <= dist)
        b.code(ds, 5)
        b.put(dist - _DBASE[ds], _DEXT[ds])
    _fixed_sym(b, 256)


def inflate_tokens(tokens):
    """What the tokens stand for, byte by byte."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def zlib_wrap(raw: bytes, data: bytes) -> bytes:
    return b"\x78\x01" + raw + struct.pack(">I", zlib.adler32(data))


def gray_of_stream(data: bytes, W):
    """The one-channel uint8 image whose filter-0 stream is `data` (len = H * (W + 1), a 0 byte
    in front of every row)."""
    a = np.frombuffer(data, np.uint8).reshape(-1, W + 1)
    assert not a[:, 0].any()
    return np.ascontiguousarray(a[:, 1:])


def token_file(tokens_per_block, W, idat_split=None):
    """A gray file of width W whose deflate stream is these fixed-Huffman blocks: (file, pixels)."""
    data = inflate_tokens([t for blk in tokens_per_block for t in blk])
    px = gray_of_stream(data, W)
    b = Bits()
    for k, blk in enumerate(tokens_per_block):
        fixed_block(b, blk, final=k + 1 == len(tokens_per_block))
    return assemble(px, split(zlib_wrap(b.bytes(), data), idat_split)), px


def token_chunks(chunks_tokens, W):
    """A gray file with one IDAT chunk per entry: its tokens in one fixed block; a chunk that is
    not the last ends with an empty stored block (byte aligned).  Distances may reach back over
    the chunk's start: that is the point."""
    data = inflate_tokens([t for c in chunks_tokens for t in c])
    px = gray_of_stream(data, W)
    idat = []
    for k, toks in enumerate(chunks_tokens):
        last = k + 1 == len(chunks_tokens)
        b = Bits()
        fixed_block(b, toks, final=last)
        if not last:
            b.put(0, 3)
            b.align()
            b.put(0, 16)
            b.put(0xFFFF, 16)
        d = b.bytes()
        if k == 0:
            d = b"\x78\x01" + d
        if last:
            d += struct.pack(">I", zlib.adler32(data))
        idat.append(d)
    return assemble(px, idat), px


# ---- the judge ----------------------------------------------------------------------------------
def judge(png: bytes):
    """The pixels of the file in its own channel order and depth, by zlib and png_np: uint8 [H, W],
    [H, W, 3], [H, W, 4] or uint16 [H, W]."""
    chunks = png_np.parse_chunks(bytes(png))
    W, H, depth, ctype = struct.unpack(">IIBB", chunks[0][1][:10])
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    bpp = ch * depth // 8
    stream = zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT"))
    assert len(stream) == H * (W * bpp + 1)
    rows = png_np.unfilter_stream(stream, H, W * bpp, bpp)
    if depth == 16:
        return rows.reshape(H, W, 2).astype(np.uint16) @ np.array([256, 1], np.uint16)
    return rows.reshape(H, W) if ch == 1 else rows.reshape(H, W, ch)


def gray_formula(bgr):
    b, g, r = (bgr[..., k].astype(np.uint32) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def expected(px, flags):
    """What imdecode(flags) returns for a file that holds px (judge)."""
    if px.dtype == np.uint16:
        if flags == -1:
            return px
        px = (px >> 8).astype(np.uint8)
    if px.ndim == 3:
        bgr = np.ascontiguousarray(px[:, :, 2::-1])
        return gray_formula(bgr) if flags == 0 else bgr
    if flags == 1:
        return np.repeat(px[:, :, None], 3, axis=2)
    return px


def pillow_pixels(png):
    import io

    import pytest

    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(bytes(png)))
    im.load()
    return np.asarray(im)


# ---- shared stream cases: name -> (file, path) with path "parallel", "serial" or None (not asserted)
def _small(kind="bgr", seed=5):
    return png_np.shape_image(kind, 41, 53, seed=seed)


def _rgb(img):
    return np.ascontiguousarray(img[:, :, ::-1]) if img.ndim == 3 else img


def foreign_cases():
    out = {}
    rgb = _rgb(_small())
    for level in (0, 1, 6, 9):
        out[f"level{level}"] = (write_png(rgb, level=level), None)
    for name, s in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman_only", zlib.Z_HUFFMAN_ONLY)):
        out[f"strategy_{name}"] = (write_png(rgb, strategy=s), None)
    out["split_1"] = (write_png(rgb, idat_split=1), "serial")
    out["split_8192"] = (write_png(_rgb(png_np.shape_image("bgr", 300, 300, seed=2)), level=6, idat_split=8192), "serial")
    out["whole"] = (write_png(rgb, idat_split=None), None)
    z = deflate_pieces(filtered(rgb))[0]
    out["zero_length_idat"] = (assemble(rgb, [z[:100], b"", z[100:]]), None)
    extra = [(b"tEXt", b"Comment\0hello"), (b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), (b"gAMA", struct.pack(">I", 45455))]
    out["ancillary"] = (write_png(rgb, idat_split=500, before=extra, between=extra), None)
    rng = np.random.default_rng(7)
    rgba = np.dstack([rgb, rng.integers(0, 256, rgb.shape[:2], dtype=np.uint8)])
    out["rgba"] = (write_png(rgba), None)
    out["gray16_level6"] = (write_png(_small("u16")), None)
    return out


def handmade_cases():
    out = {}
    rng = np.random.default_rng(11)
    # distance 32768: W = 32767 so that a row of the stream is 32768 bytes; row 1 repeats row 0
    W = 32767
    row = [0] + [int(v) for v in rng.integers(1, 256, W)]
    toks = row + [(258, 32768)] * 126 + [(257, 32768), (3, 32768)]  # 126 * 258 + 257 + 3 = 32768
    out["distance_32768"] = (token_file([toks], W)[0], "serial")
    for d in (1, 2, 3):
        W2 = 258 + d
        out[f"len258_dist{d}"] = (token_file([[0] + [int(v) for v in rng.integers(1, 256, d)] + [(258, d)]], W2)[0], None)
    out["len3"] = (token_file([[0, 5, 6, 7, 9, (3, 3), 1]], 8)[0], None)
    out["match_ends_stream"] = (token_file([[0, 1, 2, 3, (4, 3)]], 7)[0], None)
    return out


def own_literal_only():
    """Our encoder's literal-only dynamic block: the zero-length distance tree."""
    counts = np.maximum(1, (6000 * 0.8 ** np.arange(40)).astype(int))
    counts[0] += SEG - 1 - counts.sum()
    return png_np.skewed_no_neighbours(list(counts))


def path_cases():
    """name -> (file, path).  The pieces 1000 / 5 / 3000 are bytes of the stream."""
    out = {}
    rng = np.random.default_rng(3)
    gray = png_np.runny(4, (89, 44))  # a stream of 89 * 45 = 4005 bytes
    out["full_flush_pieces"] = (write_png(gray, filters=0, pieces=[1000, 5], flush=zlib.Z_FULL_FLUSH), "parallel")
    out["sync_flush_pieces"] = (write_png(gray, filters=0, pieces=[1000, 5], flush=zlib.Z_SYNC_FLUSH), "serial")
    big = rng.integers(0, 256, (900, 44), dtype=np.uint8)  # 40500 bytes: one piece above the cap
    out["full_flush_piece_above_cap"] = (write_png(big, filters=0, level=1, pieces=[1000, 5, CAP + 1000],
                                                   flush=zlib.Z_FULL_FLUSH), "serial")
    # a hand-made second chunk whose match reaches exactly to its first byte / one byte further
    first = [0] + [int(v) for v in rng.integers(1, 256, 9)]
    out["match_to_chunk_start"] = (token_chunks([first, [0, 7, 8, 9, 1, (4, 5), 2]], 9)[0], "parallel")
    out["match_before_chunk_start"] = (token_chunks([first, [0, 7, 8, 9, 1, (4, 6), 2]], 9)[0], "serial")
    return out
