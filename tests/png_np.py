"""numpy + stdlib model and validator of the PNG files of stereo_match_amd.

The model: pixel conversion (BGR -> RGB, big-endian 16-bit samples, the two disparity modes) and
libpng's adaptive filter heuristic with ties to the lowest type, as include/stereo_match_amd.h
states them.  The validator parses the file, checks every chunk's CRC with zlib.crc32, the chunk
order and the IHDR fields, inflates the concatenated IDAT data with zlib (which checks the deflate
stream and the Adler-32), inflates every chunk ON ITS OWN with a fresh raw inflater (no match may
reach before its segment), compares the stream byte for byte with the model, and unfilters it
back to the pixels."""
import struct
import zlib

import numpy as np

SEG = 32768
SIG = b"\x89PNG\r\n\x1a\n"


# ---- pixel conversion ---------------------------------------------------------------------
def kitti_i16(d):
    d = np.asarray(d).astype(np.int32)
    return np.where(d < 0, 0, np.minimum(d << 4, 65535)).astype(np.uint16)  # d << 4 fits up to d = 4095


def kitti_f32(d):
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(d * np.float32(256))  # float32, ties to even
        ok = np.isfinite(d) & (d > 0)
        v = np.where(ok, np.minimum(r, np.float32(65535)), np.float32(0))
    return v.astype(np.uint16)


def linear_u8(d, lo=None, hi=None):
    d = np.asarray(d).astype(np.int64)
    if lo is None:
        lo, hi = int(d.min()), int(d.max())
    if hi == lo:
        return np.zeros(d.shape, np.uint8)
    span = hi - lo
    return np.clip(((d - lo) * 510 + span) // (2 * span), 0, 255).astype(np.uint8)


def pixels_of(src, *, keep_channel_order=False, disp=None, lo=None, hi=None):
    """The pixels the file must hold, in the file's channel order: uint8 [H, W], uint8 [H, W, 3]
    or uint16 [H, W].  disp: None (an image), "kitti" or "u8"."""
    a = np.asarray(src)
    if disp == "kitti":
        return kitti_i16(a) if a.dtype == np.int16 else kitti_f32(a)
    if disp == "u8":
        return linear_u8(a, lo, hi)
    if a.ndim == 3 and not keep_channel_order:
        return np.ascontiguousarray(a[:, :, ::-1])
    return np.ascontiguousarray(a)


def raw_rows(px):
    """[H, W * bpp] bytes of the unfiltered rows, and bpp."""
    H = px.shape[0]
    if px.dtype == np.uint16:
        return px.astype(">u2").view(np.uint8).reshape(H, -1), 2
    return px.reshape(H, -1), (3 if px.ndim == 3 else 1)


# ---- filters --------------------------------------------------------------------------------
def _candidates(cur, up, bpp):
    x = cur.astype(np.int32)
    b = up.astype(np.int32)
    a = np.zeros_like(x)
    c = np.zeros_like(x)
    a[bpp:] = x[:-bpp]
    c[bpp:] = b[:-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return [(x - pred) & 255 for pred in (0, a, b, (a + b) >> 1, paeth)]


def filter_stream(rows, bpp, filter=-1):
    """The filtered stream: per row the type byte and the filtered bytes."""
    H, n = rows.shape
    out = np.empty((H, n + 1), np.uint8)
    up = np.zeros(n, np.uint8)
    for y in range(H):
        cand = _candidates(rows[y], up, bpp)
        if filter < 0:
            sums = [int(np.where(f < 128, f, 256 - f).sum()) for f in cand]
            t = sums.index(min(sums))  # the first minimum: ties to the lowest type
        else:
            t = filter
        out[y, 0] = t
        out[y, 1:] = cand[t]
        up = rows[y]
    return out.reshape(-1)


def unfilter_stream(stream, H, n, bpp):
    """The unfiltered rows [H, n] of a filtered stream."""
    s = np.frombuffer(bytes(stream), np.uint8).reshape(H, n + 1)
    out = np.zeros((H, n), np.uint8)
    up = np.zeros(n, np.uint8)
    for y in range(H):
        t, f = int(s[y, 0]), s[y, 1:]
        if t == 0:
            cur = f.copy()
        elif t == 1:
            w = -(-n // bpp)
            pad = np.zeros(w * bpp, np.uint64)
            pad[:n] = f
            cur = (np.cumsum(pad.reshape(w, bpp), axis=0) & 255).astype(np.uint8).reshape(-1)[:n]
        elif t == 2:
            cur = ((f.astype(np.int32) + up) & 255).astype(np.uint8)
        elif t in (3, 4):
            fb, ub, cb = f.tolist(), up.tolist(), [0] * n
            for i in range(n):
                a = cb[i - bpp] if i >= bpp else 0
                b = ub[i]
                if t == 3:
                    pred = (a + b) >> 1
                else:
                    c = ub[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cb[i] = (fb[i] + pred) & 255
            cur = np.array(cb, np.uint8)
        else:
            raise AssertionError(f"row {y}: filter type {t}")
        out[y] = cur
        up = cur
    return out


# ---- the file -------------------------------------------------------------------------------
def parse_chunks(png: bytes):
    """[(type, data)] with every CRC checked."""
    assert png[:8] == SIG, "PNG signature"
    pos, chunks = 8, []
    while pos < len(png):
        assert pos + 12 <= len(png), "truncated chunk"
        (n,) = struct.unpack(">I", png[pos:pos + 4])
        typ = png[pos + 4:pos + 8]
        assert pos + 12 + n <= len(png), f"chunk {typ!r} runs past the file"
        data = png[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + data), f"CRC of chunk {len(chunks)} ({typ!r})"
        chunks.append((typ, data))
        pos += 12 + n
    return chunks


def stream_len(px):
    rows, _ = raw_rows(px)
    return rows.shape[0] * (rows.shape[1] + 1)


def all_stored_size(nstream):
    """The derived bound of a file whose every segment is stored: stream + 5 a segment + 12 a
    chunk + 6 (zlib header, Adler-32) + 57 (signature, IHDR, IEND)."""
    nseg = -(-nstream // SEG)
    return nstream + 5 * nseg + 12 * nseg + 6 + 57


def validate(png: bytes, px, filter=-1):
    """Check the file against the pixels px (pixels_of).  Returns the inflated stream."""
    png = bytes(png)
    chunks = parse_chunks(png)
    types = [t for t, _ in chunks]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and len(chunks[-1][1]) == 0
    assert set(types[1:-1]) == {b"IDAT"}, f"chunks {types}"
    H, W = px.shape[:2]
    depth = 16 if px.dtype == np.uint16 else 8
    ctype = 2 if px.ndim == 3 else 0
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, 0), "IHDR fields"
    rows, bpp = raw_rows(px)
    n = rows.shape[1]
    want = filter_stream(rows, bpp, filter).tobytes()
    idat = [d for t, d in chunks if t == b"IDAT"]
    assert len(idat) == -(-len(want) // SEG), f"{len(idat)} IDAT chunks for a stream of {len(want)} bytes"
    assert idat[0][:2] == b"\x78\x01", "zlib header"
    stream = zlib.decompress(b"".join(idat))  # deflate validity and the Adler-32
    assert len(stream) == len(want)
    # every segment on its own: a fresh raw inflater knows nothing before the chunk
    for k, d in enumerate(idat):
        body = d[2:] if k == 0 else d
        if k == len(idat) - 1:
            body = body[:-4]
        o = zlib.decompressobj(-15)
        part = o.decompress(body) + o.flush()
        assert part == stream[k * SEG:(k + 1) * SEG], f"segment {k} does not inflate on its own to its bytes"
        assert o.unused_data == b""
    if stream != want:
        a, b = np.frombuffer(stream, np.uint8), np.frombuffer(want, np.uint8)
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"stream differs from the model at byte {i} (row {i // (n + 1)}, column {i % (n + 1) - 1}): "
                             f"{a[i]} != {b[i]}")
    back = unfilter_stream(stream, H, n, bpp)
    assert np.array_equal(back, rows), "unfiltered pixels differ from the input"
    return stream


def check_pillow(png: bytes, px):
    """Where Pillow is installed: it must read the same pixels and mode."""
    import io

    import pytest

    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(bytes(png)))
    im.load()
    modes = {"RGB"} if px.ndim == 3 else ({"L"} if px.dtype == np.uint8 else {"I;16", "I;16B", "I"})
    assert im.mode in modes, im.mode
    got = np.asarray(im)
    assert got.shape == px.shape
    assert np.array_equal(got.astype(np.int64), px.astype(np.int64))


# ---- test images ------------------------------------------------------------------------------
def runny(seed, shape, dtype=np.uint8, p_new=0.35):
    """Skewed values in runs of geometric length: literals, runs and a Huffman code that pays."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    top = 255 if dtype == np.uint8 else 65535
    vals = np.minimum(rng.geometric(0.08, n) * (1 if dtype == np.uint8 else 97), top).astype(dtype)
    new = rng.random(n) < p_new
    new[0] = True
    idx = np.maximum.accumulate(np.where(new, np.arange(n), 0))
    return vals[idx].reshape(shape)


# (name, kind, H, W): kind "gray" uint8 [H, W], "bgr" uint8 [H, W, 3], "u16" uint16 [H, W].
# W*bpp + 1 divides 32768 only for odd W*bpp, so rows land on segment boundaries in gray and BGR
# (3 * 5461 + 1 = 16384) and never in uint16 (2 * W + 1 is odd): there the nearest width stands in.
# Likewise a uint16 stream is never exactly 32768 bytes.
SHAPES = [
    ("1x1", "gray", 1, 1), ("1x1", "bgr", 1, 1), ("1x1", "u16", 1, 1),
    ("1xW", "gray", 1, 37), ("1xW", "bgr", 1, 37), ("1xW", "u16", 1, 37),
    ("Hx1", "gray", 29, 1), ("Hx1", "bgr", 29, 1), ("Hx1", "u16", 29, 1),
    ("rows_on_boundaries", "gray", 3, 32767), ("rows_on_boundaries", "bgr", 5, 5461), ("near_boundaries", "u16", 3, 16383),
    ("cuts_mid_row", "gray", 5, 13107), ("cuts_mid_row", "bgr", 5, 4369), ("cuts_mid_row", "u16", 5, 6553),
    ("one_segment", "gray", 8, 4095), ("one_segment", "bgr", 32, 341),
    ("one_segment_plus_1", "gray", 1, 32768), ("one_segment_plus_1", "bgr", 99, 110), ("one_segment_plus_1", "u16", 1, 16384),
    ("37x67", "gray", 37, 67), ("37x67", "bgr", 37, 67), ("37x67", "u16", 37, 67),
    ("41x53", "gray", 41, 53), ("41x53", "bgr", 41, 53), ("41x53", "u16", 41, 53),
]


def shape_image(kind, H, W, seed=0, random=False):
    shape = (H, W, 3) if kind == "bgr" else (H, W)
    dtype = np.uint16 if kind == "u16" else np.uint8
    if random:
        rng = np.random.default_rng(seed)
        return rng.integers(0, 65536 if kind == "u16" else 256, shape).astype(dtype)
    return runny(seed, shape, dtype)


def one_row(values):
    """A one-row gray image; with filter 0 its stream is a 0 byte and then these bytes."""
    return np.asarray(values, np.uint8).reshape(1, -1)


def repeat_blocks(blocks, seed=0):
    """A row of runs: for every R in blocks, R + 1 equal bytes (one literal and R repeating
    positions), neighbouring runs of different values, the first one not 0 (the filter byte)."""
    rng = np.random.default_rng(seed)
    out, prev = [], 0
    for R in blocks:
        v = int(rng.integers(1, 256))
        while v == prev:
            v = int(rng.integers(1, 256))
        out += [v] * (R + 1)
        prev = v
    return one_row(out)


def skewed_no_neighbours(counts, first=1):
    """Bytes first, first + 1, ... with these counts, arranged so that no two neighbours are
    equal (the largest count is at most half): even positions first, then the odd ones."""
    n = int(sum(counts))
    assert max(counts) <= (n + 1) // 2
    order = np.argsort(-np.asarray(counts), kind="stable")
    vals = np.concatenate([np.full(counts[k], first + k, np.uint8) for k in order])
    arr = np.empty(n, np.uint8)
    pos = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    arr[pos] = vals
    assert (arr[1:] != arr[:-1]).all()
    return one_row(arr)


def deep_tree_counts(limit=SEG - 1):
    """Byte counts whose Huffman tree is deeper than 15 however ties are broken, in one segment.
    With the filter byte and the end-of-block symbol (once each) there are ten symbols of count 1;
    they merge among themselves first (weight 10, at least four levels).  Every later count is
    larger than everything merged so far, a(k+2) = 10 + a(1) + ... + a(k) + 1, so each one adds a
    level: the growth of the Fibonacci sequence, the slowest that forces a chain.  F(1..24) itself
    sums to 121392, more than a segment holds; this sequence reaches 24 values within 32767 bytes."""
    counts = [1] * 8
    chain = [11, 11]
    while True:
        nxt = 10 + sum(chain[:-1]) + 1
        if sum(counts) + sum(chain) + nxt > limit:
            break
        chain.append(nxt)
    return counts + chain
