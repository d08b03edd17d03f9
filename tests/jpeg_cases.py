"""Files the JPEG decoder's tests share (host twin, device, sanitizer program): the geometry grid,
handmade streams from jpeg_np's coefficient-level writer, refused and corrupt files, and files
whose scan has a chosen sub-sequence structure.  Everything is made from seeds; nothing needs
Pillow."""
import functools
import os

import numpy as np

import jpeg_np as J

SUBSEQ = 128  # csrc/sm_jpegdec.hpp JD_SUBSEQ
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg", "pillow.npz")

SAMPLINGS = {"gray": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}
GRID_W = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
GRID_H = (1, 2, 7, 8, 9, 16, 17, 31)


def grid_file(samp, W, H, quality=75, ri=0):
    img = J.test_image(W * 100 + H, H, W, 1 if samp is None else 3)
    return J.encode_image(img, quality, samp or (1, 1), ri)


@functools.lru_cache(None)
def pillow_fixtures():
    z = np.load(GOLDEN)
    names = sorted(k[:-6] for k in z.files if k.endswith("__file"))
    return {n: (z[n + "__file"].tobytes(), z[n + "__rgb"], z[n + "__y"]) for n in names}


def scan_range(data):
    return J.parse(data)["scan"]


def n_subsequences(data):
    return sum(max(1, -(-(e - b) // SUBSEQ)) for b, e in J.scan_intervals(data)[0])


# ---- handmade streams ----------------------------------------------------------------------------
def _blocks(seed, shape, nnz, amp):
    """random quantised blocks: nnz coefficients of up to +-amp each"""
    rng = np.random.RandomState(seed)
    c = np.zeros(shape + (64,), np.int64)
    flat = c.reshape(-1, 64)
    for b in flat:
        idx = rng.choice(64, nnz, replace=False)
        b[idx] = rng.randint(-amp, amp + 1, nnz)
    return c


@functools.lru_cache(None)
def handmade():
    out = {}
    q8 = [np.full(64, 3, np.int64)]
    # every code 16 bits long
    c = [_blocks(1, (2, 3), 6, 7)]
    ac_syms = sorted({0x00, 0xF0} | {(r << 4) | s for r in range(16) for s in range(1, 4)})
    t16 = lambda syms: J.huff_table([0] * 15 + [len(syms)], syms)
    out["codes16"] = J.write_jpeg(c, q8, 16, 24, dc_tables=[t16(list(range(12)))] * 2, ac_tables=[t16(ac_syms)] * 2)
    # ZRL runs and blocks that end at index 63 without EOB
    c = [np.zeros((2, 2, 64), np.int64)]
    c[0][0, 0, J.ZIGZAG[40]] = 5
    c[0][0, 0, J.ZIGZAG[63]] = -2
    c[0][0, 1, J.ZIGZAG[63]] = 1
    c[0][1, 0, J.ZIGZAG[17]] = -9
    c[0][1, 1, J.ZIGZAG[16]] = 3
    c[0][1, 1, J.ZIGZAG[48]] = 3
    c[0][:, :, 0] = [[10, -10], [0, 100]]
    out["zrl_and_63"] = J.write_jpeg(c, q8, 16, 16)
    # coefficients no encoder makes, times a 16-bit quantiser
    c = [_blocks(2, (2, 2), 10, 32767) for _ in range(3)]
    for k in c:
        k[..., 0] = np.array([[32767, 0], [-32767, 0]])
    qw = [np.full(64, 65535, np.int64), np.arange(64, dtype=np.int64) * 1000 + 1]
    out["wild"] = J.write_jpeg(c, qw, 16, 16, (1, 1))
    c = [_blocks(3, (2, 2), 8, 40), _blocks(4, (1, 1), 8, 40), _blocks(5, (1, 1), 8, 40)]
    out["wild_420"] = J.write_jpeg([k * 800 for k in c], qw, 13, 11, (2, 2), ri=1)
    # a 16-bit quantiser with ordinary coefficients, SOF1, APPn / COM segments, fill bytes
    c = [_blocks(6, (3, 2), 5, 3)]
    out["dqt16"] = J.write_jpeg(c, [np.arange(64, dtype=np.int64) * 7 + 200], 20, 12)
    extra = J._seg(0xE1, b"Exif\0\0" + bytes(40)) + b"\xff\xff" + J._seg(0xFE, b"a comment") + J._seg(0xEC, b"x")
    out["sof1_app_com_fill"] = J.write_jpeg(c, q8, 20, 12, sof=0xC1, extra=extra, ri=2, fill_before_markers=2)
    # Adobe marker with transform 1 (YCbCr) and no JFIF
    adobe = lambda tf: J._seg(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([tf]))
    c3 = [_blocks(7, (2, 2), 6, 20), _blocks(8, (2, 1), 6, 20), _blocks(9, (2, 1), 6, 20)]
    out["adobe_ycc_422"] = J.write_jpeg(c3, q8 * 2, 12, 14, (2, 1), jfif=False, extra=adobe(1))
    return out


# ---- refused and corrupt files: name -> (bytes, SM_E_* code, part of the message) --------------------
def _patch(data, at, new):
    b = bytearray(data)
    b[at:at + len(new)] = new
    return bytes(b)


def _index_overrun_file():
    """one gray block whose AC run passes index 63"""
    ac = J.default_table(J.ac_symbols())
    dc = J.default_table(range(16))
    bw = J._BitWriter()
    bw.put(*dc["enc"][0])
    for _ in range(3):
        bw.put(*ac["enc"][0xF0])          # 48 zeros: z = 49
    bw.put(*ac["enc"][0xF1])              # run 15, size 1: index 64
    bw.put(1, 1)
    bw.flush()
    return J.write_jpeg([np.zeros((1, 1, 64), np.int64)], [np.ones(64, np.int64)], 8, 8, dc_tables=[dc] * 2,
                        ac_tables=[ac] * 2, scan=bytes(bw.out))


@functools.lru_cache(None)
def faulty():
    U, D = J.SM_E_UNSUPPORTED, J.SM_E_DATA
    img = J.test_image(11, 24, 40, 3)
    base = J.encode_image(img, 75, (1, 1))
    rst = J.encode_image(img, 75, (2, 2), ri=1)
    gray = J.encode_image(img[:, :, 0], 75)
    sof = base.index(b"\xff\xc0")
    b0, e0 = scan_range(base)
    br, er = scan_range(rst)
    first_rst = rst.index(b"\xff\xd0", br)
    dri = rst.index(b"\xff\xdd")
    dqt = base.index(b"\xff\xdb")
    adobe0 = J._seg(0xEE, b"Adobe\0\x64\0\0\0\0\0")
    coefs, qts = J.image_coefficients(img, 75, (1, 1))
    out = {
        "progressive": (_patch(base, sof + 1, b"\xc2"), U, "progressive"),
        "arithmetic": (_patch(base, sof + 1, b"\xc9"), U, "arithmetic"),
        "twelve_bit": (_patch(base, sof + 4, b"\x0c"), U, "12-bit"),
        "two_scans": (base[:-2] + base[base.index(b"\xff\xda"):b0] + base[b0:], U, "several scans"),
        "sampling_440": (_patch(base, sof + 11, b"\x12"), U, "sampling"),
        "sampling_411": (_patch(base, sof + 11, b"\x41"), U, "sampling"),
        "four_components": (_patch(base, sof + 9, b"\x04"), U, "4 components"),
        "adobe_rgb": (J.write_jpeg(coefs, qts, 24, 40, jfif=False, extra=adobe0), U, "not YCbCr"),
        "rgb_ids": (J.write_jpeg(coefs, qts, 24, 40, jfif=False, comp_ids=[82, 71, 66]), U, "not YCbCr"),
        "dnl_height_0": (_patch(base, sof + 5, b"\0\0"), U, "DNL"),
        "dnl_marker": (base[:-2] + b"\xff\xdc\0\x04\0\x18\xff\xd9", U, "DNL"),
        "truncated_header": (base[:sof + 6], D, "truncated file"),
        "truncated_scan": (base[:(b0 + e0) // 2], D, "truncated file"),
        "short_scan": (base[:(b0 + e0) // 2] + b"\xff\xd9", D, "ends before the last block"),
        "bad_code": (_patch(base, b0, b"\xff\x00\xff\x00\xff\x00"), D, "in no table"),
        "index_past_63": (_index_overrun_file(), D, "index past 63"),
        "rst_out_of_sequence": (_patch(rst, first_rst + 1, b"\xd3"), D, "restart markers"),
        "rst_missing": (_patch(rst, dri + 4, b"\0\x02"), D, "restart markers"),
        "rst_unexpected": (rst[:dri] + rst[dri + 6:], D, "restart markers"),
        "leftover": (gray[:-2] + b"\x12\x34\x56\xff\xd9", D, "left over"),
        "segment_length": (_patch(base, dqt + 2, b"\0\x30"), D, "segment length"),
        "no_eoi": (base[:-2] + b"\xff\xe0\0\x02", D, "not followed by EOI"),
        "no_table": (base[:dqt] + base[dqt + 2 + 67:], D, "not defined"),
        "garbage": (b"\xff\xd8\xff\x00garbage", D, "marker"),
    }
    return out


# the corrupt files the device tests replay (the host tests show the twin rejecting each cleanly).
# "truncated_scan" (no EOI) is refused by the host parser, which finds no end of the scan, before any
# kernel runs; "short_scan" (the scan cut, then EOI) is the truncation that reaches the kernels.  Both
# are replayed.
DEVICE_FAULTY = ("truncated_scan", "short_scan", "bad_code", "index_past_63", "rst_out_of_sequence", "rst_missing", "leftover")


# ---- scans of a chosen structure ------------------------------------------------------------------------
@functools.lru_cache(None)
def scan_of_length(nbytes, seed=0):
    """a gray file whose scan has exactly nbytes bytes (small scans): +-1 coefficients are added
    one at a time"""
    assert nbytes <= 512
    rng = np.random.RandomState(seed)
    nb = max(1, nbytes // 24)
    c = np.zeros((1, nb, 64), np.int64)
    q = [np.full(64, 2, np.int64)]
    for _ in range(4000):
        data = J.write_jpeg([c], q, 8, 8 * nb)
        b, e = scan_range(data)
        if e - b == nbytes:
            return data
        if e - b > nbytes:
            c[0, rng.randint(nb)] = 0
        c[0, rng.randint(nb), rng.randint(1, 64)] = rng.choice([-1, 1])
    raise AssertionError("no scan of that length found")


@functools.lru_cache(None)
def scan_of_lanes(lanes, seed=0):
    """a gray noise file without restart markers whose scan takes exactly `lanes` sub-sequences:
    trailing blocks lose their AC coefficients until it does (bisection)"""
    rng = np.random.RandomState(seed)
    nb = lanes * SUBSEQ // 40 + 8
    img = np.clip(rng.normal(128, 50, (8, 8 * nb)), 0, 255).astype(np.uint8)
    (c,), q = J.image_coefficients(img, 90)

    def make(k):
        d = c.copy()
        if k:
            d[0, nb - k:, 1:] = 0
        data = J.write_jpeg([d], q, 8, 8 * nb)
        return data, n_subsequences(data)

    lo, hi = 0, nb
    assert make(lo)[1] >= lanes >= make(hi)[1], (make(lo)[1], make(hi)[1])
    while True:
        mid = (lo + hi) // 2
        data, n = make(mid)
        if n == lanes:
            return data
        assert hi - lo > 1, "no scan of that many lanes found"
        if n > lanes:
            lo = mid
        else:
            hi = mid


@functools.lru_cache(None)
def noise_file(seed, H, W, samp=None, ri=0, quality=90):
    rng = np.random.RandomState(seed)
    shape = (H, W) if samp is None else (H, W, 3)
    img = np.clip(rng.normal(128, 50, shape), 0, 255).astype(np.uint8)
    return J.encode_image(img, quality, samp or (1, 1), ri)


def cut_on_stuffing(data):
    """whether a sub-sequence cut of the file's first interval falls on the 00 of an FF 00 pair"""
    (b, e), = J.scan_intervals(data)[0][:1]
    d = J.parse(data)["data"]
    return any(d[p - 1] == 0xFF and d[p] == 0 for p in range(b + SUBSEQ, e, SUBSEQ))


@functools.lru_cache(None)
def interval_of_length(nbytes, seed=0):
    """a gray file of two restart intervals (a block row each) whose first interval has exactly
    nbytes bytes: with nbytes = SUBSEQ + 1 a cut falls one byte before RST0"""
    rng = np.random.RandomState(seed)
    nb = max(1, nbytes // 24)
    c = np.zeros((2, nb, 64), np.int64)
    c[1] = _blocks(seed, (nb,), 5, 3)
    q = [np.full(64, 2, np.int64)]
    for _ in range(4000):
        data = J.write_jpeg([c], q, 16, 8 * nb, ri=nb)
        b, e = J.scan_intervals(data)[0][0]
        if e - b == nbytes:
            return data
        if e - b > nbytes:
            c[0, rng.randint(nb)] = 0
        c[0, rng.randint(nb), rng.randint(1, 64)] = rng.choice([-1, 1])
    raise AssertionError("no interval of that length found")


@functools.lru_cache(None)
def stuffing_file():
    """the first seed whose noise file has a sub-sequence cut on the 00 of an FF 00 pair"""
    for seed in range(400):
        data = noise_file(seed, 32, 64)
        if cut_on_stuffing(data):
            return data
    raise AssertionError("no seed found")


@functools.lru_cache(None)
def identical_blocks(nblocks=256):
    """a long run of identical blocks: a lane that starts at a wrong bit can stay in a wrong but
    valid phase for many sub-sequences, so the states settle lane after lane"""
    c = np.zeros((1, nblocks, 64), np.int64)
    c[0, :, 0] = 3
    c[0, :, [1, 2, 9, 17, 30]] = np.array([2, -1, 1, 1, -1])[:, None]
    return J.write_jpeg([c], [np.full(64, 4, np.int64)], 8, 8 * nblocks)
