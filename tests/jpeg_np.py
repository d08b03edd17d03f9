"""Baseline JPEG in numpy: the oracle of the JPEG decoder, written from the
standard and libjpeg's documented arithmetic, independently of csrc/sm_jpegdec.hpp.

* :func:`decode` -- parser, serial Huffman decode, dequantisation, the ``jidctint`` islow IDCT,
  ``jdsample``'s fancy (triangle) upsampling and ``jdcolor``'s YCbCr tables; ``flags`` as
  ``cv2.imread``.  A file the package refuses raises :class:`JpegError` with ``code`` -4
  (unsupported) or -5 (data) and a short ``kind``.
* :func:`write_jpeg` -- a baseline writer at coefficient level: quantised coefficients, tables,
  sampling and restart interval in, a file out.  :func:`image_coefficients` makes coefficients from
  an image (float DCT; the files only have to be valid), :func:`huff_table` any prefix code.

Intermediate arithmetic is 64-bit; the IDCT's workspace wraps to int32, as the C++ states.
"""
import numpy as np

SM_E_UNSUPPORTED, SM_E_DATA = -4, -5


class JpegError(Exception):
    def __init__(self, code, kind):
        super().__init__(f"{'unsupported' if code == SM_E_UNSUPPORTED else 'data'}: {kind}")
        self.code, self.kind = code, kind


def _unsup(kind):
    raise JpegError(SM_E_UNSUPPORTED, kind)


def _bad(kind):
    raise JpegError(SM_E_DATA, kind)


def _zigzag():
    """natural index of zigzag position k, walked along the anti-diagonals"""
    out = []
    for s in range(15):
        cells = [(i, s - i) for i in range(8) if 0 <= s - i < 8]   # (row, col)
        if s % 2 == 0:
            cells.reverse()                                       # even diagonals run upwards
        out += [r * 8 + c for r, c in cells]
    return np.array(out)


ZIGZAG = _zigzag()


# ---- parser -----------------------------------------------------------------------------------
def parse(data):
    d = bytes(data)
    n = len(d)
    if n < 3 or d[0] != 0xFF or d[1] != 0xD8 or d[2] != 0xFF:
        _bad("signature")
    pos = 2
    qt, huff = {}, {}
    frame, ri, jfif, adobe = None, 0, False, None
    while True:
        if pos + 2 > n:
            _bad("truncated")
        if d[pos] != 0xFF:
            _bad("marker")
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            _bad("truncated")
        m = d[pos]
        pos += 1
        if m == 0xD8 or m <= 0x01 or 0xD0 <= m <= 0xD7:
            _bad("marker")
        if m == 0xD9:
            _bad("noscan")
        if pos + 2 > n:
            _bad("truncated")
        L = d[pos] << 8 | d[pos + 1]
        if L < 2:
            _bad("length")
        if pos + L > n:
            _bad("truncated")
        seg = d[pos + 2:pos + L]
        pos += L
        if m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            _unsup("process")
        if m == 0xDC:
            _unsup("dnl")
        if m in (0xC0, 0xC1):
            if frame is not None:
                _bad("sof")
            if len(seg) < 6:
                _bad("length")
            prec, H, W, nc = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if prec == 12:
                _unsup("precision")
            if prec != 8:
                _bad("sof")
            if H == 0:
                _unsup("dnl")
            if W == 0:
                _bad("sof")
            if nc == 4:
                _unsup("components")
            if nc not in (1, 3):
                _unsup("components")
            if len(seg) != 6 + 3 * nc:
                _bad("length")
            comps = []
            for c in range(nc):
                cid, hv, tq = seg[6 + 3 * c:9 + 3 * c]
                h, v = hv >> 4, hv & 15
                if not (1 <= h <= 4 and 1 <= v <= 4) or tq > 3:
                    _bad("sof")
                comps.append(dict(id=cid, h=h, v=v, tq=tq))
            frame = dict(H=H, W=W, comps=comps)
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                if pq > 1 or tq > 3:
                    _bad("dqt")
                sz = 64 * (pq + 1)
                if p + 1 + sz > len(seg):
                    _bad("length")
                v = np.frombuffer(seg[p + 1:p + 1 + sz], np.uint8 if pq == 0 else ">u2").astype(np.int64)
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = v
                qt[tq] = t
                p += 1 + sz
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    _bad("length")
                tc, th = seg[p] >> 4, seg[p] & 15
                if tc > 1 or th > 3:
                    _bad("dht")
                bits = list(seg[p + 1:p + 17])
                cnt = sum(bits)
                if cnt > 256 or p + 17 + cnt > len(seg):
                    _bad("length" if cnt <= 256 else "dht")
                vals = list(seg[p + 17:p + 17 + cnt])
                code, table = 0, {}
                k = 0
                for ln in range(1, 17):
                    for _ in range(bits[ln - 1]):
                        if code >= (1 << ln):
                            _bad("dht")
                        table[(ln, code)] = vals[k]
                        k += 1
                        code += 1
                    code <<= 1
                if tc == 0 and any(s > 15 for s in vals):
                    _bad("dht")
                huff[(tc, th)] = table
                p += 17 + cnt
        elif m == 0xDD:
            if len(seg) != 2:
                _bad("length")
            ri = seg[0] << 8 | seg[1]
        elif m == 0xE0:
            if len(seg) >= 5 and seg[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                _bad("sos")
            if len(seg) < 1:
                _bad("length")
            ns = seg[0]
            if len(seg) != 4 + 2 * ns or ns < 1 or ns > 4:
                _bad("length")
            nc = len(frame["comps"])
            if ns != nc:
                _unsup("scans")
            for c in range(nc):
                cid, tt = seg[1 + 2 * c], seg[2 + 2 * c]
                if cid != frame["comps"][c]["id"]:
                    _bad("sos")
                frame["comps"][c]["td"], frame["comps"][c]["ta"] = tt >> 4, tt & 15
                if (tt >> 4) > 3 or (tt & 15) > 3:
                    _bad("sos")
            if seg[1 + 2 * ns] != 0 or seg[2 + 2 * ns] != 63 or seg[3 + 2 * ns] != 0:
                _bad("sos")
            break
        # APPn, COM and the rest: skipped
    comps = frame["comps"]
    nc = len(comps)
    if nc == 3:
        ids = tuple(c["id"] for c in comps)
        if not jfif:
            if adobe is not None:
                if adobe == 0:
                    _unsup("colorspace")
            elif ids == (ord("R"), ord("G"), ord("B")):
                _unsup("colorspace")
        s = (comps[0]["h"], comps[0]["v"])
        if s not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
            _unsup("sampling")
    else:
        comps[0]["h"] = comps[0]["v"] = 1
    for c in comps:
        if c["tq"] not in qt:
            _bad("notable")
        if (0, c["td"]) not in huff or (1, c["ta"]) not in huff:
            _bad("notable")
    # the end of the scan: the first marker that is neither a stuffed FF nor RSTn
    p = pos
    end = None
    while p < n:
        if d[p] != 0xFF:
            p += 1
            continue
        q = p
        while q < n and d[q] == 0xFF:
            q += 1
        if q >= n:
            break
        if q == p + 1 and d[q] == 0:
            p = q + 1
            continue
        if 0xD0 <= d[q] <= 0xD7:
            p = q + 1
            continue
        if d[q] == 0:       # FF FF 00: the first FF is data, the pair a stuffed FF
            p = q + 1
            continue
        end = p
        mk = d[q]
        break
    if end is None:
        _bad("truncated")
    if mk == 0xDC:
        _unsup("dnl")
    if mk in (0xDA, 0xC4, 0xDB, 0xDD):
        _unsup("scans")
    if mk != 0xD9:
        _bad("noeoi")
    hmax, vmax = comps[0]["h"], comps[0]["v"]
    frame.update(qt=qt, huff=huff, ri=ri, scan=(pos, end), data=d, hmax=hmax, vmax=vmax,
                 mcux=-(-frame["W"] // (8 * hmax)), mcuy=-(-frame["H"] // (8 * vmax)))
    return frame


def info(data):
    """(H, W, channels, subsampling): subsampling 0 gray, 444, 422 or 420"""
    f = parse(data)
    c = f["comps"]
    sub = 0 if len(c) == 1 else {(1, 1): 444, (2, 1): 422, (2, 2): 420}[(c[0]["h"], c[0]["v"])]
    return f["H"], f["W"], len(c), sub


def scan_intervals(data):
    """[(begin, end)] byte ranges of the restart intervals' entropy data, and the markers' numbers"""
    f = parse(data)
    d, (b, e) = f["data"], f["scan"]
    out, nums, at = [], [], b
    p = b
    while p + 1 < e:
        if d[p] == 0xFF and 0xD0 <= d[p + 1] <= 0xD7:
            out.append((at, p))
            nums.append(d[p + 1] - 0xD0)
            at = p + 2
            p += 2
        else:
            p += 1
    out.append((at, e))
    return out, nums


# ---- entropy decode ----------------------------------------------------------------------------
class _Bits:
    def __init__(self, raw):
        # trailing fill bytes (FF before a marker) are no data
        b = bytearray()
        i, n = 0, len(raw)
        while i < n:
            c = raw[i]
            b.append(c)
            i += 2 if (c == 0xFF and i + 1 < n and raw[i + 1] == 0) else 1
        self.b, self.n, self.pos = bytes(b), len(b) * 8, 0

    def peek(self, k):
        """k bits, zeros past the end"""
        i, off = self.pos >> 3, self.pos & 7
        chunk = int.from_bytes(self.b[i:i + 5].ljust(5, b"\0"), "big")
        return (chunk >> (40 - off - k)) & ((1 << k) - 1)

    def take(self, k):
        v = self.peek(k) if k else 0
        self.pos += k
        return v


def _symbol(br, table):
    v = br.peek(16)
    for ln in range(1, 17):
        s = table.get((ln, v >> (16 - ln)))
        if s is not None:
            br.pos += ln
            return s
    _bad("code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def decode_coefficients(f):
    """per component: int16 [blocks down, blocks across, 64] in natural order, padded to whole MCUs"""
    comps = f["comps"]
    mcux, mcuy, ri = f["mcux"], f["mcuy"], f["ri"]
    nmcu = mcux * mcuy
    coefs = [np.zeros((mcuy * c["v"], mcux * c["h"], 64), np.int64) for c in comps]
    ivals, nums = scan_intervals(f["data"])
    nint = -(-nmcu // ri) if ri else 1
    if len(ivals) != nint or any(x != (k & 7) for k, x in enumerate(nums)):
        _bad("rst")
    d = f["data"]
    for k, (b, e) in enumerate(ivals):
        br = _Bits(d[b:e])
        pred = [0] * len(comps)
        first = k * ri if ri else 0
        last = min(first + ri, nmcu) if ri else nmcu
        for m in range(first, last):
            my, mx = divmod(m, mcux)
            for ci, c in enumerate(comps):
                dct, act = f["huff"][(0, c["td"])], f["huff"][(1, c["ta"])]
                for by in range(c["v"]):
                    for bx in range(c["h"]):
                        blk = coefs[ci][my * c["v"] + by, mx * c["h"] + bx]
                        s = _symbol(br, dct)
                        pred[ci] += _extend(br.take(s), s)
                        blk[0] = pred[ci]
                        z = 1
                        while z < 64:
                            rs = _symbol(br, act)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                if z + 16 > 64:
                                    _bad("index")
                                z += 16
                                continue
                            z += r
                            if z > 63:
                                _bad("index")
                            blk[ZIGZAG[z]] = _extend(br.take(s), s)
                            z += 1
                        if br.pos > br.n:
                            _bad("scan")
        # what is left: the padding of the last byte, then fill bytes only
        rest = br.b[(br.pos + 7) >> 3:]
        if any(x != 0xFF for x in rest):
            _bad("leftover")
    return [((c + 32768) % 65536 - 32768).astype(np.int16) for c in coefs]


# ---- IDCT (jidctint.c, jpeg_idct_islow) -----------------------------------------------------------
_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299,
          f1_847=15137, f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)


def _idct_1d(x, shift):
    """x: int64 [..., 8] along the last axis; the eight outputs before the range limit"""
    F = _F
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * F["f0_541"]
    tmp2 = z1 - z3 * F["f1_847"]
    tmp3 = z1 + z2 * F["f0_765"]
    tmp0 = (x[..., 0] + x[..., 4]) * 8192
    tmp1 = (x[..., 0] - x[..., 4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F["f1_175"]
    t0, t1, t2, t3 = t0 * F["f0_298"], t1 * F["f2_053"], t2 * F["f3_072"], t3 * F["f1_501"]
    z1, z2, z3, z4 = -z1 * F["f0_899"], -z2 * F["f2_562"], -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)
    return (out + (1 << (shift - 1))) >> shift


def range_limit(x):
    x = x & 1023
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))).astype(np.uint8)


def idct_blocks(coef, q):
    """coef int16 [..., 64] natural order, q [64]: uint8 [..., 8, 8]"""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    ws = _idct_1d(np.swapaxes(x, -1, -2), 11)              # columns: [..., col, row]
    ws = np.swapaxes(ws, -1, -2).astype(np.int32).astype(np.int64)
    return range_limit(_idct_1d(ws, 18))


def _plane(blocks):
    by, bx = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


# ---- upsampling (jdsample.c) and colour (jdcolor.c) -------------------------------------------------
def upsample_h2v1(p):
    """p int64 [rows, dw] -> [rows, 2 * dw]"""
    dw = p.shape[1]
    if dw <= 2:
        return np.repeat(p, 2, axis=1)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * dw), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def upsample_h2v2(p):
    """p int64 [dh, dw] (real rows and columns only) -> [2 * dh, 2 * dw]"""
    dh, dw = p.shape
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up = np.concatenate([p[:1], p[:-1]], 0)
    dn = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for v, far in ((0, up), (1, dn)):
        s = 3 * p + far
        last = np.concatenate([s[:, :1], s[:, :-1]], 1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        o = np.empty((dh, 2 * dw), np.int64)
        o[:, 0::2] = (3 * s + last + 8) >> 4
        o[:, 1::2] = (3 * s + nxt + 7) >> 4
        o[:, 0] = (4 * s[:, 0] + 8) >> 4
        o[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[v::2] = o
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = (np.asarray(a, np.int64) for a in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return tuple(np.clip(a, 0, 255).astype(np.uint8) for a in (r, g, b))


def decode(data, flags=1, keep_channel_order=False):
    f = parse(data)
    H, W, comps = f["H"], f["W"], f["comps"]
    coefs = decode_coefficients(f)
    gray_out = flags == 0 or (flags == -1 and len(comps) == 1)
    y = _plane(idct_blocks(coefs[0], f["qt"][comps[0]["tq"]]))[:H, :W]
    if gray_out:
        return y.copy()
    if len(comps) == 1:
        return np.repeat(y[:, :, None], 3, axis=2)
    hmax, vmax = f["hmax"], f["vmax"]
    dw, dh = -(-W // hmax), -(-H // vmax)
    ch = []
    for ci in (1, 2):
        p = _plane(idct_blocks(coefs[ci], f["qt"][comps[ci]["tq"]]))[:dh, :dw].astype(np.int64)
        if (hmax, vmax) == (2, 1):
            p = upsample_h2v1(p)
        elif (hmax, vmax) == (2, 2):
            p = upsample_h2v2(p)
        ch.append(p[:H, :W])
    r, g, b = ycc_to_rgb(y, ch[0], ch[1])
    return np.stack([r, g, b] if keep_channel_order else [b, g, r], axis=2)


# ---- writer ------------------------------------------------------------------------------------
def huff_table(bits, vals):
    """(bits[16], vals) as in a DHT segment -> the table; checks that it is a prefix code"""
    bits, vals = list(bits), list(vals)
    assert len(bits) == 16 and sum(bits) == len(vals) and len(set(vals)) == len(vals)
    code, k, enc = 0, 0, {}
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            assert code < (1 << ln), "not a prefix code"
            enc[vals[k]] = (code, ln)
            k += 1
            code += 1
        code <<= 1
    return dict(bits=bits, vals=vals, enc=enc)


def default_table(symbols, first_len=2):
    """a prefix code for ``symbols`` (most frequent first): a quarter of the free codes at every
    length, the rest at the last lengths; the all-ones code stays free"""
    symbols = list(symbols)
    bits, rem, avail = [0] * 16, len(symbols), 1 << first_len
    for ln in range(first_len, 17):
        left_levels = 16 - ln
        take = min(rem, max(1, avail // 4))
        if rem - take > (avail - take) * (1 << left_levels) - 1 or ln == 16:   # the rest must still fit
            take = min(rem, avail - 1)
        while take < rem and (avail - take) * (1 << left_levels) - 1 < rem - take:
            take += 1
        bits[ln - 1] = take
        rem -= take
        avail = (avail - take) * 2
    assert rem == 0
    return huff_table(bits, symbols)


def ac_symbols(max_size=10):
    """EOB, the short runs and sizes first, ZRL, then the rest"""
    head = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x12, 0x21, 0x31, 0x41, 0x05, 0x13, 0x51, 0x61, 0x22, 0x71, 0xF0]
    rest = [(r << 4) | s for s in range(1, max_size + 1) for r in range(16)]
    return head + [x for x in rest if x not in head]


STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def quality_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((t * s + 50) // 100, 1, 255) for t in (STD_LUMA_Q, STD_CHROMA_Q)]


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v):
    return int(abs(int(v))).bit_length()


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def write_jpeg(coefs, qts, H, W, sampling=(1, 1), ri=0, dc_tables=None, ac_tables=None, sof=0xC0,
               extra=b"", jfif=True, tq=None, comp_ids=None, fill_before_markers=0, scan=None):
    """A baseline file from quantised coefficients.

    coefs: per component an integer array [blocks down, blocks across, 64] in natural order, padded to
    whole MCUs; qts: quantisation tables in natural order (values above 255 are written as 16-bit
    entries), ``tq[c]`` the table of component c (default 0 for luma, 1 for chroma when there are
    two); sampling: the luma factors (h, v); dc_tables / ac_tables: one table (see
    :func:`default_table`) for luma and one for chroma, default codes that cover every symbol the
    coefficients need.  A block whose coefficient 63 is non-zero gets no EOB.  ``extra`` goes between
    the header segments (APPn / COM); ``fill_before_markers`` FF bytes go before every RSTn and EOI;
    ``scan`` replaces the entropy data (handmade streams)."""
    nc = len(coefs)
    coefs = [np.asarray(c, np.int64) for c in coefs]
    hs = [sampling[0]] + [1] * (nc - 1)
    vs = [sampling[1]] + [1] * (nc - 1)
    mcux, mcuy = -(-W // (8 * hs[0])), -(-H // (8 * vs[0]))
    for c in range(nc):
        assert coefs[c].shape == (mcuy * vs[c], mcux * hs[c], 64), (coefs[c].shape, (mcuy * vs[c], mcux * hs[c], 64))
    if tq is None:
        tq = [0] + [min(1, len(qts) - 1)] * (nc - 1)
    ids = comp_ids or list(range(1, nc + 1))
    max_ac = max(1, max(_size(c[..., 1:].max(initial=0)) for c in coefs), max(_size(c[..., 1:].min(initial=0)) for c in coefs))
    if dc_tables is None:
        dc_tables = [default_table(range(16))] * 2
    if ac_tables is None:
        ac_tables = [default_table(ac_symbols(max(10, max_ac)))] * 2
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    out += extra
    for i, q in enumerate(qts):
        q = np.asarray(q, np.int64)[ZIGZAG]
        if q.max() > 255:
            out += _seg(0xDB, bytes([0x10 | i]) + q.astype(">u2").tobytes())
        else:
            out += _seg(0xDB, bytes([i]) + q.astype(np.uint8).tobytes())
    out += _seg(sof, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
                + b"".join(bytes([ids[c], hs[c] << 4 | vs[c], tq[c]]) for c in range(nc)))
    ntab = 1 if nc == 1 else 2
    for i in range(ntab):
        out += _seg(0xC4, bytes([i]) + bytes(dc_tables[i]["bits"]) + bytes(dc_tables[i]["vals"]))
        out += _seg(0xC4, bytes([0x10 | i]) + bytes(ac_tables[i]["bits"]) + bytes(ac_tables[i]["vals"]))
    if ri:
        out += _seg(0xDD, ri.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([nc]) + b"".join(bytes([ids[c], (0x11 if c and ntab == 2 else 0)]) for c in range(nc))
                + bytes([0, 63, 0]))
    bw = _BitWriter()
    pred = [0] * nc
    nmcu = mcux * mcuy
    for m in range(nmcu):
        if ri and m and m % ri == 0:
            bw.flush()
            bw.out += b"\xff" * fill_before_markers + bytes([0xFF, 0xD0 + ((m // ri - 1) & 7)])
            pred = [0] * nc
        my, mx = divmod(m, mcux)
        for c in range(nc):
            dct, act = dc_tables[min(c, 1) if ntab == 2 else 0]["enc"], ac_tables[min(c, 1) if ntab == 2 else 0]["enc"]
            for by in range(vs[c]):
                for bx in range(hs[c]):
                    blk = coefs[c][my * vs[c] + by, mx * hs[c] + bx][ZIGZAG]
                    diff = int(blk[0]) - pred[c]
                    diff = (diff + 32768) % 65536 - 32768 if abs(diff) > 32767 else diff
                    pred[c] = int(blk[0])
                    s = _size(diff)
                    bw.put(*dct[s])
                    if s:
                        bw.put(diff if diff >= 0 else diff + (1 << s) - 1, s)
                    run = 0
                    nz = np.nonzero(blk[1:])[0]
                    lastnz = int(nz[-1]) + 1 if nz.size else 0
                    for z in range(1, lastnz + 1):
                        v = int(blk[z])
                        if v == 0:
                            run += 1
                            continue
                        while run > 15:
                            bw.put(*act[0xF0])
                            run -= 16
                        s = _size(v)
                        bw.put(*act[run << 4 | s])
                        bw.put(v if v >= 0 else v + (1 << s) - 1, s)
                        run = 0
                    if lastnz < 63:
                        bw.put(*act[0x00])
    bw.flush()
    out += (bw.out if scan is None else scan) + b"\xff" * fill_before_markers + b"\xff\xd9"
    return bytes(out)


def _dct_matrix():
    k = np.arange(8)
    c = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    c[0] /= np.sqrt(2)
    return c


def image_coefficients(img, quality=75, sampling=(1, 1)):
    """(coefs, qts) of an image, uint8 [H, W] or RGB [H, W, 3], for :func:`write_jpeg`"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    qts = quality_tables(quality)
    if img.ndim == 2:
        planes, fac = [img.astype(np.float64)], [(1, 1)]
        qts = qts[:1]
    else:
        r, g, b = (img[..., i].astype(np.float64) for i in range(3))
        y = 0.299 * r + 0.587 * g + 0.114 * b
        planes = [y, 128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b]
        fac = [(1, 1), sampling, sampling]
    mcux, mcuy = -(-W // (8 * sampling[0])), -(-H // (8 * sampling[1]))
    C = _dct_matrix()
    coefs = []
    for i, (p, (fh, fv)) in enumerate(zip(planes, fac)):
        ph, pw = mcuy * 8 * sampling[1], mcux * 8 * sampling[0]
        p = np.pad(p, ((0, ph - H), (0, pw - W)), mode="edge")
        if (fh, fv) != (1, 1):
            p = p.reshape(ph // fv, fv, pw // fh, fh).mean(axis=(1, 3))
        bh, bw_ = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(bh, 8, bw_, 8).transpose(0, 2, 1, 3) - 128.0
        d = np.einsum("ij,abjk,lk->abil", C, blocks, C)
        q = qts[min(i, len(qts) - 1)].reshape(8, 8)
        coefs.append(np.rint(d / q).astype(np.int64).reshape(bh, bw_, 64))
    return coefs, qts


def test_image(seed, H, W, channels=3):
    """a synthetic picture with smooth parts, edges and noise"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for c in range(channels):
        a, b, ph = rng.uniform(0.05, 0.6, 3)
        p = 128 + 70 * np.sin(a * xx + ph * 5) * np.cos(b * yy + c) + 40 * ((xx // 5 + yy // 3 + c) % 2)
        p += rng.normal(0, 12, (H, W))
        out.append(np.clip(p, 0, 255))
    img = np.stack(out, 2).astype(np.uint8)
    return img[:, :, 0] if channels == 1 else img


def encode_image(img, quality=75, sampling=(1, 1), ri=0, **kw):
    """a file of ``img`` (uint8 gray or RGB) by this module's own writer"""
    coefs, qts = image_coefficients(img, quality, sampling)
    H, W = np.asarray(img).shape[:2]
    return write_jpeg(coefs, qts, H, W, sampling if np.asarray(img).ndim == 3 else (1, 1), ri, **kw)
