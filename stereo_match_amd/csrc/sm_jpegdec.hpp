// sm_jpegdec.hpp — baseline JPEG input on the device: cv2.imread(".jpg") of the
// reference's production flow (build_npz.py:229, io_functions.py:92, try_try.py:56-57).
//
// The arithmetic is libjpeg-turbo's defaults restated once, as __host__ __device__ functions the
// kernels and the CPU twin (jpegdec_host) share: integer dequantisation, the islow 8x8 IDCT of
// jidctint.c (CONST_BITS 13, PASS1_BITS 2, columns then rows), jdsample.c's fancy (triangle)
// upsampling for h2v1 and h2v2 (plain replication at a downsampled width of 1 or 2), jdcolor.c's
// YCbCr tables.  Intermediate arithmetic is 64-bit (jd_long; libjpeg's JLONG is 64-bit on Linux)
// and the IDCT's workspace wraps to int32 (libjpeg's `int workspace[]`): no encoder-made file
// comes near either limit, and for coefficients no encoder makes (+-32767 times a 16-bit
// quantiser) the device, the twin and tests/jpeg_np.py still agree bit for bit without undefined
// behaviour.  Nothing is claimed against libjpeg for such files.
//
// Stages (kernels at the end of the file, launched from sm_api.hip):
//   host          jd_parse: the segments before the scan into a JdDesc (geometry, sampling, the
//                 components' quantisation and Huffman tables as maxcode / valoff / huffval plus a
//                 9-bit look-ahead, restart interval, the scan's byte range).  The host reads
//                 entropy-coded bytes only to find the marker that ends the scan.
//   k_jpeg_split  the descriptor checked against the stated geometry; a byte-parallel search for
//                 FF D0..D7 in the scan, compacted into the restart intervals' byte ranges; their
//                 count must be ceil(MCUs / Ri) and the numbers must run modulo 8.  Each interval
//                 is cut into sub-sequences of JD_SUBSEQ raw bytes, one lane each.
//   k_jpeg_sync_a every lane decodes its sub-sequence from the guessed state (bit 0 of its first
//                 byte, block 0 of the MCU, zigzag index 0; a cut on the 00 of an FF 00 pair steps
//                 over it) and records the state in which it leaves: the bit position of the first
//                 symbol that starts at or past its end, the block within the MCU, the zigzag
//                 index, and the blocks it completed.  The first lane of an interval starts from
//                 the true state.
//   k_jpeg_sync_b / k_jpeg_sync_loop
//                 a lane whose predecessor left in another state than the one it last started
//                 from decodes again from that state: once grid-wide, then in one workgroup per
//                 image until no lane changes (at most as many rounds as there are lanes).  By
//                 induction from each interval's first lane the fixed point is the serial decode.
//                 In these passes a code in no table is stepped over and a coefficient index past
//                 63 ends the block: a wrong guess must be able to find the code words' phase, the
//                 zigzag index and the block of the MCU again (measured: a lane that stopped at
//                 such a fault never synchronised, and the rounds equalled the lanes); a lane that
//                 runs out of data leaves "stuck", no error.
//                 The workgroup then scans the block counts.
//   k_jpeg_write  the lanes decode once more from their final start states and write int16
//                 coefficients in natural order into the zeroed [block][64] buffer, DC as
//                 differences.  Errors count only here; the one of the lowest lane is the image's
//                 status, which is what a serial decoder meets first.
//   k_jpeg_dc     the DC differences summed per component, restarted at every restart interval,
//                 wrapping as libjpeg's int accumulator cast to JCOEF does.
//   k_jpeg_idct   dequantisation + IDCT, eight lanes per block (a column each, the transpose through
//                 LDS, then a row each) into uint8 component planes padded to whole MCUs; Cb / Cr
//                 are skipped when the output is the Y plane.
//   k_jpeg_color  upsampling of both chroma planes from rows staged in LDS, colour conversion,
//                 channel order and the strided store.
// Every loop is bounded by the scan's byte count or the lane count, every read by the file's size,
// every write by the buffers' sizes: a corrupt file ends in a status.
//
// Not libjpeg's behaviour, on purpose: libjpeg warns and returns a picture for a truncated scan, a
// bad code, a missing RSTn or left-over data; this decoder refuses those files.  A lone FF inside
// entropy data that is followed by neither 00 nor RSTn is read as the data byte FF; FF fill bytes
// before a marker are skipped.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#ifndef SM_HD
#define SM_HD __host__ __device__ inline
#endif

namespace smk {

typedef long long jd_long;  // width of the intermediate arithmetic

#ifndef SM_JD_SUBSEQ
#define SM_JD_SUBSEQ 128  // 64 and 256 were measured against it
#endif
constexpr uint32_t JD_SUBSEQ = SM_JD_SUBSEQ;  // raw bytes of entropy data per lane
constexpr int JD_BLOCK = 256;
constexpr int JD_LOOP_BLOCK = 1024;
constexpr uint32_t JD_MAX_FILE = (1u << 28) - 1;  // bit positions stay below 2^31
constexpr uint32_t JD_STUCK = 0xFFFFFFFFu;

enum : int {
    JD_OK = 0,
    JD_E_SIG,
    JD_E_TRUNC,
    JD_E_MARKER,
    JD_E_LENGTH,
    JD_E_SOF,
    JD_E_DQT,
    JD_E_DHT,
    JD_E_SOS,
    JD_E_NOTABLE,
    JD_E_NOSCAN,
    JD_E_NOEOI,
    JD_E_GEOM,
    JD_E_LIMIT,
    JD_E_PROCESS,  // first of the unsupported
    JD_E_PRECISION,
    JD_E_SCANS,
    JD_E_SAMPLING,
    JD_E_COMPONENTS,
    JD_E_COLORSPACE,
    JD_E_DNL,
    JD_E_SIZE,  // last of the unsupported
    JD_E_RST,
    JD_E_CODE,
    JD_E_INDEX,
    JD_E_SCAN,
    JD_E_LEFTOVER,
    JD_N
};

inline const char* jpegdec_message(int code)
{
    static const char* const msg[JD_N] = {
        "ok",
        "not a JPEG file (no SOI marker)",
        "truncated file (a segment or the scan runs past the end)",
        "a marker is missing or misplaced between the segments",
        "wrong segment length",
        "malformed or repeated frame header (SOF)",
        "malformed quantisation table (DQT)",
        "malformed Huffman table (DHT)",
        "malformed scan header (SOS)",
        "the scan uses a quantisation or Huffman table that was not defined",
        "no scan before EOI",
        "the scan is not followed by EOI",
        "the file differs from the stated geometry (width, height, channels or subsampling)",
        "more bytes than max_file_bytes allows",
        "unsupported: progressive, lossless or arithmetic coding (SOF2 and above)",
        "unsupported: 12-bit precision",
        "unsupported: several scans",
        "unsupported: sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2)",
        "unsupported: 4 components (CMYK / YCCK) or another component count than 1 and 3",
        "unsupported: a 3-component file that is not YCbCr (Adobe RGB)",
        "unsupported: DNL (the height comes after the scan)",
        "unsupported: a file of 2^28 bytes or pixels and more",
        "restart markers missing, too many or out of sequence",
        "a Huffman code that is in no table",
        "a coefficient index past 63",
        "the entropy data ends before the last block",
        "entropy data left over after the last block",
    };
    return code >= 0 && code < JD_N ? msg[code] : "unknown status";
}

SM_HD bool jpegdec_unsupported(int status) { return status >= JD_E_PROCESS && status <= JD_E_SIZE; }

// ---- descriptor ----------------------------------------------------------------------------------
struct JdHuff {
    int32_t maxcode[18];  // [l] largest code of length l, -1 when there is none
    int32_t valoff[17];   // [l] index of the first value of length l minus its code
    uint16_t look[512];   // 9 bits ahead: length << 8 | value, 0 when the code is longer
    uint8_t huffval[256];
};

struct JdDesc {
    uint32_t status;  // of the parse
    uint32_t W, H;
    int32_t ncomp, hs, vs;  // components; the luma sampling factors (chroma is 1x1)
    uint32_t ri;            // restart interval in MCUs, 0 none
    uint32_t scan_begin, scan_end;  // the entropy data: [begin, end) in the file, end at the closing marker
    uint32_t pad;
    uint16_t qt[3][64];  // per component, natural order
    JdHuff dc[3], ac[3];  // per component
};

struct JdState {
    uint32_t bit;  // position in the file of the next symbol's first bit
    uint32_t bz;   // block in the MCU | zigzag index << 8, or JD_STUCK
};
SM_HD bool operator!=(const JdState& a, const JdState& b) { return a.bit != b.bit || a.bz != b.bz; }

struct JdImg {
    uint32_t status;  // of the header checks and the restart split
    uint32_t nint, nsub, rounds, changed;
    unsigned long long errkey;  // lane << 8 | status of the entropy decode, the smallest wins
};

struct JdArgs {
    const uint8_t* files;
    const uint64_t* offsets;
    const uint64_t* sizes;
    const JdDesc* desc;
    int nimg, H, W, ncomp, hs, vs, out_ch, y_only, keep;
    uint32_t mcux, mcuy, nmcu, bpm, max_file, lane_cap, iv_cap;
    uint32_t yw, yh, cw, ch, dw, dh;  // plane sizes; the real downsampled chroma size
    uint8_t* out;
    size_t img_stride, row_stride;
    JdImg* img;
    uint32_t *ibeg, *iend, *ilane;  // [nimg][iv_cap + 1]
    JdState *start, *exit_a, *exit_b;  // [nimg][lane_cap]
    uint32_t *nblk, *lane_iv, *gpre;
    uint8_t* flag;
    int16_t* coef;  // [nimg][nmcu * bpm][64]
    uint8_t* planes;  // [nimg][yw * yh + 2 * cw * ch]
    size_t plane_stride;
};

SM_HD uint32_t jd_be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }

SM_HD uint8_t jd_natural(int z)
{
    constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[z & 63];
}

// (bits[16], vals) of a DHT segment into a table; false for counts that are no prefix code
inline bool jd_build_huff(const uint8_t* bits, const uint8_t* vals, int nvals, bool is_dc, JdHuff& h)
{
    std::memset(&h, 0, sizeof h);
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - (int32_t)code;
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            if (code >= (1u << l) || k >= nvals) return false;
            if (is_dc && vals[k] > 15) return false;
            h.huffval[k] = vals[k];
            if (l <= 9)
                for (uint32_t e = code << (9 - l); e < ((code + 1) << (9 - l)); ++e) h.look[e] = (uint16_t)(l << 8 | vals[k]);
        }
        h.maxcode[l] = bits[l - 1] ? (int32_t)code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[0] = -1, h.maxcode[17] = 0x7FFFFFFF;
    return k == nvals;
}

// the segments up to the scan and the scan's end; a status
inline int jd_parse(const uint8_t* f, size_t n, JdDesc& d)
{
    std::memset(&d, 0, sizeof d);
    auto done = [&](int st) { d.status = (uint32_t)st; return st; };
    if (n < 3 || f[0] != 0xFF || f[1] != 0xD8 || f[2] != 0xFF) return done(JD_E_SIG);
    if (n > JD_MAX_FILE) return done(JD_E_SIZE);
    struct Raw {
        bool have;
        uint8_t bits[16], vals[256];
        int nvals;
    };
    std::vector<Raw> huff(8, Raw{});
    uint16_t qt[4][64];
    bool have_q[4] = {false, false, false, false}, have_sof = false, jfif = false, adobe = false;
    int adobe_tf = 0, cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n) return done(JD_E_TRUNC);
        if (f[pos] != 0xFF) return done(JD_E_MARKER);
        while (pos < n && f[pos] == 0xFF) ++pos;
        if (pos >= n) return done(JD_E_TRUNC);
        const int m = f[pos++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0x00) return done(JD_E_MARKER);
        if (m == 0xD9) return done(JD_E_NOSCAN);
        if (pos + 2 > n) return done(JD_E_TRUNC);
        const size_t L = jd_be16(f + pos);
        if (L < 2) return done(JD_E_LENGTH);
        if (pos + L > n) return done(JD_E_TRUNC);
        const uint8_t* s = f + pos + 2;
        const size_t sl = L - 2;
        pos += L;
        if (m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF))
            return done(JD_E_PROCESS);
        if (m == 0xDC) return done(JD_E_DNL);
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof) return done(JD_E_SOF);
            if (sl < 6) return done(JD_E_LENGTH);
            if (s[0] == 12) return done(JD_E_PRECISION);
            if (s[0] != 8) return done(JD_E_SOF);
            d.H = jd_be16(s + 1), d.W = jd_be16(s + 3), d.ncomp = s[5];
            if (d.H == 0) return done(JD_E_DNL);
            if (d.W == 0) return done(JD_E_SOF);
            if (d.ncomp != 1 && d.ncomp != 3) return done(JD_E_COMPONENTS);
            if (sl != 6 + 3 * (size_t)d.ncomp) return done(JD_E_LENGTH);
            for (int c = 0; c < d.ncomp; ++c) {
                cid[c] = s[6 + 3 * c], ch[c] = s[7 + 3 * c] >> 4, cv[c] = s[7 + 3 * c] & 15, ctq[c] = s[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4 || ctq[c] > 3) return done(JD_E_SOF);
            }
            have_sof = true;
        } else if (m == 0xDB) {
            size_t p = 0;
            while (p < sl) {
                const int pq = s[p] >> 4, tq = s[p] & 15;
                if (pq > 1 || tq > 3) return done(JD_E_DQT);
                const size_t sz = 64 * (size_t)(pq + 1);
                if (p + 1 + sz > sl) return done(JD_E_LENGTH);
                for (int k = 0; k < 64; ++k)
                    qt[tq][jd_natural(k)] = pq ? (uint16_t)jd_be16(s + p + 1 + 2 * k) : (uint16_t)s[p + 1 + k];
                have_q[tq] = true;
                p += 1 + sz;
            }
        } else if (m == 0xC4) {
            size_t p = 0;
            while (p < sl) {
                if (p + 17 > sl) return done(JD_E_LENGTH);
                const int tc = s[p] >> 4, th = s[p] & 15;
                if (tc > 1 || th > 3) return done(JD_E_DHT);
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += s[p + 1 + i];
                if (cnt > 256) return done(JD_E_DHT);
                if (p + 17 + (size_t)cnt > sl) return done(JD_E_LENGTH);
                Raw& r = huff[(size_t)(tc * 4 + th)];
                r.have = true, r.nvals = cnt;
                std::memcpy(r.bits, s + p + 1, 16);
                std::memcpy(r.vals, s + p + 17, (size_t)cnt);
                JdHuff probe;
                if (!jd_build_huff(r.bits, r.vals, cnt, tc == 0, probe)) return done(JD_E_DHT);
                p += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return done(JD_E_LENGTH);
            d.ri = jd_be16(s);
        } else if (m == 0xE0) {
            if (sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) adobe = true, adobe_tf = s[11];
        } else if (m == 0xDA) {
            if (!have_sof) return done(JD_E_SOS);
            if (sl < 1) return done(JD_E_LENGTH);
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * (size_t)ns) return done(JD_E_LENGTH);
            if (ns != d.ncomp) return done(JD_E_SCANS);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != cid[c]) return done(JD_E_SOS);
                td[c] = s[2 + 2 * c] >> 4, ta[c] = s[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3) return done(JD_E_SOS);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return done(JD_E_SOS);
            break;
        }
        // APPn, COM and any other segment: skipped
    }
    if (d.ncomp == 3) {
        // libjpeg's rule: JFIF says YCbCr; else Adobe's transform flag; else the component ids
        if (!jfif) {
            if (adobe) {
                if (adobe_tf == 0) return done(JD_E_COLORSPACE);
            } else if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') {
                return done(JD_E_COLORSPACE);
            }
        }
        const bool ok = (ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2);
        if (!ok || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return done(JD_E_SAMPLING);
        d.hs = ch[0], d.vs = cv[0];
    } else {
        d.hs = d.vs = 1;  // a single component is never interleaved: its factors do not matter
    }
    for (int c = 0; c < d.ncomp; ++c) {
        const Raw &rd = huff[(size_t)td[c]], &ra = huff[(size_t)(4 + ta[c])];
        if (!have_q[ctq[c]] || !rd.have || !ra.have) return done(JD_E_NOTABLE);
        std::memcpy(d.qt[c], qt[ctq[c]], sizeof d.qt[c]);
        jd_build_huff(rd.bits, rd.vals, rd.nvals, true, d.dc[c]);
        jd_build_huff(ra.bits, ra.vals, ra.nvals, false, d.ac[c]);
    }
    // the end of the scan: the first marker that is neither a stuffed FF nor RSTn
    size_t p = pos;
    int mk = -1;
    while (p < n) {
        if (f[p] != 0xFF) {
            ++p;
            continue;
        }
        size_t q = p;
        while (q < n && f[q] == 0xFF) ++q;
        if (q >= n) break;
        if (f[q] == 0 || (f[q] >= 0xD0 && f[q] <= 0xD7)) {
            p = q + 1;
            continue;
        }
        mk = f[q];
        break;
    }
    if (mk < 0) return done(JD_E_TRUNC);
    if (mk == 0xDC) return done(JD_E_DNL);
    if (mk == 0xDA || mk == 0xC4 || mk == 0xDB || mk == 0xDD) return done(JD_E_SCANS);
    if (mk != 0xD9) return done(JD_E_NOEOI);
    d.scan_begin = (uint32_t)pos, d.scan_end = (uint32_t)p;
    return done(JD_OK);
}

SM_HD int jd_subsampling(const JdDesc& d) { return d.ncomp == 1 ? 0 : d.hs == 1 ? 444 : d.vs == 1 ? 422 : 420; }

// ---- bit reader ------------------------------------------------------------------------------------
struct JdBits {
    const uint8_t* f;
    uint32_t pos, end;  // the next raw byte; the end of the restart interval
    unsigned long long acc;
    int n;
    uint32_t stuff;  // bit j: the j-th last byte loaded was an FF with a stuffed 00 behind it

    SM_HD void fill()
    {
        while (n <= 56) {
            uint32_t c = 0, st = 0;
            if (pos < end) {
                c = f[pos];
                if (c == 0xFF && pos + 1 < end && f[pos + 1] == 0) st = 1;
            }
            pos += 1 + st;
            acc |= (unsigned long long)c << (56 - n);
            n += 8;
            stuff = stuff << 1 | st;
        }
    }
    SM_HD void drop(int k) { acc <<= k, n -= k; }
    SM_HD void start(const uint8_t* file, uint32_t bit, uint32_t iend)
    {
        f = file, pos = bit >> 3, end = iend, acc = 0, n = 0, stuff = 0;
        fill();
        drop((int)(bit & 7));
    }
    SM_HD uint32_t peek16() const { return (uint32_t)(acc >> 48); }
    SM_HD uint32_t take(int k)
    {
        const uint32_t v = k ? (uint32_t)(acc >> (64 - k)) : 0u;
        drop(k);
        return v;
    }
    // position in the file of the next unread bit (past `end` once zeros have been supplied)
    SM_HD uint32_t bitpos() const
    {
        const int r = (n + 7) >> 3;
        const uint32_t byte = pos - (uint32_t)r - (uint32_t)__builtin_popcount(stuff & ((1u << r) - 1u));
        return byte * 8u + (uint32_t)((8 - (n & 7)) & 7);
    }
};

// one Huffman symbol; -1 for a code that is in no table
SM_HD int jd_symbol(JdBits& br, const JdHuff& h)
{
    const uint32_t v = br.peek16();
    const uint32_t e = h.look[v >> 7];
    if (e) {
        br.drop((int)(e >> 8) & 15);
        return (int)(e & 255u);
    }
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)(v >> (16 - l));
        if (code <= h.maxcode[l]) {
            br.drop(l);
            return h.huffval[(uint32_t)(code + h.valoff[l]) & 255u];
        }
    }
    return -1;
}

SM_HD int jd_extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

struct JdTabs {
    const JdHuff* dc;  // [3], per component
    const JdHuff* ac;
    int bpm, nluma;  // blocks per MCU; of them luma
};

// Symbols from state `s` while they start before bit `seg_end` (and, when writing, before block
// `blk_end`).  Returns a status; `out` is the state left in (JD_STUCK after a fault), `nblk` the
// blocks completed.  WRITE: coefficients of block blk0 + nblk go to coef (DC as differences).
template <bool WRITE>
SM_HD int jd_run(const JdTabs& T, const uint8_t* f, uint32_t iend, uint32_t seg_end, JdState s, JdState& out, uint32_t& nblk,
                 int16_t* coef, uint32_t blk0, uint32_t blk_end, bool& hit_end)
{
    nblk = 0, hit_end = false;
    out.bit = s.bit, out.bz = JD_STUCK;
    if (s.bz == JD_STUCK) return JD_OK;
    JdBits br;
    br.start(f, s.bit, iend);
    uint32_t b = s.bz & 255u, z = (s.bz >> 8) & 255u;
    if ((int)b >= T.bpm || z > 63) return JD_E_CODE;
    int st = JD_OK;
    for (;;) {
        const uint32_t cur = br.bitpos();
        if (WRITE && blk0 + nblk >= blk_end) {
            hit_end = true;
            out.bit = cur, out.bz = b | z << 8;
            break;
        }
        if (cur >= seg_end) {
            out.bit = cur, out.bz = b | z << 8;
            break;
        }
        br.fill();
        const int c = (int)b < T.nluma ? 0 : (int)b - T.nluma + 1;
        if (z == 0) {
            const int sym = jd_symbol(br, T.dc[c]);
            if (sym < 0) {
                if (!WRITE) {  // a wrong guess: step on and let the code words find their phase again
                    br.drop(16);
                    continue;
                }
                st = JD_E_CODE;
                break;
            }
            const int size = sym & 15;
            const int diff = jd_extend(br.take(size), size);
            if (WRITE) coef[(size_t)(blk0 + nblk) * 64] = (int16_t)diff;
            z = 1;
        } else {
            const int sym = jd_symbol(br, T.ac[c]);
            if (sym < 0) {
                if (!WRITE) {
                    br.drop(16);
                    continue;
                }
                st = JD_E_CODE;
                break;
            }
            const uint32_t run = (uint32_t)sym >> 4;
            const int size = sym & 15;
            if (size == 0) {
                if (run == 15) {
                    if (z + 16 > 64) {
                        if (WRITE) {
                            st = JD_E_INDEX;
                            break;
                        }
                        z = 64;  // a wrong guess ends the block here, so that the lane can still synchronise
                    } else {
                        z += 16;
                    }
                } else {
                    z = 64;
                }
            } else {
                z += run;
                if (z > 63 && WRITE) {
                    st = JD_E_INDEX;
                    break;
                }
                const int val = jd_extend(br.take(size), size);
                if (WRITE) coef[(size_t)(blk0 + nblk) * 64 + jd_natural((int)z)] = (int16_t)val;
                z = z > 63 ? 64 : z + 1;
            }
        }
        if (br.bitpos() > iend * 8u) {
            st = JD_E_SCAN;
            break;
        }
        if (z == 64) {
            z = 0;
            b = (int)b + 1 == T.bpm ? 0 : b + 1;
            ++nblk;
        }
    }
    return st;
}

// what the lane that holds the end of an interval's data checks after writing: every block there,
// and nothing but fill bytes behind the last symbol's byte
SM_HD int jd_tail_check(const uint8_t* f, uint32_t iend, const JdState& out, bool complete)
{
    if (!complete || (out.bz >> 8) != 0) return JD_E_SCAN;
    uint32_t p = (out.bit + 7) >> 3;
    if ((out.bit & 7u) && p < iend && f[p] == 0 && f[p - 1] == 0xFF) ++p;  // the last byte was a stuffed FF
    for (; p < iend; ++p)
        if (f[p] != 0xFF) return JD_E_LEFTOVER;
    return JD_OK;
}

// lane j of an interval [ibeg, iend): its first byte and the bit it ends before
SM_HD void jd_lane_seg(uint32_t ibeg, uint32_t iend, uint32_t j, uint32_t& first, uint32_t& end_bit)
{
    first = ibeg + j * JD_SUBSEQ;
    const unsigned long long e = (unsigned long long)first + JD_SUBSEQ;
    end_bit = (uint32_t)(e < iend ? e : iend) * 8u;
}

SM_HD uint32_t jd_lanes_of(uint32_t ibeg, uint32_t iend)
{
    const uint32_t len = iend - ibeg;
    return len ? (len + JD_SUBSEQ - 1) / JD_SUBSEQ : 1u;
}

// ---- IDCT (jidctint.c) ------------------------------------------------------------------------------
// one pass over eight values; the outputs descaled by `shift`
SM_HD void jd_idct8(const jd_long* in, int shift, jd_long* o)
{
    jd_long z2 = in[2], z3 = in[6];
    jd_long z1 = (z2 + z3) * 4433;
    jd_long tmp2 = z1 - z3 * 15137, tmp3 = z1 + z2 * 6270;
    jd_long tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;
    const jd_long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    jd_long z4 = tmp1 + tmp3;
    const jd_long z5 = (z3 + z4) * 9633;
    tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const jd_long r = (jd_long)1 << (shift - 1);
    o[0] = (tmp10 + tmp3 + r) >> shift, o[7] = (tmp10 - tmp3 + r) >> shift;
    o[1] = (tmp11 + tmp2 + r) >> shift, o[6] = (tmp11 - tmp2 + r) >> shift;
    o[2] = (tmp12 + tmp1 + r) >> shift, o[5] = (tmp12 - tmp1 + r) >> shift;
    o[3] = (tmp13 + tmp0 + r) >> shift, o[4] = (tmp13 - tmp0 + r) >> shift;
}

SM_HD uint8_t jd_range_limit(jd_long v)
{
    const int x = (int)(v & 1023);
    return (uint8_t)(x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896);
}

// column c of a block (natural order, stride 8) dequantised and transformed into ws[r * stride + c]
SM_HD void jd_idct_column(const int16_t* coef, const uint16_t* q, int c, int32_t* ws, int stride)
{
    jd_long in[8], o[8];
    for (int r = 0; r < 8; ++r) in[r] = (jd_long)coef[r * 8 + c] * (jd_long)q[r * 8 + c];
    jd_idct8(in, 11, o);
    for (int r = 0; r < 8; ++r) ws[r * stride + c] = (int32_t)(uint32_t)(unsigned long long)o[r];
}

SM_HD void jd_idct_row(const int32_t* ws, uint8_t* px)
{
    jd_long in[8], o[8];
    for (int k = 0; k < 8; ++k) in[k] = ws[k];
    jd_idct8(in, 18, o);
    for (int k = 0; k < 8; ++k) px[k] = jd_range_limit(o[k]);
}

// ---- upsampling (jdsample.c) and colour (jdcolor.c) ---------------------------------------------------
// sample x of a row upsampled 2:1 from `row` (dw real samples; row[i - off] is sample i)
SM_HD int jd_up_h2v1(const uint8_t* row, int off, int dw, int x)
{
    const int i = x >> 1, v = row[i - off];
    if (dw <= 2 || (i == 0 && !(x & 1)) || (i == dw - 1 && (x & 1))) return v;
    return (x & 1) ? (3 * v + row[i + 1 - off] + 2) >> 2 : (3 * v + row[i - 1 - off] + 1) >> 2;
}

// the same for 2:1 in both directions: `near` is the chroma row of the output row, `far` its
// neighbour on the output row's side (the same row at the picture's edge)
SM_HD int jd_up_h2v2(const uint8_t* near, const uint8_t* far, int off, int dw, int x)
{
    const int i = x >> 1;
    if (dw <= 2) return near[i - off];
    const int t = 3 * near[i - off] + far[i - off];
    if (x & 1) {
        if (i == dw - 1) return (4 * t + 7) >> 4;
        return (3 * t + 3 * near[i + 1 - off] + far[i + 1 - off] + 7) >> 4;
    }
    if (i == 0) return (4 * t + 8) >> 4;
    return (3 * t + 3 * near[i - 1 - off] + far[i - 1 - off] + 8) >> 4;
}

SM_HD uint8_t jd_clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

SM_HD void jd_ycc(int y, int cb, int cr, uint8_t& r, uint8_t& g, uint8_t& b)
{
    cb -= 128, cr -= 128;
    r = jd_clamp8(y + ((91881 * cr + 32768) >> 16));
    g = jd_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    b = jd_clamp8(y + ((116130 * cb + 32768) >> 16));
}

// the chroma row of output row y and its far neighbour
SM_HD void jd_chroma_rows(int vs, int dh, int y, int& near, int& far)
{
    if (vs == 1) {
        near = far = y;
        return;
    }
    near = y >> 1;
    far = (y & 1) ? (near + 1 < dh ? near + 1 : dh - 1) : (near > 0 ? near - 1 : 0);
}

// one output pixel from the luma sample and the two chroma rows of each plane
SM_HD void jd_store_pixel(const JdArgs& a, uint8_t* dst, int yv, const uint8_t* cb_n, const uint8_t* cb_f, const uint8_t* cr_n,
                          const uint8_t* cr_f, int off, int x)
{
    if (a.out_ch == 1) {
        dst[0] = (uint8_t)yv;
        return;
    }
    if (a.ncomp == 1) {
        dst[0] = dst[1] = dst[2] = (uint8_t)yv;
        return;
    }
    int cb, cr;
    if (a.hs == 1) {
        cb = cb_n[x - off], cr = cr_n[x - off];
    } else if (a.vs == 1) {
        cb = jd_up_h2v1(cb_n, off, (int)a.dw, x), cr = jd_up_h2v1(cr_n, off, (int)a.dw, x);
    } else {
        cb = jd_up_h2v2(cb_n, cb_f, off, (int)a.dw, x), cr = jd_up_h2v2(cr_n, cr_f, off, (int)a.dw, x);
    }
    uint8_t r, g, b;
    jd_ycc(yv, cb, cr, r, g, b);
    dst[0] = a.keep ? r : b, dst[1] = g, dst[2] = a.keep ? b : r;
}

// the geometry every entry point derives from (H, W, components, luma factors)
SM_HD void jd_geometry(JdArgs& a)
{
    a.mcux = ((uint32_t)a.W + 8u * a.hs - 1) / (8u * a.hs), a.mcuy = ((uint32_t)a.H + 8u * a.vs - 1) / (8u * a.vs);
    a.nmcu = a.mcux * a.mcuy;
    a.bpm = a.ncomp == 1 ? 1u : (uint32_t)(a.hs * a.vs + 2);
    a.yw = a.mcux * 8u * a.hs, a.yh = a.mcuy * 8u * a.vs;
    a.cw = a.ncomp == 1 ? 0u : a.mcux * 8u, a.ch = a.ncomp == 1 ? 0u : a.mcuy * 8u;
    a.dw = ((uint32_t)a.W + a.hs - 1) / a.hs, a.dh = ((uint32_t)a.H + a.vs - 1) / a.vs;
    a.plane_stride = ((size_t)a.yw * a.yh + 2 * (size_t)a.cw * a.ch + 15) & ~(size_t)15;
}

// the descriptor against the stated geometry and the file's size
SM_HD int jd_check_desc(const JdArgs& a, const JdDesc& d, unsigned long long size)
{
    if (d.status) return (int)d.status < JD_N ? (int)d.status : JD_E_GEOM;
    if ((int)d.H != a.H || (int)d.W != a.W || d.ncomp != a.ncomp || d.hs != a.hs || d.vs != a.vs) return JD_E_GEOM;
    if (size > a.max_file) return JD_E_LIMIT;
    if (d.scan_begin > d.scan_end || d.scan_end > size) return JD_E_TRUNC;
    return JD_OK;
}

SM_HD uint32_t jd_intervals(const JdArgs& a, const JdDesc& d) { return d.ri ? (a.nmcu + d.ri - 1) / d.ri : 1u; }

SM_HD void jd_tabs(const JdArgs& a, const JdHuff* dc, const JdHuff* ac, JdTabs& T)
{
    T.dc = dc, T.ac = ac;
    T.bpm = (int)a.bpm, T.nluma = a.ncomp == 1 ? 1 : a.hs * a.vs;
}

// block `blk` of the scan: its component and the top-left sample in that component's plane
SM_HD void jd_block_place(const JdArgs& a, uint32_t blk, int& comp, uint32_t& px, uint32_t& py)
{
    const uint32_t mcu = blk / a.bpm, b = blk % a.bpm, mx = mcu % a.mcux, my = mcu / a.mcux;
    const uint32_t nl = a.ncomp == 1 ? 1u : (uint32_t)(a.hs * a.vs);
    if (b < nl) {
        comp = 0;
        px = (mx * a.hs + b % a.hs) * 8u, py = (my * a.vs + b / a.hs) * 8u;
    } else {
        comp = (int)(b - nl) + 1;
        px = mx * 8u, py = my * 8u;
    }
}

SM_HD uint8_t* jd_plane(const JdArgs& a, uint8_t* planes, int comp, uint32_t& stride)
{
    stride = comp ? a.cw : a.yw;
    return planes + (comp ? (size_t)a.yw * a.yh + (size_t)(comp - 1) * a.cw * a.ch : 0);
}

// ---- the CPU twin: a plain serial decoder from the same functions -------------------------------------
// a.files / offsets / sizes / desc name one file in host memory; nsub: the lanes the device would use
inline int jpegdec_host(JdArgs a, uint32_t& nsub)
{
    nsub = 0;
    const uint8_t* f = a.files + a.offsets[0];
    const unsigned long long size = a.sizes[0];
    const JdDesc& d = a.desc[0];
    int st = jd_check_desc(a, d, size);
    if (st) return st;
    // restart split
    const uint32_t nint = jd_intervals(a, d);
    std::vector<uint32_t> ibeg{d.scan_begin}, iend;
    bool rst_ok = true;
    for (uint32_t p = d.scan_begin; p + 1 < d.scan_end; ++p)
        if (f[p] == 0xFF && f[p + 1] >= 0xD0 && f[p + 1] <= 0xD7) {
            rst_ok = rst_ok && (uint32_t)(f[p + 1] - 0xD0) == ((uint32_t)iend.size() & 7u);
            iend.push_back(p);
            ibeg.push_back(p + 2);
        }
    iend.push_back(d.scan_end);
    if (!rst_ok || iend.size() != nint) return JD_E_RST;
    for (uint32_t k = 0; k < nint; ++k) nsub += jd_lanes_of(ibeg[k], iend[k]);
    JdTabs T;
    jd_tabs(a, d.dc, d.ac, T);
    const size_t nblocks = (size_t)a.nmcu * a.bpm;
    std::vector<int16_t> coef(nblocks * 64, 0);
    for (uint32_t k = 0; k < nint; ++k) {
        const uint32_t blk0 = d.ri ? k * d.ri * a.bpm : 0u;
        const uint32_t blk_end = d.ri ? std::min((k + 1) * d.ri, a.nmcu) * a.bpm : a.nmcu * a.bpm;
        JdState s{ibeg[k] * 8u, 0u}, out;
        uint32_t nb = 0;
        bool hit = false;
        st = jd_run<true>(T, f, iend[k], iend[k] * 8u, s, out, nb, coef.data(), blk0, blk_end, hit);
        if (st) return st;
        st = jd_tail_check(f, iend[k], out, blk0 + nb == blk_end);
        if (st) return st;
    }
    // DC prediction
    const uint32_t nl = (uint32_t)T.nluma;
    for (int c = 0; c < a.ncomp; ++c) {
        uint32_t acc = 0;
        for (uint32_t m = 0; m < a.nmcu; ++m) {
            if (d.ri ? m % d.ri == 0 : m == 0) acc = 0;
            const uint32_t first = c ? nl + (uint32_t)c - 1 : 0u, cnt = c ? 1u : nl;
            for (uint32_t i = 0; i < cnt; ++i) {
                int16_t& v = coef[((size_t)m * a.bpm + first + i) * 64];
                acc += (uint32_t)(int32_t)v;
                v = (int16_t)(uint16_t)acc;
            }
        }
    }
    // IDCT into the planes
    std::vector<uint8_t> planes(a.plane_stride + 16, 0);
    for (size_t blk = 0; blk < nblocks; ++blk) {
        int comp;
        uint32_t px, py, stride;
        jd_block_place(a, (uint32_t)blk, comp, px, py);
        if (comp && a.y_only) continue;
        uint8_t* pl = jd_plane(a, planes.data(), comp, stride);
        int32_t ws[64];
        for (int c = 0; c < 8; ++c) jd_idct_column(&coef[blk * 64], d.qt[comp], c, ws, 8);
        for (int r = 0; r < 8; ++r) jd_idct_row(ws + r * 8, pl + (size_t)(py + r) * stride + px);
    }
    // upsampling, colour, store
    uint32_t ys, cs = 0;
    const uint8_t* yp = jd_plane(a, planes.data(), 0, ys);
    const uint8_t* cbp = a.ncomp == 3 ? jd_plane(a, planes.data(), 1, cs) : nullptr;
    const uint8_t* crp = a.ncomp == 3 ? jd_plane(a, planes.data(), 2, cs) : nullptr;
    for (int y = 0; y < a.H; ++y) {
        int near = 0, far = 0;
        jd_chroma_rows(a.vs, (int)a.dh, y, near, far);
        for (int x = 0; x < a.W; ++x)
            jd_store_pixel(a, a.out + (size_t)y * a.row_stride + (size_t)x * a.out_ch, yp[(size_t)y * ys + x],
                           cbp ? cbp + (size_t)near * cs : nullptr, cbp ? cbp + (size_t)far * cs : nullptr,
                           crp ? crp + (size_t)near * cs : nullptr, crp ? crp + (size_t)far * cs : nullptr, 0, x);
    }
    return JD_OK;
}

#if defined(__HIPCC__)

// exclusive scan of v[0..n) into o[0..n] (o[n] the total) by one workgroup; tmp: blockDim.x + 1 words of LDS
__device__ inline void jd_block_scan(const uint32_t* v, uint32_t n, uint32_t* o, uint32_t* tmp)
{
    const uint32_t t = threadIdx.x, nt = blockDim.x, chunk = (n + nt - 1) / nt;
    const uint32_t lo = min(t * chunk, n), hi = min(lo + chunk, n);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += v[i];
    tmp[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < nt; ++i) {
            const uint32_t x = tmp[i];
            tmp[i] = run;
            run += x;
        }
        tmp[nt] = run;
    }
    __syncthreads();
    s = tmp[t];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t x = v[i];
        o[i] = s;
        s += x;
    }
    if (t == 0) o[n] = tmp[nt];
    __syncthreads();
}

struct JdLdsTabs {
    JdHuff dc[3], ac[3];
};

__device__ inline void jd_load_tabs(const JdArgs& a, int im, JdLdsTabs& L)
{
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.desc[im].dc);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&L);
    for (uint32_t i = threadIdx.x; i < sizeof(JdLdsTabs) / 4; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_split(JdArgs a)
{
    __shared__ uint32_t tmp[JD_BLOCK + 1];
    __shared__ uint32_t s_bad;
    const int im = blockIdx.x;
    const uint32_t t = threadIdx.x;
    JdImg& img = a.img[im];
    const JdDesc& d = a.desc[im];
    const uint8_t* f = a.files + a.offsets[im];
    const int st0 = jd_check_desc(a, d, a.sizes[im]);
    if (t == 0) {
        img.status = (uint32_t)st0, img.nint = 0, img.nsub = 0, img.rounds = 0, img.changed = 0;
        img.errkey = ~0ull;
        s_bad = 0;
    }
    __syncthreads();
    if (st0) return;
    const uint32_t sb = d.scan_begin, se = d.scan_end, nint = jd_intervals(a, d);
    uint32_t* ibeg = a.ibeg + (size_t)im * (a.iv_cap + 1);
    uint32_t* iend = a.iend + (size_t)im * (a.iv_cap + 1);
    uint32_t* ilane = a.ilane + (size_t)im * (a.iv_cap + 1);
    // markers: counted per thread over a contiguous piece, then placed
    const uint32_t len = se - sb, chunk = (len + JD_BLOCK - 1) / JD_BLOCK;
    const uint32_t lo = sb + min(t * chunk, len), hi = sb + min((t + 1) * chunk, len);
    uint32_t cnt = 0;
    for (uint32_t p = lo; p < hi; ++p)
        if (f[p] == 0xFF && p + 1 < se && f[p + 1] >= 0xD0 && f[p + 1] <= 0xD7) ++cnt;
    tmp[t] = cnt;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < JD_BLOCK; ++i) {
            const uint32_t x = tmp[i];
            tmp[i] = run;
            run += x;
        }
        tmp[JD_BLOCK] = run;
        if (run != nint - 1) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {
        if (t == 0) img.status = JD_E_RST;
        return;
    }
    uint32_t k = tmp[t];
    for (uint32_t p = lo; p < hi; ++p)
        if (f[p] == 0xFF && p + 1 < se && f[p + 1] >= 0xD0 && f[p + 1] <= 0xD7) {
            if ((uint32_t)(f[p + 1] - 0xD0) != (k & 7u)) s_bad = 1;
            iend[k] = p, ibeg[k + 1] = p + 2;  // k < nint - 1 <= iv_cap - 1
            ++k;
        }
    if (t == 0) ibeg[0] = sb, iend[nint - 1] = se;
    __syncthreads();
    if (s_bad) {
        if (t == 0) img.status = JD_E_RST;
        return;
    }
    // lanes per interval (kept in iend's shadow: ilane first holds the counts)
    uint32_t* cntv = a.gpre + (size_t)im * a.lane_cap;  // scratch: lane_cap >= nint
    for (uint32_t i = t; i < nint; i += JD_BLOCK) cntv[i] = jd_lanes_of(ibeg[i], iend[i]);
    __syncthreads();
    jd_block_scan(cntv, nint, ilane, tmp);
    if (t == 0) {
        img.nint = nint, img.nsub = ilane[nint];
        if (img.nsub >= a.lane_cap) img.status = JD_E_LIMIT;  // cannot happen for sizes within max_file
    }
}

// the interval of a lane: the last k with ilane[k] <= lane
__device__ inline uint32_t jd_find_interval(const uint32_t* ilane, uint32_t nint, uint32_t lane)
{
    uint32_t lo = 0, hi = nint;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ilane[mid] <= lane) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_sync_a(JdArgs a)
{
    __shared__ JdLdsTabs L;
    const int im = blockIdx.y;
    const JdImg& img = a.img[im];
    if (img.status || blockIdx.x * JD_BLOCK >= img.nsub) return;  // the grid is sized for the largest file
    jd_load_tabs(a, im, L);
    const uint32_t lane = blockIdx.x * JD_BLOCK + threadIdx.x;
    if (lane >= img.nsub) return;
    const size_t iv0 = (size_t)im * (a.iv_cap + 1), l0 = (size_t)im * a.lane_cap;
    const uint32_t k = jd_find_interval(a.ilane + iv0, img.nint, lane), j = lane - a.ilane[iv0 + k];
    const uint32_t ibeg = a.ibeg[iv0 + k], iend = a.iend[iv0 + k];
    const uint8_t* f = a.files + a.offsets[im];
    uint32_t first, end_bit;
    jd_lane_seg(ibeg, iend, j, first, end_bit);
    if (j && first < iend && f[first] == 0 && f[first - 1] == 0xFF) ++first;  // the cut fell on a stuffed 00
    JdTabs T;
    jd_tabs(a, L.dc, L.ac, T);
    const JdState s{first * 8u, 0u};
    JdState out;
    uint32_t nb;
    bool hit;
    jd_run<false>(T, f, iend, end_bit, s, out, nb, nullptr, 0, 0, hit);
    a.start[l0 + lane] = s, a.exit_a[l0 + lane] = out, a.nblk[l0 + lane] = nb;
    a.lane_iv[l0 + lane] = k << 1 | (j == 0 ? 1u : 0u);
}

// one grid-wide round: exit_a -> exit_b
__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_sync_b(JdArgs a)
{
    __shared__ JdLdsTabs L;
    const int im = blockIdx.y;
    JdImg& img = a.img[im];
    if (img.status || blockIdx.x * JD_BLOCK >= img.nsub) return;  // the grid is sized for the largest file
    jd_load_tabs(a, im, L);
    const uint32_t lane = blockIdx.x * JD_BLOCK + threadIdx.x;
    if (lane >= img.nsub) return;
    const size_t iv0 = (size_t)im * (a.iv_cap + 1), l0 = (size_t)im * a.lane_cap;
    const uint32_t liv = a.lane_iv[l0 + lane], k = liv >> 1;
    JdState out = a.exit_a[l0 + lane];
    if (!(liv & 1u)) {
        const JdState pred = a.exit_a[l0 + lane - 1];
        if (pred != a.start[l0 + lane]) {
            const uint32_t ibeg = a.ibeg[iv0 + k], iend = a.iend[iv0 + k];
            uint32_t first, end_bit, nb;
            jd_lane_seg(ibeg, iend, lane - a.ilane[iv0 + k], first, end_bit);
            JdTabs T;
            jd_tabs(a, L.dc, L.ac, T);
            bool hit;
            jd_run<false>(T, a.files + a.offsets[im], iend, end_bit, pred, out, nb, nullptr, 0, 0, hit);
            a.start[l0 + lane] = pred, a.nblk[l0 + lane] = nb;
            img.changed = 1;
        }
    }
    a.exit_b[l0 + lane] = out;
}

// the remaining rounds in one workgroup per image, then the scan of the block counts
__global__ void __launch_bounds__(JD_LOOP_BLOCK) k_jpeg_sync_loop(JdArgs a)
{
    __shared__ JdLdsTabs L;
    __shared__ uint32_t tmp[JD_LOOP_BLOCK + 1];
    __shared__ uint32_t s_any;
    const int im = blockIdx.x;
    JdImg& img = a.img[im];
    if (img.status) return;
    jd_load_tabs(a, im, L);
    const uint32_t nsub = img.nsub, t = threadIdx.x;
    const size_t iv0 = (size_t)im * (a.iv_cap + 1), l0 = (size_t)im * a.lane_cap;
    JdTabs T;
    jd_tabs(a, L.dc, L.ac, T);
    const uint8_t* f = a.files + a.offsets[im];
    uint32_t rounds = img.changed ? 1u : 0u;
    for (uint32_t round = 0; round < nsub; ++round) {
        if (t == 0) s_any = 0;
        __syncthreads();
        for (uint32_t lane = t; lane < nsub; lane += JD_LOOP_BLOCK) {
            uint8_t todo = 0;
            if (!(a.lane_iv[l0 + lane] & 1u)) {
                const JdState pred = a.exit_b[l0 + lane - 1];
                if (pred != a.start[l0 + lane]) a.start[l0 + lane] = pred, todo = 1, s_any = 1;
            }
            a.flag[l0 + lane] = todo;
        }
        __syncthreads();
        const bool any = s_any != 0;
        for (uint32_t lane = t; lane < nsub; lane += JD_LOOP_BLOCK) {
            if (!a.flag[l0 + lane]) continue;
            const uint32_t k = a.lane_iv[l0 + lane] >> 1, ibeg = a.ibeg[iv0 + k], iend = a.iend[iv0 + k];
            uint32_t first, end_bit, nb;
            jd_lane_seg(ibeg, iend, lane - a.ilane[iv0 + k], first, end_bit);
            JdState out;
            bool hit;
            jd_run<false>(T, f, iend, end_bit, a.start[l0 + lane], out, nb, nullptr, 0, 0, hit);
            a.exit_b[l0 + lane] = out, a.nblk[l0 + lane] = nb;
        }
        __syncthreads();
        if (!any) break;
        ++rounds;
    }
    if (t == 0) img.rounds = rounds;
    jd_block_scan(a.nblk + l0, nsub, a.gpre + l0, tmp);  // lane_cap > nsub: room for the total
}

__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_write(JdArgs a)
{
    __shared__ JdLdsTabs L;
    const int im = blockIdx.y;
    JdImg& img = a.img[im];
    if (img.status || blockIdx.x * JD_BLOCK >= img.nsub) return;  // the grid is sized for the largest file
    jd_load_tabs(a, im, L);
    const uint32_t lane = blockIdx.x * JD_BLOCK + threadIdx.x;
    if (lane >= img.nsub) return;
    const size_t iv0 = (size_t)im * (a.iv_cap + 1), l0 = (size_t)im * a.lane_cap;
    const uint32_t k = a.lane_iv[l0 + lane] >> 1, ibeg = a.ibeg[iv0 + k], iend = a.iend[iv0 + k];
    const uint32_t lane0 = a.ilane[iv0 + k], nl = a.ilane[iv0 + k + 1] - lane0;
    const uint32_t ri = a.desc[im].ri, total = a.nmcu * a.bpm;
    const uint32_t base = ri ? min(k * ri, a.nmcu) * a.bpm : 0u;
    const uint32_t blk_end = ri ? min((k + 1) * ri, a.nmcu) * a.bpm : total;
    const unsigned long long b0 = (unsigned long long)base + (a.gpre[l0 + lane] - a.gpre[l0 + lane0]);
    // a lane behind the one that completes the interval's last block has nothing to decode, and its
    // start state comes from passes that did not stop there: that lane has made the tail check
    if (b0 >= blk_end) return;
    const uint32_t blk0 = (uint32_t)b0;
    const JdState s = a.start[l0 + lane];
    if (s.bz == JD_STUCK) return;  // the lane before met the fault and reports it
    uint32_t first, end_bit, nb;
    jd_lane_seg(ibeg, iend, lane - lane0, first, end_bit);
    JdTabs T;
    jd_tabs(a, L.dc, L.ac, T);
    const uint8_t* f = a.files + a.offsets[im];
    JdState out;
    bool hit;
    int st = jd_run<true>(T, f, iend, end_bit, s, out, nb, a.coef + (size_t)im * total * 64, blk0, blk_end, hit);
    if (!st && (hit || lane - lane0 == nl - 1)) st = jd_tail_check(f, iend, out, blk0 + nb == blk_end);
    if (st) atomicMin(&img.errkey, (unsigned long long)lane << 8 | (unsigned long long)st);
}

// grid (components, images)
__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_dc(JdArgs a)
{
    __shared__ uint32_t s_sum[JD_BLOCK], s_cut[JD_BLOCK];
    const int im = blockIdx.y, c = blockIdx.x;
    const JdImg& img = a.img[im];
    if (img.status || img.errkey != ~0ull) return;
    const uint32_t nl = a.ncomp == 1 ? 1u : (uint32_t)(a.hs * a.vs);
    const uint32_t per = c ? 1u : nl, first = c ? nl + (uint32_t)c - 1 : 0u, n = a.nmcu * per;
    const uint32_t ri = a.desc[im].ri, t = threadIdx.x, chunk = (n + JD_BLOCK - 1) / JD_BLOCK;
    const uint32_t lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int16_t* coef = a.coef + (size_t)im * a.nmcu * a.bpm * 64;
    uint32_t acc = 0, cut = 0;
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t m = e / per, i = e % per;
        if (i == 0 && (ri ? m % ri == 0 : m == 0)) acc = 0, cut = 1;
        acc += (uint32_t)(int32_t)coef[((size_t)m * a.bpm + first + i) * 64];
    }
    s_sum[t] = acc, s_cut[t] = cut;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < JD_BLOCK; ++i) {
            const uint32_t in = run;
            run = s_cut[i] ? s_sum[i] : run + s_sum[i];
            s_sum[i] = in;
        }
    }
    __syncthreads();
    acc = s_sum[t];
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t m = e / per, i = e % per;
        if (i == 0 && (ri ? m % ri == 0 : m == 0)) acc = 0;
        int16_t& v = coef[((size_t)m * a.bpm + first + i) * 64];
        acc += (uint32_t)(int32_t)v;
        v = (int16_t)(uint16_t)acc;
    }
}

// eight lanes per block, 32 blocks per workgroup
__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_idct(JdArgs a)
{
    __shared__ int32_t ws[32][8 * 9 + 1];
    __shared__ uint16_t qt[3][64];
    const int im = blockIdx.y;
    const JdImg& img = a.img[im];
    if (img.status || img.errkey != ~0ull) return;
    const uint32_t t = threadIdx.x, total = a.nmcu * a.bpm;
    if (t < 192) qt[t >> 6][t & 63] = a.desc[im].qt[t >> 6][t & 63];
    __syncthreads();
    const uint32_t blk = blockIdx.x * 32u + (t >> 3), l = t & 7u;
    int comp = 0;
    uint32_t px = 0, py = 0;
    const bool live = blk < total;
    if (live) jd_block_place(a, blk, comp, px, py);
    const bool work = live && !(comp && a.y_only);
    if (work) jd_idct_column(a.coef + ((size_t)im * total + blk) * 64, qt[comp], (int)l, ws[t >> 3], 9);
    __syncthreads();
    if (work) {
        uint32_t stride;
        uint8_t* pl = jd_plane(a, a.planes + (size_t)im * a.plane_stride, comp, stride);
        union {
            uint8_t b[8];
            uint2 v;
        } o;
        jd_idct_row(&ws[t >> 3][l * 9], o.b);
        *reinterpret_cast<uint2*>(pl + (size_t)(py + l) * stride + px) = o.v;  // planes, strides and px are multiples of 8
    }
}

// a workgroup per 256 output columns of an output row pair; grid (column tiles, row pairs, images)
__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_color(JdArgs a)
{
    __shared__ uint8_t s_c[2][4][JD_BLOCK + 8];  // plane, {near, far} of the two rows
    const int im = blockIdx.z;
    const JdImg& img = a.img[im];
    if (img.status || img.errkey != ~0ull) return;
    const int t = threadIdx.x, x0 = blockIdx.x * JD_BLOCK, y0 = blockIdx.y * 2;
    const uint8_t* planes = a.planes + (size_t)im * a.plane_stride;
    const bool colour = a.ncomp == 3 && a.out_ch == 3;
    // chroma samples x0 / hs - 1 .. (x0 + 255) / hs + 1 of the rows the two output rows read
    const int c0 = max(x0 / a.hs - 1, 0);
    if (colour) {
        const int c1 = min((x0 + JD_BLOCK - 1) / a.hs + 1, (int)a.dw - 1), ncol = c1 - c0 + 1;
        for (int i = t; i < 8 * ncol; i += JD_BLOCK) {
            const int col = i % ncol, slot = (i / ncol) & 3, pl = i / ncol / 4;
            int near, far;
            jd_chroma_rows(a.vs, (int)a.dh, min(y0 + (slot >> 1), a.H - 1), near, far);
            const uint8_t* src = planes + (size_t)a.yw * a.yh + (size_t)pl * a.cw * a.ch;
            s_c[pl][slot][col] = src[(size_t)((slot & 1) ? far : near) * a.cw + c0 + col];
        }
    }
    __syncthreads();
    const int x = x0 + t;
    if (x >= a.W) return;
    uint8_t* out = a.out + (size_t)im * a.img_stride;
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (y >= a.H) break;
        jd_store_pixel(a, out + (size_t)y * a.row_stride + (size_t)x * a.out_ch, planes[(size_t)y * a.yw + x], s_c[0][2 * r],
                       s_c[0][2 * r + 1], s_c[1][2 * r], s_c[1][2 * r + 1], c0, x);
    }
}

__global__ void __launch_bounds__(JD_BLOCK) k_jpeg_status(JdArgs a, int* status)
{
    const int im = blockIdx.x * JD_BLOCK + threadIdx.x;
    if (im >= a.nimg) return;
    const JdImg& g = a.img[im];
    status[im] = g.status ? (int)g.status : g.errkey != ~0ull ? (int)(g.errkey & 255ull) : 0;
}

#endif  // __HIPCC__

}  // namespace smk
