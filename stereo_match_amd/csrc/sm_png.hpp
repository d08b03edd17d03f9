// sm_png.hpp — PNG output: what the reference's scripts hand to cv2.imwrite
// (disparity_calculation.py:247-291, rectified_img_cal.py:316-319, disparity_test.py:114-115,
// try_try.py:155,190) and the KITTI disparity format (16-bit gray, disparity * 256, 0 invalid),
// encoded where the images already are.
//
// The file: signature, IHDR, one IDAT chunk per 32 KiB segment of the filtered stream, IEND.
//   filter    per row one type byte and W*bpp filtered bytes; the type by libpng's heuristic (the
//             smallest sum of the filtered bytes taken as signed magnitudes, ties to the lowest
//             type) or fixed.  Pixel conversion (BGR -> RGB, big-endian 16-bit samples, disparity
//             maps to KITTI uint16 or to min-max uint8) happens on load: png_raw_byte.
//   deflate   every segment on its own: runs (matches at distance 1) + literals, one dynamic
//             Huffman block (lit/len code limited to 15 bits, code-length code to 7), or a stored
//             block when that is smaller.  A segment that is not the last ends on a byte boundary
//             through an empty stored block, so the chunks concatenate to one zlib stream.
//   checksums each chunk's CRC-32 covers that segment alone; the stream's Adler-32 is combined
//             from per-segment sums.
// Every function that decides a byte of the output is __host__ __device__ and runs on both sides:
// sm_png_encode_host (png_encode_host below) gives the file of the kernels byte for byte.
//
// Launches (plain, on the ctx stream, the boundaries are the ordering): k_png_minmax (only for
// min-max uint8 without given bounds), k_png_filter (a wave per row), k_png_deflate (a workgroup
// of 1024 threads per segment, the segment in LDS), k_png_assemble (a workgroup per image: scan of the chunk
// sizes, Adler combination, signature, IHDR, IEND, size), k_png_scatter (a workgroup per chunk).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace smk {

#ifndef SM_HD
#define SM_HD __host__ __device__ inline
#endif

constexpr uint32_t PNG_SEG = 32768;         // SM_PNG_SEG: bytes of the filtered stream per IDAT chunk
constexpr uint32_t PNG_SLOT = PNG_SEG + 8;  // a segment's data at most: zlib header 2 + stored header 5 + PNG_SEG
constexpr uint32_t PNG_MAX_ROW = 12288;     // W*bpp up to which the filter kernel stages its rows (5 rows in 60 KiB of LDS)
constexpr int PNG_BLOCK = 256;
constexpr int PNG_DBLOCK = 1024;                 // threads of k_png_deflate: the walks are chains of dependent
                                                 // LDS reads, so short ones on many waves
constexpr int PNG_CHUNK = PNG_SEG / PNG_DBLOCK;  // positions of a segment one thread walks
constexpr int PNG_FILTER_ROWS = 4;              // rows (waves) per workgroup of k_png_filter
constexpr uint32_t PNG_ADLER = 65521u;

// source kinds and disparity modes: SM_PNG_SRC_* / SM_PNG_DISP_* of the header
constexpr int PNG_SRC_U8 = 0, PNG_SRC_U16 = 1, PNG_SRC_DISP_I16 = 2, PNG_SRC_DISP_F32 = 3;
constexpr int PNG_DISP_KITTI = 0, PNG_DISP_LINEAR_U8 = 1;

struct PngSegInfo {
    uint32_t nbytes;  // the chunk's data (without the Adler-32 that follows the last segment)
    uint32_t crc;     // CRC-32 of "IDAT" + data
    uint32_t a, b;    // Adler partial: sum of the bytes, sum of (len - i) * byte[i], both mod 65521
};

struct PngImgInfo {
    uint32_t adler, last_crc;  // the stream's Adler-32; the last chunk's CRC with the Adler bytes in
};

struct PngArgs {
    const uint8_t* img;  // image i at img + i * img_stride, rows row_stride bytes apart
    size_t img_stride, row_stride;
    int H, W;
    int kind, channels, keep, filter, mode;  // sm_png_params
    int lo, hi;                              // LINEAR_U8 bounds
    const int* range;                        // device forms: [img][2] = min d, min -d (or null: lo / hi)
    int bpp, depth, out_channels;            // of the file
    uint32_t rowbytes, nseg;
    uint64_t stream_len;     // (rowbytes + 1) * H
    uint64_t stream_stride;  // bytes between the images' streams (a multiple of 16)
    uint8_t* stream;         // [img][stream_stride]
    uint8_t* slots;          // [img][nseg][PNG_SLOT]
    PngSegInfo* seginfo;     // [img][nseg]
    PngImgInfo* imginfo;     // [img]
    uint64_t* offs;          // [img][nseg] file offset of every chunk
    uint8_t* out;            // file i at out + i * capacity
    uint64_t capacity;
    uint64_t* nbytes;        // [img]
};

// ---------------------------------------------------------------------------------------------
// pixel conversion
// x16 maps: disparity * 256 = d << 4, which fits uint16 up to d = 4095 (disparity 255.9375);
// above, 65535 as for a float32 map
SM_HD uint32_t png_kitti_i16(int d) { return d < 0 ? 0u : d > 4095 ? 65535u : (uint32_t)d << 4; }

SM_HD uint32_t png_kitti_f32(float d)
{
    if (!(d > 0.f) || d == INFINITY) return 0u;  // NaN, -inf, -0, 0, negative; +inf
    const float r = rintf(d * 256.f);            // round to nearest even in float32; d * 256 is exact
    return r >= 65535.f ? 65535u : (uint32_t)r;
}

// clamp((d - lo) * 255 / (hi - lo), 0, 255), round half up, in integers
SM_HD uint32_t png_linear_u8(int d, int lo, int hi)
{
    if (hi <= lo || d <= lo) return 0u;
    if (d >= hi) return 255u;
    const int64_t span = (int64_t)hi - lo;
    return (uint32_t)((((int64_t)d - lo) * 510 + span) / (2 * span));
}

// byte i of the unfiltered row whose source row starts at `row`
SM_HD uint32_t png_raw_byte(const PngArgs& s, const uint8_t* row, uint32_t i, int lo, int hi)
{
    switch (s.kind) {
    case PNG_SRC_U8:
        if (s.channels == 3 && !s.keep) {
            const uint32_t px = i / 3u, c = i - 3u * px;
            return row[3u * px + 2u - c];
        }
        return row[i];
    case PNG_SRC_U16:
        return row[i ^ 1u];  // little-endian samples in memory, big-endian in the file
    case PNG_SRC_DISP_I16: {
        if (s.mode == PNG_DISP_LINEAR_U8) return png_linear_u8(reinterpret_cast<const int16_t*>(row)[i], lo, hi);
        const uint32_t v = png_kitti_i16(reinterpret_cast<const int16_t*>(row)[i >> 1]);
        return (i & 1u) ? (v & 255u) : (v >> 8);
    }
    default: {
        const uint32_t v = png_kitti_f32(reinterpret_cast<const float*>(row)[i >> 1]);
        return (i & 1u) ? (v & 255u) : (v >> 8);
    }
    }
}

// ---------------------------------------------------------------------------------------------
// scanline filters: x the byte, a the byte bpp to the left, b above, c above left (0 outside)
SM_HD uint32_t png_filt(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t pred;
    switch (type) {
    case 0: pred = 0; break;
    case 1: pred = a; break;
    case 2: pred = b; break;
    case 3: pred = (a + b) >> 1; break;
    default: {
        const int p = (int)a + (int)b - (int)c;
        int pa = p - (int)a, pb = p - (int)b, pc = p - (int)c;
        pa = pa < 0 ? -pa : pa, pb = pb < 0 ? -pb : pb, pc = pc < 0 ? -pc : pc;
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    }
    return (x - pred) & 255u;
}

// the bits of v in reverse order
SM_HD uint32_t png_bitrev32(uint32_t v)
{
#if defined(__clang__)
    return __builtin_bitreverse32(v);
#else
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
#endif
}

SM_HD uint32_t png_mag(uint32_t f) { return f < 128u ? f : 256u - f; }

// the type with the smallest sum, ties to the lowest type
SM_HD int png_pick_filter(const uint32_t* sum)
{
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (sum[t] < sum[best]) best = t;
    return best;
}

// ---------------------------------------------------------------------------------------------
// checksums
SM_HD uint32_t png_crc_table_entry(uint32_t n)
{
    uint32_t c = n;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    return c;
}

// register update by one byte without a table
SM_HD uint32_t png_crc_byte(uint32_t reg, uint32_t byte) { return (reg >> 8) ^ png_crc_table_entry((reg ^ byte) & 255u); }

// a * b mod P in the reflected representation (bit 31 is x^0)
SM_HD uint32_t png_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// x^(8 n) mod P; crc(A || B) = png_crc_mul(png_crc_shift(|B|), crc(A)) ^ crc(B) for finished CRCs
SM_HD uint32_t png_crc_shift(uint32_t n)
{
    uint32_t p = 0x80000000u, base = 0x00800000u;  // 1, x^8
    while (n) {
        if (n & 1u) p = png_crc_mul(base, p);
        base = png_crc_mul(base, base);
        n >>= 1;
    }
    return p;
}

// ---------------------------------------------------------------------------------------------
// tokens.  Position i repeats when byte[i] == byte[i - 1] (never at the segment's start).  A maximal
// block of R repeating positions is R / 258 matches of 258 at distance 1, one more match for a
// remainder >= 3, literals for a remainder of 1 or 2.  off: the position's index in its block.
// Returns 0 (inside a match: nothing), 1 (a literal) or 2 (a match of `len` starts here).
SM_HD int png_token(uint32_t off, uint32_t R, uint32_t& len)
{
    const uint32_t full = R / 258u, rem = R - full * 258u, q = off / 258u;
    if (q < full) {
        len = 258u;
        return off == q * 258u ? 2 : 0;
    }
    if (rem >= 3u) {
        len = rem;
        return off == full * 258u ? 2 : 0;
    }
    return 1;
}

// length symbol 257..285 of a match length 3..258 with its extra bits
SM_HD uint32_t png_len_sym(uint32_t len, uint32_t& ebits, uint32_t& eval)
{
    ebits = eval = 0;
    if (len == 258u) return 285u;
    const uint32_t l = len - 3u;
    if (l < 8u) return 257u + l;
    const uint32_t e = (uint32_t)(31 - __builtin_clz(l)) - 2u;
    ebits = e, eval = l & ((1u << e) - 1u);
    return 257u + 4u * (e + 1u) + ((l >> e) & 3u);
}

// ---------------------------------------------------------------------------------------------
// Huffman codes: the optimal code from two queues over the symbols sorted by (count, symbol); a
// code deeper than maxbits is repaired by the counts-per-length method zlib uses (move one leaf
// of the longest length < maxbits down, pair an overflowing leaf with it) and the lengths are
// handed out again in sorted order, the longest to the rarest; canonical codes (RFC 1951
// §3.2.2), bit-reversed for the LSB-first stream.
// The construction is cut into pieces of one element each (a symbol's rank, a node's depth, a
// rank's length, a symbol's code) around the two serial ones (the merge, the repair): the CPU
// calls them in loops (png_huff_build_host), the device a thread an element (png_huff_build_dev).
constexpr int PNG_NLIT = 286;
constexpr int PNG_NSYM_MAX = 288;

struct PngHuffWork {
    uint32_t nfreq[2 * PNG_NSYM_MAX];   // leaves in sorted order, then the internal nodes
    uint16_t parent[2 * PNG_NSYM_MAX];
    uint16_t order[PNG_NSYM_MAX];       // the used symbols by ascending (count, symbol)
    uint32_t blc[16];                   // symbols per code length
    uint32_t n, overflow;               // used symbols; nodes deeper than maxbits
};

// rank of the used symbol s among the used symbols
SM_HD uint32_t png_sort_rank(const uint32_t* freq, int nsym, int s)
{
    const uint32_t fs = freq[s];
    uint32_t r = 0;
    for (int t = 0; t < nsym; ++t) {
        const uint32_t ft = freq[t];
        r += (ft != 0u && (ft < fs || (ft == fs && t < s))) ? 1u : 0u;
    }
    return r;
}

// the tree over the n >= 2 sorted leaves w.nfreq[0 .. n): nodes n .. 2n - 2 (the root) in the order
// they are made; of two equal counts the leaf goes first.  The queues' heads stay in registers.
SM_HD void png_huff_merge(PngHuffWork& w, int n)
{
    int li = 0, ii = n;
    uint32_t lf = w.nfreq[0], lf1 = n > 1 ? w.nfreq[1] : 0u, nf = 0;  // leaf head, the leaf after it, internal head
    for (int k = n; k < 2 * n - 1; ++k) {
        uint32_t f = 0;
        for (int j = 0; j < 2; ++j) {
            if (li < n && (ii >= k || lf <= nf)) {
                f += lf;
                w.parent[li] = (uint16_t)k;
                ++li;
                lf = lf1;
                lf1 = li + 1 < n ? w.nfreq[li + 1] : 0u;
            } else {
                f += nf;
                w.parent[ii] = (uint16_t)k;
                ++ii;
                nf = ii < k ? w.nfreq[ii] : 0u;
            }
        }
        w.nfreq[k] = f;
        if (ii == k) nf = f;  // the internal queue was empty: the new node is its head
    }
}

// depth of node k below the root
SM_HD uint32_t png_node_depth(const PngHuffWork& w, int k, int root)
{
    uint32_t d = 0;
    while (k != root) k = w.parent[k], ++d;
    return d;
}

// w.blc holds the leaves per depth clamped to maxbits, `overflow` the nodes (leaves and internal)
// deeper than maxbits: make room for them
SM_HD void png_huff_repair(PngHuffWork& w, int maxbits, int overflow)
{
    while (overflow > 0) {
        int bits = maxbits - 1;
        while (w.blc[bits] == 0) --bits;
        --w.blc[bits];
        w.blc[bits + 1] += 2;
        --w.blc[maxbits];
        overflow -= 2;
    }
}

// the length of the leaf of rank k (0 the rarest): the longest lengths first
SM_HD uint32_t png_len_of_rank(const uint32_t* blc, int maxbits, uint32_t k)
{
    uint32_t acc = 0;
    for (int bits = maxbits; bits >= 1; --bits) {
        acc += blc[bits];
        if (k < acc) return (uint32_t)bits;
    }
    return 0;
}

// the canonical code of symbol s: the first code of its length plus the symbols of that length
// before it, bit-reversed
SM_HD uint32_t png_code_of(const uint8_t* len, const uint32_t* blc, int s)
{
    const uint32_t l = len[s];
    if (!l) return 0;
    uint32_t c = 0;
    for (uint32_t b = 2; b <= l; ++b) c = (c + blc[b - 1]) << 1;
    for (int t = 0; t < s; ++t) c += len[t] == l ? 1u : 0u;
    return png_bitrev32(c) >> (32u - l);
}

inline void png_huff_build_host(const uint32_t* freq, int nsym, int maxbits, uint8_t* len, uint16_t* code, PngHuffWork& w)
{
    int n = 0;
    for (int b = 0; b < 16; ++b) w.blc[b] = 0;
    for (int s = 0; s < nsym; ++s) {
        len[s] = 0;
        if (freq[s]) {
            const uint32_t r = png_sort_rank(freq, nsym, s);
            w.order[r] = (uint16_t)s, w.nfreq[r] = freq[s];
            ++n;
        }
    }
    if (n >= 2) {
        png_huff_merge(w, n);
        int overflow = 0;
        for (int k = 0; k < 2 * n - 2; ++k) {
            uint32_t d = png_node_depth(w, k, 2 * n - 2);
            if (d > (uint32_t)maxbits) d = (uint32_t)maxbits, ++overflow;
            if (k < n) ++w.blc[d];
        }
        png_huff_repair(w, maxbits, overflow);
    } else if (n == 1) {
        w.blc[1] = 1;
    }
    for (int k = 0; k < n; ++k) len[w.order[k]] = (uint8_t)png_len_of_rank(w.blc, maxbits, (uint32_t)k);
    for (int s = 0; s < nsym; ++s) code[s] = (uint16_t)png_code_of(len, w.blc, s);
}

#if defined(__HIPCC__)
// the same by all threads of a workgroup (w, len and code in LDS)
__device__ inline void png_huff_build_dev(const uint32_t* freq, int nsym, int maxbits, uint8_t* len, uint16_t* code,
                                          PngHuffWork& w)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid < 16) w.blc[tid] = 0;
    if (tid == 0) w.n = 0, w.overflow = 0;
    for (int s = tid; s < nsym; s += nt) len[s] = 0;
    __syncthreads();
    for (int s = tid; s < nsym; s += nt)
        if (freq[s]) {
            const uint32_t r = png_sort_rank(freq, nsym, s);
            w.order[r] = (uint16_t)s, w.nfreq[r] = freq[s];
            atomicAdd(&w.n, 1u);
        }
    __syncthreads();
    const int n = (int)w.n;  // workgroup-uniform
    if (n >= 2) {
        if (tid == 0) png_huff_merge(w, n);
        __syncthreads();
        for (int k = tid; k < 2 * n - 2; k += nt) {
            uint32_t d = png_node_depth(w, k, 2 * n - 2);
            if (d > (uint32_t)maxbits) d = (uint32_t)maxbits, atomicAdd(&w.overflow, 1u);
            if (k < n) atomicAdd(&w.blc[d], 1u);
        }
        __syncthreads();
        if (tid == 0) png_huff_repair(w, maxbits, (int)w.overflow);
    } else if (n == 1 && tid == 0) {
        w.blc[1] = 1;
    }
    __syncthreads();
    for (int k = tid; k < n; k += nt) len[w.order[k]] = (uint8_t)png_len_of_rank(w.blc, maxbits, (uint32_t)k);
    __syncthreads();
    for (int s = tid; s < nsym; s += nt) code[s] = (uint16_t)png_code_of(len, w.blc, s);
    __syncthreads();
}
#endif

// LSB-first bit writer into zeroed 32-bit words.  On the device the words are shared by the
// workgroup's threads, so every word goes in by an atomic OR.
struct PngBits {
    uint32_t* words;
    uint32_t w;      // word the pending bits begin in
    uint32_t cnt;    // pending bits (< 32 between calls), the first (pos & 31) of them zeros
    uint64_t acc;

    SM_HD void start(uint32_t* words_, uint32_t bitpos) { words = words_, w = bitpos >> 5, cnt = bitpos & 31u, acc = 0; }
    SM_HD uint32_t pos() const { return (w << 5) + cnt; }
    SM_HD void or_word(uint32_t v)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        if (v) atomicOr(&words[w], v);
#else
        words[w] |= v;
#endif
    }
    SM_HD void put(uint32_t bits, uint32_t n)  // n <= 32
    {
        acc |= (uint64_t)bits << cnt;
        cnt += n;
        if (cnt >= 32u) {
            or_word((uint32_t)acc);
            acc >>= 32;
            cnt -= 32u;
            ++w;
        }
    }
    SM_HD void flush()
    {
        if (cnt) or_word((uint32_t)acc);
        acc = 0;  // a later put goes on from the same position: the bits written stay (OR)
    }
};

struct PngTables {
    uint32_t freq[PNG_NSYM_MAX];  // lit/len counts
    uint16_t code[PNG_NSYM_MAX];
    uint8_t len[PNG_NSYM_MAX];
    uint32_t clfreq[20];
    uint16_t clcode[20];
    uint8_t cllen[20];
    uint16_t cltok[PNG_NSYM_MAX + 8];  // code-length symbols: symbol | extra << 5
    uint8_t seq[PNG_NSYM_MAX];         // the lit/len lengths followed by the distance length
    PngHuffWork w;
};

// the token's bits and their count: a literal, or a match (length code, extra bits, the one-bit
// distance code 0)
SM_HD uint32_t png_lit_bits(const PngTables& t, uint32_t byte, uint32_t& n)
{
    n = t.len[byte];
    return t.code[byte];
}

SM_HD uint32_t png_match_bits(const PngTables& t, uint32_t mlen, uint32_t& n)
{
    uint32_t eb, ev;
    const uint32_t sym = png_len_sym(mlen, eb, ev), l = t.len[sym];
    n = l + eb + 1u;
    return (uint32_t)t.code[sym] | (ev << l);
}

// The block's header after the lit/len code is made: BFINAL, BTYPE = dynamic, HLIT, HDIST = one
// code (one bit when a match exists, else the zero-length code), HCLEN and the code lengths
// through the code-length code.  Three steps: png_hdr_tokens (serial: t.seq and its run-length
// tokens, counted in t.clfreq), the code-length code from t.clfreq, png_hdr_emit (serial).

// lit/len codes sent (257 .. 286): up to the last used symbol
SM_HD int png_hdr_nlit(const PngTables& t)
{
    int nlit = PNG_NLIT;
    while (nlit > 257 && t.len[nlit - 1] == 0) --nlit;
    return nlit;
}

// t.seq = the nlit lit/len lengths and the distance length; their tokens into t.cltok (16 repeats
// the previous length 3..6 times, 17 / 18 are 3..10 / 11..138 zeros), counted in t.clfreq (zeroed
// by the caller); returns the number of tokens
SM_HD int png_hdr_tokens(PngTables& t, int nlit)
{
    bool any_match = false;
    for (int s = 257; s < nlit; ++s) any_match = any_match || t.len[s] != 0;
    for (int s = 0; s < nlit; ++s) t.seq[s] = t.len[s];
    t.seq[nlit] = any_match ? 1 : 0;
    const int nl = nlit + 1;
    int ncl = 0;
    auto emit = [&](uint32_t sym, uint32_t extra) {
        t.cltok[ncl++] = (uint16_t)(sym | (extra << 5));
        ++t.clfreq[sym];
    };
    for (int i = 0; i < nl;) {
        const uint32_t v = t.seq[i];
        int run = 1;
        while (i + run < nl && t.seq[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run > 0) {
                if (run >= 11) {
                    const int k = run < 138 ? run : 138;
                    emit(18u, (uint32_t)(k - 11));
                    run -= k;
                } else if (run >= 3) {
                    emit(17u, (uint32_t)(run - 3));
                    run = 0;
                } else {
                    emit(0u, 0u);
                    --run;
                }
            }
        } else {
            emit(v, 0u);
            --run;
            while (run >= 3) {
                const int k = run < 6 ? run : 6;
                emit(16u, (uint32_t)(k - 3));
                run -= k;
            }
            for (; run > 0; --run) emit(v, 0u);
        }
    }
    return ncl;
}

SM_HD void png_hdr_emit(const PngTables& t, PngBits& bw, bool last, int nlit, int ncl)
{
    const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 19;
    while (hclen > 4 && t.cllen[ord[hclen - 1]] == 0) --hclen;
    bw.put((last ? 1u : 0u) | (2u << 1), 3);
    bw.put((uint32_t)(nlit - 257), 5);
    bw.put(0u, 5);
    bw.put((uint32_t)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) bw.put(t.cllen[ord[k]], 3);
    for (int k = 0; k < ncl; ++k) {
        const uint32_t sym = t.cltok[k] & 31u, ex = t.cltok[k] >> 5;
        bw.put(t.clcode[sym], t.cllen[sym]);
        if (sym == 16u) bw.put(ex, 2);
        else if (sym == 17u) bw.put(ex, 3);
        else if (sym == 18u) bw.put(ex, 7);
    }
}

// all of it on the CPU: the lit/len code from t.freq and the header at bw
inline void png_dyn_header_host(PngTables& t, PngBits& bw, bool last)
{
    png_huff_build_host(t.freq, PNG_NLIT, 15, t.len, t.code, t.w);
    const int nlit = png_hdr_nlit(t);
    for (int s = 0; s < 20; ++s) t.clfreq[s] = 0;
    const int ncl = png_hdr_tokens(t, nlit);
    png_huff_build_host(t.clfreq, 19, 7, t.cllen, t.clcode, t.w);
    png_hdr_emit(t, bw, last, nlit, ncl);
}

// bytes of the segment's data as a dynamic block that ends at bit `end` (after the end-of-block
// code), with the empty stored block that closes a segment which is not the last
SM_HD uint32_t png_dyn_bytes(uint32_t end, bool last) { return last ? (end + 7u) >> 3 : ((end + 3u + 7u) >> 3) + 4u; }

// ... and as a stored block of n bytes from byte `base` (2 after the zlib header, else 0)
SM_HD uint32_t png_stored_bytes(uint32_t base, uint32_t n) { return base + 5u + n; }

// the end of a dynamic block: end-of-block code at bit `at`, then the closing bytes
SM_HD void png_dyn_finish(const PngTables& t, PngBits& bw, bool last)
{
    bw.put(t.code[256], t.len[256]);
    if (!last) {
        bw.put(0u, 3);
        const uint32_t pad = (8u - (bw.pos() & 7u)) & 7u;
        bw.put(0u, pad);
        bw.put(0u, 16);
        bw.put(0xFFFFu, 16);
    }
    bw.flush();
}

// the five header bytes of a stored block of n bytes
SM_HD void png_stored_header(uint8_t* o, uint32_t n, bool last)
{
    o[0] = last ? 1 : 0;
    o[1] = (uint8_t)(n & 255u), o[2] = (uint8_t)(n >> 8);
    o[3] = (uint8_t)(~n & 255u), o[4] = (uint8_t)((~n >> 8) & 255u);
}

SM_HD void png_put_be32(uint8_t* o, uint32_t v)
{
    o[0] = (uint8_t)(v >> 24), o[1] = (uint8_t)(v >> 16), o[2] = (uint8_t)(v >> 8), o[3] = (uint8_t)v;
}

// the 33 bytes before the first chunk: signature and IHDR
SM_HD void png_file_head(const PngArgs& s, uint8_t* o)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) o[i] = sig[i];
    png_put_be32(o + 8, 13u);
    o[12] = 'I', o[13] = 'H', o[14] = 'D', o[15] = 'R';
    png_put_be32(o + 16, (uint32_t)s.W);
    png_put_be32(o + 20, (uint32_t)s.H);
    o[24] = (uint8_t)s.depth, o[25] = s.out_channels == 3 ? 2 : 0, o[26] = 0, o[27] = 0, o[28] = 0;
    uint32_t reg = 0xFFFFFFFFu;
    for (int i = 12; i < 29; ++i) reg = png_crc_byte(reg, o[i]);
    png_put_be32(o + 29, ~reg);
}

// the 12 bytes of IEND
SM_HD void png_file_tail(uint8_t* o)
{
    png_put_be32(o, 0u);
    o[4] = 'I', o[5] = 'E', o[6] = 'N', o[7] = 'D';
    png_put_be32(o + 8, 0xAE426082u);
}

// the last chunk's CRC once the Adler-32 follows its data
SM_HD uint32_t png_crc_append_be32(uint32_t crc, uint32_t v)
{
    uint32_t reg = ~crc;
    reg = png_crc_byte(reg, v >> 24), reg = png_crc_byte(reg, (v >> 16) & 255u);
    reg = png_crc_byte(reg, (v >> 8) & 255u), reg = png_crc_byte(reg, v & 255u);
    return ~reg;
}

// ---------------------------------------------------------------------------------------------
// the CPU twin: the same functions, one after the other
// one row of the filtered stream; cur / up: the unfiltered rows (up all zeros above row 0)
inline void png_filter_row_host(const PngArgs& s, const uint8_t* cur, const uint8_t* up, uint8_t* dst)
{
    const uint32_t n = s.rowbytes, bpp = (uint32_t)s.bpp;
    int type = s.filter;
    if (type < 0) {
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t a = i >= bpp ? cur[i - bpp] : 0u, c = i >= bpp ? up[i - bpp] : 0u;
            for (int t = 0; t < 5; ++t) sum[t] += png_mag(png_filt(t, cur[i], a, up[i], c));
        }
        type = png_pick_filter(sum);
    }
    dst[0] = (uint8_t)type;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t a = i >= bpp ? cur[i - bpp] : 0u, c = i >= bpp ? up[i - bpp] : 0u;
        dst[1 + i] = (uint8_t)png_filt(type, cur[i], a, up[i], c);
    }
}

// one segment: data into out (PNG_SLOT bytes, 4-byte aligned), its info returned
inline PngSegInfo png_deflate_segment_host(const uint8_t* seg, uint32_t n, bool first, bool last, uint8_t* out,
                                           PngTables& t)
{
    uint32_t* words = reinterpret_cast<uint32_t*>(out);
    for (uint32_t i = 0; i < PNG_SLOT / 4; ++i) words[i] = 0;
    for (int s = 0; s < PNG_NSYM_MAX; ++s) t.freq[s] = 0;
    // run ends: for a repeating position, the end of its block
    auto walk = [&](auto&& lit, auto&& match) {
        uint32_t i = 0;
        while (i < n) {
            if (i == 0 || seg[i] != seg[i - 1]) {
                lit(seg[i]);
                ++i;
                continue;
            }
            uint32_t e = i + 1;
            while (e < n && seg[e] == seg[i]) ++e;
            const uint32_t R = e - i;
            for (uint32_t off = 0; off < R; ++off) {
                uint32_t len;
                const int k = png_token(off, R, len);
                if (k == 1) lit(seg[i]);
                else if (k == 2) match(len);
            }
            i = e;
        }
    };
    walk([&](uint32_t b) { ++t.freq[b]; },
         [&](uint32_t len) {
             uint32_t eb, ev;
             ++t.freq[png_len_sym(len, eb, ev)];
         });
    t.freq[256] = 1;
    const uint32_t base = first ? 2u : 0u;
    if (first) words[0] = 0x0178u;
    PngBits bw;
    bw.start(words, base * 8u);
    png_dyn_header_host(t, bw, last);
    uint64_t tokbits = 0;
    walk([&](uint32_t b) { tokbits += t.len[b]; },
         [&](uint32_t len) {
             uint32_t nb;
             png_match_bits(t, len, nb);
             tokbits += nb;
         });
    const uint64_t end = (uint64_t)bw.pos() + tokbits + t.len[256];
    const uint32_t stored = png_stored_bytes(base, n);
    PngSegInfo info;
    if (end > 8ull * stored || png_dyn_bytes((uint32_t)end, last) > stored) {
        png_stored_header(out + base, n, last);
        for (uint32_t i = 0; i < n; ++i) out[base + 5u + i] = seg[i];
        info.nbytes = stored;
    } else {
        walk([&](uint32_t b) {
                 uint32_t nb;
                 const uint32_t v = png_lit_bits(t, b, nb);
                 bw.put(v, nb);
             },
             [&](uint32_t len) {
                 uint32_t nb;
                 const uint32_t v = png_match_bits(t, len, nb);
                 bw.put(v, nb);
             });
        png_dyn_finish(t, bw, last);
        info.nbytes = png_dyn_bytes((uint32_t)end, last);
    }
    uint32_t reg = 0xFFFFFFFFu;
    const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
    for (int i = 0; i < 4; ++i) reg = png_crc_byte(reg, idat[i]);
    for (uint32_t i = 0; i < info.nbytes; ++i) reg = png_crc_byte(reg, out[i]);
    info.crc = ~reg;
    uint64_t a = 0, b = 0;
    for (uint32_t i = 0; i < n; ++i) a += seg[i], b += (uint64_t)(n - i) * seg[i];
    info.a = (uint32_t)(a % PNG_ADLER), info.b = (uint32_t)(b % PNG_ADLER);
    return info;
}

// the whole file of one image (s.img on the host; s.lo / s.hi set), appended to `file`
inline void png_encode_host(const PngArgs& s, std::vector<uint8_t>& file)
{
    const uint32_t n = s.rowbytes;
    std::vector<uint8_t> stream(s.stream_len), rows(2 * (size_t)n, 0);
    uint8_t* up = rows.data();
    uint8_t* cur = up + n;
    for (int y = 0; y < s.H; ++y) {
        const uint8_t* row = s.img + (size_t)y * s.row_stride;
        for (uint32_t i = 0; i < n; ++i) cur[i] = (uint8_t)png_raw_byte(s, row, i, s.lo, s.hi);
        png_filter_row_host(s, cur, up, stream.data() + (size_t)y * (n + 1u));
        std::swap(cur, up);
    }
    file.resize(33);
    png_file_head(s, file.data());
    std::vector<uint32_t> slot(PNG_SLOT / 4 + 2);
    std::vector<PngTables> tab(1);
    uint64_t asum = 1, bsum = 0;
    for (uint32_t seg = 0; seg < s.nseg; ++seg) {
        const uint64_t s0 = (uint64_t)seg * PNG_SEG;
        const uint32_t len = (uint32_t)std::min<uint64_t>(PNG_SEG, s.stream_len - s0);
        const bool last = seg + 1 == s.nseg;
        uint8_t* data = reinterpret_cast<uint8_t*>(slot.data());
        const PngSegInfo v = png_deflate_segment_host(stream.data() + s0, len, seg == 0, last, data, tab[0]);
        bsum = (bsum + v.b + (uint64_t)len * asum) % PNG_ADLER;
        asum = (asum + v.a) % PNG_ADLER;
        const uint32_t adler = (uint32_t)((bsum << 16) | asum);
        const size_t at = file.size();
        const uint32_t ndata = v.nbytes + (last ? 4u : 0u);
        file.resize(at + 12 + ndata);
        uint8_t* o = file.data() + at;
        png_put_be32(o, ndata);
        o[4] = 'I', o[5] = 'D', o[6] = 'A', o[7] = 'T';
        std::memcpy(o + 8, data, v.nbytes);
        if (last) png_put_be32(o + 8 + v.nbytes, adler);
        png_put_be32(o + 8 + ndata, last ? png_crc_append_be32(v.crc, adler) : v.crc);
    }
    const size_t at = file.size();
    file.resize(at + 12);
    png_file_tail(file.data() + at);
}

// ---------------------------------------------------------------------------------------------
// kernels (left out when a host compiler reads this header for the CPU twins alone)
#if defined(__HIPCC__)

// per image the minimum of d and of -d of an int16 map: keys[img][2], initialised to INT_MAX
__global__ void __launch_bounds__(PNG_BLOCK) k_png_minmax(PngArgs a, int* keys)
{
    __shared__ int wmin[PNG_BLOCK / 64], wneg[PNG_BLOCK / 64];
    const int tid = threadIdx.x, img = blockIdx.y;
    const uint8_t* base = a.img + (size_t)img * a.img_stride;
    int mn = 0x7FFFFFFF, ng = 0x7FFFFFFF;
    for (int y = blockIdx.x; y < a.H; y += gridDim.x) {
        const int16_t* row = reinterpret_cast<const int16_t*>(base + (size_t)y * a.row_stride);
        for (int x = tid; x < a.W; x += PNG_BLOCK) {
            const int d = row[x];
            mn = d < mn ? d : mn, ng = -d < ng ? -d : ng;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int m2 = __shfl_xor(mn, o), n2 = __shfl_xor(ng, o);
        mn = m2 < mn ? m2 : mn, ng = n2 < ng ? n2 : ng;
    }
    if ((tid & 63) == 0) wmin[tid >> 6] = mn, wneg[tid >> 6] = ng;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PNG_BLOCK / 64; ++w) {
            mn = wmin[w] < mn ? wmin[w] : mn;
            ng = wneg[w] < ng ? wneg[w] : ng;
        }
        atomicMin(&keys[2 * img], mn);
        atomicMin(&keys[2 * img + 1], ng);
    }
}

// PNG_FILTER_ROWS rows a workgroup, a wave each: the five candidate sums reduced across the wave,
// the chosen row written.  STAGED: the rows and the one above them are converted into LDS once
// (rows of at most PNG_MAX_ROW bytes); else every byte is converted where it is used.
template <bool STAGED>
__global__ void __launch_bounds__(PNG_BLOCK) k_png_filter(PngArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t png_rows[];  // [PNG_FILTER_ROWS + 1][pitch]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y;
    const uint32_t n = a.rowbytes, pitch = (n + 3u) & ~3u, bpp = (uint32_t)a.bpp;
    const int y0 = blockIdx.x * PNG_FILTER_ROWS;
    const uint8_t* base = a.img + (size_t)img * a.img_stride;
    int lo = a.lo, hi = a.hi;
    if (a.range) lo = a.range[2 * img], hi = -a.range[2 * img + 1];
    if (STAGED) {
        for (int r = 0; r <= PNG_FILTER_ROWS; ++r) {
            const int y = y0 - 1 + r;
            const bool in = y >= 0 && y < a.H;  // workgroup-uniform
            const uint8_t* row = base + (size_t)(in ? y : 0) * a.row_stride;
            for (uint32_t i = tid; i < n; i += PNG_BLOCK)
                png_rows[r * pitch + i] = in ? (uint8_t)png_raw_byte(a, row, i, lo, hi) : 0;
        }
        __syncthreads();
    }
    const int y = y0 + wave;
    if (y >= a.H) return;
    const uint8_t* up = png_rows + wave * pitch;
    const uint8_t* cur = up + pitch;
    const uint8_t* src_cur = base + (size_t)y * a.row_stride;
    const uint8_t* src_up = base + (size_t)(y > 0 ? y - 1 : 0) * a.row_stride;
    auto cur_at = [&](uint32_t i) -> uint32_t { return STAGED ? cur[i] : png_raw_byte(a, src_cur, i, lo, hi); };
    auto up_at = [&](uint32_t i) -> uint32_t { return STAGED ? up[i] : (y > 0 ? png_raw_byte(a, src_up, i, lo, hi) : 0u); };
    int type = a.filter;
    if (type < 0) {
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t i = lane; i < n; i += 64) {
            const uint32_t x = cur_at(i), b = up_at(i), l = i >= bpp ? cur_at(i - bpp) : 0u, c = i >= bpp ? up_at(i - bpp) : 0u;
#pragma unroll
            for (int t = 0; t < 5; ++t) sum[t] += png_mag(png_filt(t, x, l, b, c));
        }
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum[t] += __shfl_xor(sum[t], o);
        type = png_pick_filter(sum);
    }
    uint8_t* dst = a.stream + (size_t)img * a.stream_stride + (size_t)y * (n + 1u);
    if (lane == 0) dst[0] = (uint8_t)type;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t l = i >= bpp ? cur_at(i - bpp) : 0u, c = i >= bpp ? up_at(i - bpp) : 0u;
        dst[1 + i] = (uint8_t)png_filt(type, cur_at(i), l, up_at(i), c);
    }
}

// position i of the segment in LDS: four bytes of padding after every thread's PNG_CHUNK
// positions, so that the threads' walks start on different banks
__device__ inline uint32_t png_lds_at(uint32_t i) { return i + ((i / PNG_CHUNK) << 2); }
constexpr uint32_t PNG_SEG_LDS = PNG_SEG + (PNG_SEG / PNG_CHUNK) * 4;
constexpr uint32_t PNG_OUT_WORDS = PNG_SLOT / 4 + 2;

struct PngDeflateLds {
    uint8_t seg[PNG_SEG_LDS];
    uint32_t out[PNG_OUT_WORDS];
    PngTables t;
    uint32_t crc_table[256];
    int wlast[PNG_DBLOCK / 64];        // per wave: its last non-repeating position, or -1
    uint32_t wfirst[PNG_DBLOCK / 64];  // its first one, or n
    uint32_t wsum[PNG_DBLOCK / 64], wa[PNG_DBLOCK / 64], wb[PNG_DBLOCK / 64], wc[PNG_DBLOCK / 64];
    uint32_t hdr_end;
    int ncl;
};

// the tokens of positions [c0, c1) in order.  prev_nr: the last non-repeating position before c0;
// next_nr: the first one at or after c1 (n when there is none).
template <class L, class M>
__device__ inline void png_walk(const uint8_t* seg, uint32_t c0, uint32_t c1, int prev_nr, uint32_t next_nr, L&& lit,
                                M&& match)
{
    uint32_t i = c0;
    while (i < c1) {
        const uint32_t b = seg[png_lds_at(i)];
        if (i == 0 || b != seg[png_lds_at(i - 1)]) {
            lit(b);
            ++i;
            continue;
        }
        const uint32_t rs = i == c0 ? (uint32_t)(prev_nr + 1) : i;  // a block met past c0 begins there
        uint32_t e = i + 1;
        while (e < c1 && seg[png_lds_at(e)] == b) ++e;
        const uint32_t stop = e;
        if (e == c1) e = next_nr;
        const uint32_t R = e - rs;
        for (; i < stop; ++i) {
            uint32_t len;
            const int k = png_token(i - rs, R, len);
            if (k == 1) lit(b);
            else if (k == 2) match(len);
        }
    }
}

__global__ void __launch_bounds__(PNG_DBLOCK) k_png_deflate(PngArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds_raw[];
    PngDeflateLds& S = *reinterpret_cast<PngDeflateLds*>(png_lds_raw);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, seg = blockIdx.x, img = blockIdx.y;
    const bool first = seg == 0, last = seg + 1 == a.nseg;
    const uint64_t s0 = (uint64_t)seg * PNG_SEG;
    const uint32_t n = (uint32_t)(a.stream_len - s0 < PNG_SEG ? a.stream_len - s0 : PNG_SEG);
    const uint8_t* src = a.stream + (size_t)img * a.stream_stride + s0;  // 16-byte aligned
    for (uint32_t wi = tid; wi < n / 4u; wi += PNG_DBLOCK)
        *reinterpret_cast<uint32_t*>(&S.seg[png_lds_at(4u * wi)]) = reinterpret_cast<const uint32_t*>(src)[wi];
    if (tid < (n & 3u)) S.seg[png_lds_at((n & ~3u) + tid)] = src[(n & ~3u) + tid];
    for (uint32_t i = tid; i < PNG_OUT_WORDS; i += PNG_DBLOCK) S.out[i] = 0;
    for (uint32_t i = tid; i < PNG_NSYM_MAX; i += PNG_DBLOCK) S.t.freq[i] = 0;
    if (tid < 256u) S.crc_table[tid] = png_crc_table_entry(tid);
    __syncthreads();

    // every thread's PNG_CHUNK positions: its non-repeating ends, and the Adler sums
    const uint32_t c0 = tid * PNG_CHUNK < n ? tid * PNG_CHUNK : n, c1 = c0 + PNG_CHUNK < n ? c0 + PNG_CHUNK : n;
    int prev_nr;       // the last non-repeating position before c0
    uint32_t next_nr;  // the first one at or after c1, or n
    {
        int lnr = -1;
        uint32_t fnr = n, sa = 0, sb = 0;
        for (uint32_t i = c0; i < c1; ++i) {
            const uint32_t b = S.seg[png_lds_at(i)];
            if (i == 0 || b != S.seg[png_lds_at(i - 1)]) {
                lnr = (int)i;
                fnr = fnr == n ? i : fnr;
            }
            sa += b, sb += (n - i) * b;  // below 32 * 255 * 32768 < 2^32
        }
        // exclusive scans over the threads: the maximum of lnr before, the minimum of fnr behind
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int l2 = __shfl_up(lnr, o);
            const uint32_t f2 = __shfl_down(fnr, o);
            if (lane >= (uint32_t)o) lnr = l2 > lnr ? l2 : lnr;
            if (lane + (uint32_t)o < 64u) fnr = f2 < fnr ? f2 : fnr;
        }
        if (lane == 63u) S.wlast[wave] = lnr;
        if (lane == 0u) S.wfirst[wave] = fnr;
        prev_nr = __shfl_up(lnr, 1);
        next_nr = __shfl_down(fnr, 1);
        if (lane == 0u) prev_nr = -1;
        if (lane == 63u) next_nr = n;
        sa %= PNG_ADLER, sb %= PNG_ADLER;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sa += __shfl_xor(sa, o), sb += __shfl_xor(sb, o);
        if (lane == 0) S.wa[wave] = sa, S.wb[wave] = sb;
    }
    __syncthreads();
    for (uint32_t w = 0; w < PNG_DBLOCK / 64; ++w) {
        const int l = S.wlast[w];
        const uint32_t f = S.wfirst[w];
        if (w < wave) prev_nr = l > prev_nr ? l : prev_nr;
        if (w > wave) next_nr = f < next_nr ? f : next_nr;
    }
    const uint8_t* sg = S.seg;
    PngTables& T = S.t;

    // counts
    png_walk(sg, c0, c1, prev_nr, next_nr, [&](uint32_t b) { atomicAdd(&T.freq[b], 1u); },
             [&](uint32_t len) {
                 uint32_t eb, ev;
                 atomicAdd(&T.freq[png_len_sym(len, eb, ev)], 1u);
             });
    if (tid == 0) atomicAdd(&T.freq[256], 1u);
    __syncthreads();
    // the lit/len code by all threads; the header's tokens and its bits by one lane, the
    // code-length code between them by all threads again
    png_huff_build_dev(T.freq, PNG_NLIT, 15, T.len, T.code, T.w);
    const int nlit = png_hdr_nlit(T);
    if (tid < 20) T.clfreq[tid] = 0;
    __syncthreads();
    if (tid == 0) S.ncl = png_hdr_tokens(T, nlit);
    __syncthreads();
    png_huff_build_dev(T.clfreq, 19, 7, T.cllen, T.clcode, T.w);
    const uint32_t base = first ? 2u : 0u;
    if (tid == 0) {
        if (first) S.out[0] = 0x0178u;
        PngBits bw;
        bw.start(S.out, base * 8u);
        png_hdr_emit(T, bw, last, nlit, S.ncl);
        bw.flush();
        S.hdr_end = bw.pos();
    }
    __syncthreads();

    // bit offsets: every thread's token bits, scanned over the workgroup
    uint32_t mybits = 0;
    png_walk(sg, c0, c1, prev_nr, next_nr, [&](uint32_t b) { mybits += T.len[b]; },
             [&](uint32_t len) {
                 uint32_t nb;
                 png_match_bits(T, len, nb);
                 mybits += nb;
             });
    uint32_t incl = mybits;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += v;
    }
    if (lane == 63u) S.wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tokbits = 0;
    for (uint32_t w = 0; w < PNG_DBLOCK / 64; ++w) {
        const uint32_t x = S.wsum[w];
        if (w < wave) before += x;
        tokbits += x;
    }
    // at most 32768 * 15 token bits: no overflow
    const uint32_t tok0 = S.hdr_end, end = tok0 + tokbits + T.len[256];
    const uint32_t stored = png_stored_bytes(base, n);
    uint32_t nbytes;
    uint8_t* out8 = reinterpret_cast<uint8_t*>(S.out);
    if (end > 8u * stored || png_dyn_bytes(end, last) > stored) {  // workgroup-uniform
        nbytes = stored;
        if (tid == 0) png_stored_header(out8 + base, n, last);
        for (uint32_t i = tid; i < n; i += PNG_DBLOCK) out8[base + 5u + i] = sg[png_lds_at(i)];
    } else {
        nbytes = png_dyn_bytes(end, last);
        PngBits bw;
        bw.start(S.out, tok0 + before + incl - mybits);
        png_walk(sg, c0, c1, prev_nr, next_nr,
                 [&](uint32_t b) {
                     uint32_t nb;
                     const uint32_t v = png_lit_bits(T, b, nb);
                     bw.put(v, nb);
                 },
                 [&](uint32_t len) {
                     uint32_t nb;
                     const uint32_t v = png_match_bits(T, len, nb);
                     bw.put(v, nb);
                 });
        bw.flush();
        if (tid == PNG_DBLOCK - 1) {
            bw.start(S.out, tok0 + tokbits);
            png_dyn_finish(T, bw, last);
        }
    }
    __syncthreads();

    // CRC-32 of "IDAT" + data: equal slices, joined by x^(8 * bytes behind the slice) mod P
    {
        const uint32_t per = ((nbytes + PNG_DBLOCK - 1) / PNG_DBLOCK + 3u) & ~3u;
        const uint32_t b0 = tid * per < nbytes ? tid * per : nbytes, b1 = b0 + per < nbytes ? b0 + per : nbytes;
        uint32_t reg = 0xFFFFFFFFu;
        if (tid == 0) {
            const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
            for (int i = 0; i < 4; ++i) reg = (reg >> 8) ^ S.crc_table[(reg ^ idat[i]) & 255u];
        }
        for (uint32_t i = b0; i < b1; ++i) reg = (reg >> 8) ^ S.crc_table[(reg ^ out8[i]) & 255u];
        uint32_t part = 0;
        if (b1 > b0 || tid == 0) part = png_crc_mul(png_crc_shift(nbytes - b1), ~reg);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part ^= __shfl_xor(part, o);
        if (lane == 0) S.wc[wave] = part;
    }
    uint8_t* slot = a.slots + ((size_t)img * a.nseg + seg) * PNG_SLOT;
    for (uint32_t wi = tid; wi < (nbytes + 3u) / 4u; wi += PNG_DBLOCK) reinterpret_cast<uint32_t*>(slot)[wi] = S.out[wi];
    __syncthreads();
    if (tid == 0) {
        PngSegInfo info;
        info.nbytes = nbytes;
        uint32_t crc = 0, sa = 0, sb = 0;
        for (uint32_t w = 0; w < PNG_DBLOCK / 64; ++w) crc ^= S.wc[w], sa += S.wa[w], sb += S.wb[w];
        info.crc = crc, info.a = sa % PNG_ADLER, info.b = sb % PNG_ADLER;
        a.seginfo[(size_t)img * a.nseg + seg] = info;
    }
}

// the file's size and everything outside the chunks, a workgroup an image.  Chunk s holds
// 12 + nbytes[s] bytes (+ 4, the Adler-32, in the last one); the stream's Adler-32 from the
// partials: a = 1 + sum a_s, b = sum (b_s + len_s * (1 + sum of the a before s)).
__global__ void __launch_bounds__(PNG_BLOCK) k_png_assemble(PngArgs a)
{
    __shared__ unsigned long long wsz[PNG_BLOCK / 64], wad[PNG_BLOCK / 64], wbs[PNG_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, img = blockIdx.x;
    const PngSegInfo* si = a.seginfo + (size_t)img * a.nseg;
    uint64_t* offs = a.offs + (size_t)img * a.nseg;
    unsigned long long at = 33, asum = 1, bsum = 0;  // running: file offset, Adler a, Adler b (not reduced)
    for (uint32_t s0 = 0; s0 < a.nseg; s0 += PNG_BLOCK) {
        const uint32_t s = s0 + tid;
        const bool in = s < a.nseg;
        PngSegInfo v{};
        if (in) v = si[s];
        const unsigned long long len = in ? (uint64_t)((a.stream_len - (uint64_t)s * PNG_SEG < PNG_SEG)
                                                            ? a.stream_len - (uint64_t)s * PNG_SEG
                                                            : PNG_SEG)
                                          : 0ull;
        const unsigned long long sz = in ? 12ull + v.nbytes + (s + 1 == a.nseg ? 4ull : 0ull) : 0ull;
        unsigned long long isz = sz, iad = v.a;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long x = __shfl_up(isz, o), y = __shfl_up(iad, o);
            if (lane >= (uint32_t)o) isz += x, iad += y;
        }
        if (lane == 63u) wsz[wave] = isz, wad[wave] = iad;
        __syncthreads();
        unsigned long long bsz = 0, bad = 0, tsz = 0, tad = 0;
        for (uint32_t w = 0; w < PNG_BLOCK / 64; ++w) {
            if (w < wave) bsz += wsz[w], bad += wad[w];
            tsz += wsz[w], tad += wad[w];
        }
        if (in) offs[s] = at + bsz + isz - sz;
        const unsigned long long a_before = (asum + bad + iad - v.a) % PNG_ADLER;
        unsigned long long bterm = in ? (v.b + len * a_before) % PNG_ADLER : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bterm += __shfl_xor(bterm, o);
        __syncthreads();
        if (lane == 0) wbs[wave] = bterm;
        __syncthreads();
        at += tsz, asum = (asum + tad) % PNG_ADLER;
        for (uint32_t w = 0; w < PNG_BLOCK / 64; ++w) bsum += wbs[w];
        bsum %= PNG_ADLER;
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t adler = (uint32_t)((bsum << 16) | asum);
        PngImgInfo ii;
        ii.adler = adler;
        ii.last_crc = png_crc_append_be32(si[a.nseg - 1].crc, adler);
        a.imginfo[img] = ii;
        a.nbytes[img] = at + 12;
        if (a.out) {
            uint8_t* o = a.out + (size_t)img * a.capacity;
            uint8_t head[33], tail[12];
            png_file_head(a, head);
            png_file_tail(tail);
            for (uint32_t i = 0; i < 33; ++i)
                if (i < a.capacity) o[i] = head[i];
            for (uint32_t i = 0; i < 12; ++i)
                if (at + i < a.capacity) o[at + i] = tail[i];
        }
    }
}

// chunk s of image i to its place: length, "IDAT", data (and the Adler-32 after the last
// segment's), CRC.  A byte at or past the capacity is not written.
__global__ void __launch_bounds__(PNG_BLOCK) k_png_scatter(PngArgs a)
{
    const uint32_t tid = threadIdx.x, seg = blockIdx.x, img = blockIdx.y;
    const size_t k = (size_t)img * a.nseg + seg;
    const PngSegInfo v = a.seginfo[k];
    const bool last = seg + 1 == a.nseg;
    const uint64_t at = a.offs[k], cap = a.capacity;
    uint8_t* o = a.out + (size_t)img * cap;
    const uint8_t* slot = a.slots + k * PNG_SLOT;
    const uint32_t ndata = v.nbytes + (last ? 4u : 0u);
    if (tid < 8u) {
        const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
        const uint8_t b = tid < 4u ? (uint8_t)(ndata >> (24 - 8 * tid)) : idat[tid - 4u];
        if (at + tid < cap) o[at + tid] = b;
    } else if (tid < 16u) {
        const uint32_t j = tid - 8u;  // 0..3 the Adler-32 (last chunk), 4..7 the CRC
        const PngImgInfo ii = a.imginfo[img];
        if (j < 4u) {
            if (last && at + 8 + v.nbytes + j < cap) o[at + 8 + v.nbytes + j] = (uint8_t)(ii.adler >> (24 - 8 * j));
        } else {
            const uint32_t crc = last ? ii.last_crc : v.crc;
            const uint64_t p = at + 8 + ndata + (j - 4u);
            if (p < cap) o[p] = (uint8_t)(crc >> (24 - 8 * (j - 4u)));
        }
    }
    for (uint32_t i = tid; i < v.nbytes; i += PNG_BLOCK)
        if (at + 8 + i < cap) o[at + 8 + i] = slot[i];
}

#endif  // __HIPCC__

}  // namespace smk
