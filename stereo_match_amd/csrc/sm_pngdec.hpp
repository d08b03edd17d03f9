// sm_pngdec.hpp — PNG input: what the reference's scripts take from cv2.imread
// (disparity_test.py:79-80, mapTo3D.py:78-79, mapTo3D_mc_cnn.py:70-77) and the KITTI 16-bit
// disparity maps, decoded on the device: chunk walk, CRC-32, inflate, Adler-32, scanline
// unfilter and pixel conversion.
//
// Supported: non-interlaced files of colour type 0 (depth 8 or 16), 2 (depth 8) and 6 (depth 8,
// alpha dropped), filtered stream (rowbytes + 1) * H < 2^31 as in the encoder.  Ancillary chunks
// are skipped; every chunk up to IEND has its CRC checked.
//
// Every function that decides an output byte or a verdict is __host__ __device__ (SM_HD) and runs
// on both sides: pngdec_host below calls in loops what the kernels call, and gives the same
// pixels, the same status and the same inflate path.
//
// Launches (plain, on the ctx stream, ordered by the kernel boundaries alone; no workgroup waits
// for another one, nothing spins):
//   k_pngdec_parse           a wave per file: the bounded chunk walk (pd_parse), tables of all
//                            chunks and of the IDAT chunks, IHDR against the stated geometry
//   k_pngdec_crc             a workgroup per chunk: slices joined by x^(8 n) mod P (sm_png.hpp)
//   k_pngdec_inflate         a wave per IDAT chunk, speculative: the chunk is taken to begin at a
//                            block boundary and is inflated into PNGDEC_CAP bytes of LDS
//   k_pngdec_place           per image: are all chunks good, do the lengths sum to the stream, does
//                            the combined Adler-32 equal the trailer -> path, slot offsets
//   k_pngdec_compact         a workgroup per chunk: its slot to its place in the stream
//   k_pngdec_gather          (images not accepted) the IDAT data concatenated
//   k_pngdec_inflate_serial  (images not accepted) a wave per image, the same block decoder with
//                            the global stream buffer as sink and window
//   k_pngdec_adler, k_pngdec_verify   (serial path) Adler-32 in 32 KiB pieces, combined, compared
//   k_pngdec_unfilter        a workgroup per row group of an image (cut at rows of type None or
//                            Sub): skewed wavefront over blocks of 64 rows
//
// The chunk-parallel path is exact.  A chunk is GOOD when, inflated from its first bit as if that
// were a block boundary with nothing before it, (1) the last bit consumed lies in its last byte,
// (2) its last block is the final one (BFINAL) in the last chunk and in no other, or it ends
// exactly on the chunk's last byte boundary, (3) no match distance reaches before the chunk's own
// first output byte, (4) its output fits PNGDEC_CAP.  Claim: if every chunk is good the
// concatenated outputs are what a serial inflater makes of the concatenated data.  Induction over
// the chunks: the serial inflater begins chunk 0 behind the zlib header at a block boundary with
// an empty window, as the speculative one does.  If it enters chunk k byte-aligned at a block
// boundary, it reads the very bits the speculative decoder read; no code of a block depends on
// earlier blocks, and by (3) no copy reads a byte from before the chunk, so both produce the same
// bytes and, by (1) and (2), the serial inflater is byte-aligned at a block boundary at the first
// byte of chunk k + 1 (or has met BFINAL in the last chunk, in front of the four Adler bytes).
// The sum of the lengths must be the stream's length and the Adler-32 combined from the chunks'
// partial sums must equal the trailer; anything else hands the image to the serial path, which
// gives the verdict for every valid or invalid zlib stream.
// The parallel path is tried only when nidat <= 2 * ceil(stream_len / PNGDEC_CAP) + 4, so that its
// scratch (nidat slots of PNGDEC_CAP bytes) stays within about twice the stream plus four slots; a
// file cut into thousands of tiny IDAT chunks goes straight to the serial path.
//
// Inside a wave the symbol loop runs redundantly on all 64 lanes (wave-uniform control flow, the
// tables in LDS written by lane 0); a match or a stored block is copied by the whole wave.  An
// overlapping copy (distance < length) reads out[pos - dist + i % dist], which is the byte-serial
// result.
#pragma once
#include "sm_png.hpp"

namespace smk {

constexpr uint32_t PNGDEC_CAP = 32768;  // bytes of output an IDAT chunk may make on the parallel path
constexpr int PNGDEC_BLOCK = 256;
constexpr int PNGDEC_TILE = 64;         // steps of the unfilter wavefront per LDS tile

// sm_pngdec_params.out_kind
constexpr int PD_OUT_U8 = 0, PD_OUT_U16 = 1, PD_OUT_DISP_I16 = 2, PD_OUT_DISP_F32 = 3;
constexpr uint32_t PD_PATH_NONE = 0, PD_PATH_PARALLEL = 1, PD_PATH_SERIAL = 2;

// per-image status
enum : int {
    PD_OK = 0,
    PD_E_SIG,
    PD_E_TRUNC,
    PD_E_LIMIT,
    PD_E_IHDR,
    PD_E_GEOM,
    PD_E_INTERLACE,
    PD_E_PALETTE,
    PD_E_DEPTH,
    PD_E_COLOR16,
    PD_E_GRAYALPHA,
    PD_E_SIZE,
    PD_E_NOIDAT,
    PD_E_CRC,
    PD_E_ZHDR,
    PD_E_EOF,
    PD_E_BTYPE,
    PD_E_STORED,
    PD_E_CODES,
    PD_E_SYM,
    PD_E_DIST,
    PD_E_LONG,
    PD_E_SHORT,
    PD_E_ADLER,
    PD_E_FILTER,
    PD_N
};

inline const char* pngdec_message(int code)
{
    static const char* const msg[PD_N] = {
        "ok",
        "not a PNG file (bad signature)",
        "truncated file (a chunk runs past the end, or IEND is missing)",
        "more chunks or bytes than max_chunks / max_file_bytes allow",
        "IHDR is missing, misplaced or malformed",
        "IHDR differs from the stated geometry (width, height, channels or depth)",
        "unsupported: interlace method 1 (Adam7)",
        "unsupported: palette (colour type 3)",
        "unsupported: bit depth 1, 2 or 4",
        "unsupported: 16-bit colour",
        "unsupported: gray + alpha (colour type 4)",
        "unsupported: an empty image or a filtered stream of 2^31 bytes and more",
        "no IDAT chunk",
        "CRC mismatch in a chunk",
        "bad zlib header (CM, window, FCHECK or FDICT)",
        "the deflate data ends inside a block or before the Adler-32",
        "deflate block type 3",
        "stored block: LEN / NLEN mismatch",
        "over-subscribed or incomplete set of code lengths",
        "invalid literal/length or distance symbol",
        "match distance beyond the start of the stream",
        "the inflated stream is longer than (rowbytes + 1) * H",
        "the inflated stream is shorter than (rowbytes + 1) * H",
        "Adler-32 mismatch",
        "filter type above 4",
    };
    return code >= 0 && code < PD_N ? msg[code] : "unknown status";
}

struct PdHdr {
    uint32_t W, H;
    int depth, channels;  // channels of the file: 1, 3 or 4 (with alpha)
};

struct PdImg {
    uint32_t status, path, nchunks, nidat;
    uint32_t try_par, adler_want, pad0, pad1;
    uint64_t zlen;  // bytes of all IDAT data
};

struct PdChunk {
    uint32_t off, len;  // offset of the type field in the file; bytes of data
};

struct PdIdat {
    uint32_t off, len;  // offset and bytes of the data
    uint64_t zoff;      // bytes of IDAT data before it
    uint64_t ooff;      // parallel path: bytes of the stream before its output
};

struct PdChunkInfo {
    uint32_t out_len, good;
    uint32_t a, b;  // Adler partial as PngSegInfo: sum of the bytes, sum of (len - i) * byte[i], mod 65521
};

struct PdArgs {
    const uint8_t* files;  // file i at files + offsets[i], sizes[i] bytes
    const uint64_t* offsets;
    const uint64_t* sizes;
    int nimg, H, W;
    int file_ch, depth, bpp;  // the stated geometry of the files
    uint32_t rowbytes, nseg;  // nseg: 32 KiB pieces of the stream (Adler pass)
    uint64_t stream_len, stream_stride;
    int kind, out_ch, keep, inv_i16;  // output
    float inv_f32;
    uint8_t* out;
    size_t img_stride, row_stride;
    uint32_t max_chunks, maxpar;  // table rows per image; chunks up to which the parallel path is tried
    uint64_t max_file, zstride;
    PdImg* img;          // [img]
    PdChunk* chunks;     // [img][max_chunks]
    PdIdat* idat;        // [img][max_chunks]
    PdChunkInfo* cinfo;  // [img][maxpar]
    uint8_t* slots;      // [img][maxpar][PNGDEC_CAP]
    uint8_t* zbuf;       // [img][zstride]
    uint8_t* stream;     // [img][stream_stride]
    PdChunkInfo* seg;    // [img][nseg]
    uint32_t* carry;     // [img][ceil(H / 64)][W] per row group the last row of a block of 64 rows, packed pixels
};

SM_HD uint32_t pd_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// the 13 bytes of IHDR
SM_HD int pd_ihdr(const uint8_t* d, PdHdr& h)
{
    h.W = pd_be32(d), h.H = pd_be32(d + 4), h.depth = d[8], h.channels = 0;
    const int ctype = d[9];
    if (d[10] != 0 || d[11] != 0 || d[12] > 1) return PD_E_IHDR;
    if (d[12] == 1) return PD_E_INTERLACE;
    const int dp = h.depth;
    if (ctype == 3) return (dp == 1 || dp == 2 || dp == 4 || dp == 8) ? PD_E_PALETTE : PD_E_IHDR;
    if (ctype == 0) {
        if (dp == 1 || dp == 2 || dp == 4) return PD_E_DEPTH;
        if (dp != 8 && dp != 16) return PD_E_IHDR;
        h.channels = 1;
    } else if (ctype == 2 || ctype == 6) {
        if (dp == 16) return PD_E_COLOR16;
        if (dp != 8) return PD_E_IHDR;
        h.channels = ctype == 2 ? 3 : 4;
    } else if (ctype == 4) {
        return (dp == 8 || dp == 16) ? PD_E_GRAYALPHA : PD_E_IHDR;
    } else {
        return PD_E_IHDR;
    }
    if (h.W < 1 || h.W > 0x7FFFFFFFu || h.H < 1 || h.H > 0x7FFFFFFFu) return PD_E_SIZE;
    if (((uint64_t)h.W * h.channels * (dp / 8) + 1) * h.H >= (1ull << 31)) return PD_E_SIZE;
    return PD_OK;
}

// The chunk walk of one file: every length is checked against the file before it is used, at most
// max_chunks chunks.  chunks / idat: this image's rows of the tables.
SM_HD int pd_parse(const PdArgs& a, const uint8_t* f, uint64_t n, PdChunk* chunks, PdIdat* idat, PdImg& im)
{
    im.nchunks = im.nidat = 0, im.zlen = 0, im.try_par = 0, im.path = PD_PATH_NONE, im.adler_want = 0;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8) return PD_E_SIG;
    for (int i = 0; i < 8; ++i)
        if (f[i] != sig[i]) return PD_E_SIG;
    if (n > a.max_file || n > 0xFFFFFFFFull) return PD_E_LIMIT;
    uint64_t pos = 8;
    uint32_t nc = 0, ni = 0;
    uint64_t z = 0;
    for (;;) {
        if (pos == n) return PD_E_TRUNC;  // no IEND
        if (n - pos < 12) return PD_E_TRUNC;
        const uint32_t len = pd_be32(f + pos);
        if ((uint64_t)len > n - pos - 12) return PD_E_TRUNC;
        if (nc >= a.max_chunks) return PD_E_LIMIT;
        const uint8_t* t = f + pos + 4;
        const uint32_t typ = pd_be32(t);
        chunks[nc].off = (uint32_t)(pos + 4), chunks[nc].len = len;
        if (nc == 0) {
            if (typ != 0x49484452u || len != 13) return PD_E_IHDR;
            PdHdr h;
            const int rc = pd_ihdr(t + 4, h);
            if (rc != PD_OK) return rc;
            if (h.W != (uint32_t)a.W || h.H != (uint32_t)a.H || h.channels != a.file_ch || h.depth != a.depth) return PD_E_GEOM;
        } else if (typ == 0x49484452u) {
            return PD_E_IHDR;
        }
        ++nc;
        if (typ == 0x49444154u) {  // IDAT
            idat[ni].off = (uint32_t)(pos + 8), idat[ni].len = len, idat[ni].zoff = z, idat[ni].ooff = 0;
            ++ni, z += len;
        }
        pos += 12ull + len;
        if (typ == 0x49454E44u) break;  // IEND: what follows is not looked at
    }
    im.nchunks = nc, im.nidat = ni, im.zlen = z;
    if (ni == 0) return PD_E_NOIDAT;
    im.try_par = ni <= a.maxpar ? 1u : 0u;
    return PD_OK;
}

// ---------------------------------------------------------------------------------------------
// inflate
#if defined(__HIP_DEVICE_COMPILE__)
#define PD_SYNC() __syncthreads()
// Lane 0 writes LDS (a literal, a code length) that all lanes of the same wave read back later
// without a workgroup barrier.  What is relied on: the decoding workgroup is one wave, a wave's
// LDS operations complete in issue order, and this wavefront-scope fence keeps the compiler from
// moving the read above the write (it costs no instruction).
#define PD_WAVE_FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
#else
#define PD_SYNC() ((void)0)
#define PD_WAVE_FENCE() ((void)0)
#endif

// LSB-first bit reader over p[0 .. n): never reads at or past n; bits past the end read as zeros
// and cannot be dropped.  The next eight bytes are loaded two refills ahead (nxt0, nxt1), so that
// the latency of a global load is spent under the symbols decoded meanwhile.
struct PdBits {
    const uint8_t* p;
    uint64_t n, pos;  // pos: next byte to fetch
    uint64_t acc;
    uint32_t cnt;               // valid bits in acc
    uint32_t nxt0, nn0, nxt1, nn1;  // nn0 + nn1 <= 8 bytes fetched ahead; nn1 > 0 only behind nn0 == 4

    SM_HD void prime()
    {
        nxt0 = nxt1, nn0 = nn1;
        const uint64_t left = n - pos;
        nn1 = left < 4 ? (uint32_t)left : 4u;
        nxt1 = 0;
        for (uint32_t k = 0; k < 4u; ++k)
            if (k < nn1) nxt1 |= (uint32_t)p[pos + k] << (8u * k);
        pos += nn1;
    }
    SM_HD void start(const uint8_t* p_, uint64_t n_)
    {
        p = p_, n = n_, pos = 0, acc = 0, cnt = 0, nxt1 = 0, nn1 = 0;
        prime();
        prime();
    }
    SM_HD void fill()
    {
        while (cnt <= 32u && nn0) {
            acc |= (uint64_t)nxt0 << cnt;
            cnt += 8u * nn0;
            prime();
        }
    }
    SM_HD uint32_t peek(uint32_t k) const { return (uint32_t)acc & ((1u << k) - 1u); }  // k <= 16
    SM_HD bool drop(uint32_t k)
    {
        if (k > cnt) return false;
        acc >>= k, cnt -= k;
        return true;
    }
    // fill, read k <= 16 bits
    SM_HD bool get(uint32_t k, uint32_t& v)
    {
        fill();
        v = peek(k);
        return drop(k);
    }
    SM_HD uint64_t byte_pos() const { return pos - nn0 - nn1 - (cnt >> 3); }  // the byte behind the last bit consumed
    SM_HD bool at_end() const { return cnt == 0u && nn0 == 0u && nn1 == 0u && pos == n; }
    // on a byte boundary (cnt a multiple of 8): skip `skip` bytes from there
    SM_HD void seek_from_byte(uint64_t skip)
    {
        pos = byte_pos() + skip, acc = 0, cnt = 0, nxt1 = 0, nn1 = 0;
        prime();
        prime();
    }
};

// the output: out[0 .. cap), `lane` of `nl` lanes (1 on the CPU).  GLOBAL: out is global memory
// written and read back by different lanes of the wave, so a copy begins behind a fence.
template <bool GLOBAL>
struct PdSink {
    uint8_t* out;
    uint64_t pos, cap;
    uint32_t lane, nl;

    SM_HD int lit(uint32_t b)
    {
        if (pos >= cap) return PD_E_LONG;
        if (lane == 0) out[pos] = (uint8_t)b;
        ++pos;
        return PD_OK;
    }
    SM_HD int raw(const uint8_t* src, uint32_t len)
    {
        if (len > cap - pos) return PD_E_LONG;
        for (uint32_t i = lane; i < len; i += nl) out[pos + i] = src[i];
        pos += len;
        return PD_OK;
    }
    SM_HD int match(uint32_t len, uint32_t dist)
    {
        if (dist > pos) return PD_E_DIST;
        if (len > cap - pos) return PD_E_LONG;
#if defined(__HIP_DEVICE_COMPILE__)
        if (GLOBAL) __threadfence_block();
#endif
        PD_WAVE_FENCE();
        const uint8_t* src = out + (pos - dist);
        if (dist >= len) {
            for (uint32_t i = lane; i < len; i += nl) out[pos + i] = src[i];
        } else {
            for (uint32_t i = lane; i < len; i += nl) out[pos + i] = src[i % dist];
        }
#if defined(__HIP_DEVICE_COMPILE__)
        if (GLOBAL) __threadfence_block();
#endif
        pos += len;
        return PD_OK;
    }
};

// a canonical code: symbols per length and the symbols in code order (RFC 1951 §3.2.2)
constexpr uint32_t PD_FAST = 10;  // codes of up to PD_FAST bits decode by one table read
struct PdHuff {
    uint16_t count[16];
    uint16_t offs[16];
    uint16_t sym[288];
    uint16_t fast[1u << PD_FAST];  // by the next PD_FAST bits: symbol << 4 | length, 0: a longer code (or none)
};

struct PdWork {
    PdHuff lit, dist;
    uint8_t lens[320];
};

// The code of n lengths.  Returns -1 for an over-subscribed set, else what is left of the code
// space (0: complete); maxl: the longest length.  Lane 0 of nl writes count and sym, all lanes
// the table `fast`.
SM_HD int pd_build(PdHuff& h, const uint8_t* len, int n, uint32_t lane, uint32_t nl, int& maxl)
{
    const bool wr = lane == 0;
    PD_SYNC();
    if (wr) {
        for (int l = 0; l < 16; ++l) h.count[l] = 0;
        for (int s = 0; s < n; ++s) h.count[len[s] & 15] = (uint16_t)(h.count[len[s] & 15] + 1);
    }
    PD_SYNC();
    int left = 1, total = 0;
    maxl = 0;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= (int)h.count[l];
        if (left < 0) return -1;
        if (h.count[l]) maxl = l;
        total += h.count[l];
    }
    if (wr) {
        h.offs[1] = 0;
        for (int l = 1; l < 15; ++l) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
        for (int s = 0; s < n; ++s) {
            const int l = len[s] & 15;
            if (l) {
                h.sym[h.offs[l]] = (uint16_t)s;
                h.offs[l] = (uint16_t)(h.offs[l] + 1);
            }
        }
    }
    for (uint32_t k = lane; k < (1u << PD_FAST); k += nl) h.fast[k] = 0;
    PD_SYNC();
    // entry i of sym: its length l and canonical code, from the counts
    for (uint32_t i = lane; i < (uint32_t)total; i += nl) {
        uint32_t l = 1, startl = 0, first = 0;
        while (i >= startl + h.count[l]) {  // i < total: ends at l <= 15
            startl += h.count[l];
            first = (first + h.count[l]) << 1;
            ++l;
        }
        if (l <= PD_FAST) {
            const uint32_t code = first + (i - startl), r = png_bitrev32(code) >> (32u - l);
            const uint16_t e = (uint16_t)((uint32_t)h.sym[i] << 4 | l);
            for (uint32_t k = r; k < (1u << PD_FAST); k += 1u << l) h.fast[k] = e;
        }
    }
    PD_SYNC();
    return left;
}

// one symbol, or -status
SM_HD int pd_decode(PdBits& br, const PdHuff& h)
{
    br.fill();
    const uint32_t e = h.fast[(uint32_t)br.acc & ((1u << PD_FAST) - 1u)];
    if (e) {
        if (!br.drop(e & 15u)) return -PD_E_EOF;
        return (int)(e >> 4);
    }
    uint32_t bits = (uint32_t)br.acc;
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int cnt = h.count[len];
        if (code - cnt < first) {
            if (!br.drop(len)) return -PD_E_EOF;
            return h.sym[index + (code - first)];
        }
        index += cnt, first += cnt;
        first <<= 1, code <<= 1;
    }
    return br.cnt < 15u ? -PD_E_EOF : -PD_E_SYM;
}

// the symbols of one block up to its end-of-block code
template <bool G>
SM_HD int pd_codes(PdBits& br, PdSink<G>& o, const PdHuff& lit, const PdHuff& dist)
{
    for (;;) {  // every turn drops at least one bit
        const int s = pd_decode(br, lit);
        if (s < 0) return -s;
        if (s < 256) {
            const int rc = o.lit((uint32_t)s);
            if (rc) return rc;
            continue;
        }
        if (s == 256) return PD_OK;
        if (s > 285) return PD_E_SYM;
        uint32_t len, ev;
        if (s < 265) {
            len = (uint32_t)s - 254u;
        } else if (s == 285) {
            len = 258u;
        } else {
            const uint32_t k = (uint32_t)s - 257u, e = (k >> 2) - 1u;
            if (!br.get(e, ev)) return PD_E_EOF;
            len = 3u + ((4u + (k & 3u)) << e) + ev;
        }
        const int d = pd_decode(br, dist);
        if (d < 0) return -d;
        if (d > 29) return PD_E_SYM;
        uint32_t dd;
        if (d < 4) {
            dd = (uint32_t)d + 1u;
        } else {
            const uint32_t e = ((uint32_t)d >> 1) - 1u;
            if (!br.get(e, ev)) return PD_E_EOF;
            dd = 1u + ((2u + ((uint32_t)d & 1u)) << e) + ev;
        }
        const int rc = o.match(len, dd);
        if (rc) return rc;
    }
}

// the code lengths of a dynamic block into w.lit / w.dist, by zlib's rules: an incomplete set is
// accepted only when it is a single code of length 1 (or, for distances, no code at all)
SM_HD int pd_dynamic(PdBits& br, PdWork& w, uint32_t lane, uint32_t nl)
{
    const bool wr = lane == 0;
    const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v;
    if (!br.get(14, v)) return PD_E_EOF;
    const int nlen = (int)(v & 31u) + 257, ndist = (int)((v >> 5) & 31u) + 1, ncode = (int)(v >> 10) + 4;
    if (nlen > 286 || ndist > 30) return PD_E_CODES;
    PD_SYNC();
    if (wr)
        for (int i = 0; i < 19; ++i) w.lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!br.get(3, v)) return PD_E_EOF;
        if (wr) w.lens[ord[i]] = (uint8_t)v;
    }
    int maxl;
    int left = pd_build(w.lit, w.lens, 19, lane, nl, maxl);
    if (left != 0) return PD_E_CODES;
    const int total = nlen + ndist;
    for (int i = 0; i < total;) {  // every turn drops at least one bit
        const int s = pd_decode(br, w.lit);
        if (s < 0) return s == -PD_E_SYM ? PD_E_CODES : -s;
        if (s < 16) {
            if (wr) w.lens[i] = (uint8_t)s;
            ++i;
            continue;
        }
        uint32_t prev = 0, rep;
        if (s == 16) {
            if (i == 0) return PD_E_CODES;
            PD_WAVE_FENCE();
            prev = w.lens[i - 1];
            if (!br.get(2, v)) return PD_E_EOF;
            rep = 3u + v;
        } else if (s == 17) {
            if (!br.get(3, v)) return PD_E_EOF;
            rep = 3u + v;
        } else {
            if (!br.get(7, v)) return PD_E_EOF;
            rep = 11u + v;
        }
        if (i + (int)rep > total) return PD_E_CODES;
        if (wr)
            for (uint32_t k = 0; k < rep; ++k) w.lens[i + (int)k] = (uint8_t)prev;
        i += (int)rep;
    }
    PD_SYNC();
    if (w.lens[256] == 0) return PD_E_CODES;
    // the code-length code lived in w.lit: both codes are built from the lengths now
    left = pd_build(w.dist, w.lens + nlen, ndist, lane, nl, maxl);
    if (left < 0 || (left > 0 && maxl > 1)) return PD_E_CODES;
    left = pd_build(w.lit, w.lens, nlen, lane, nl, maxl);
    if (left < 0 || (left > 0 && maxl != 1)) return PD_E_CODES;
    return PD_OK;
}

SM_HD void pd_fixed(PdWork& w, uint32_t lane, uint32_t nl)
{
    const bool wr = lane == 0;
    PD_SYNC();
    if (wr) {
        for (int s = 0; s < 288; ++s) w.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        for (int s = 0; s < 30; ++s) w.lens[288 + s] = 5;
    }
    int maxl;
    pd_build(w.lit, w.lens, 288, lane, nl, maxl);
    pd_build(w.dist, w.lens + 288, 30, lane, nl, maxl);
}

// Blocks from br into o until the final block (final_seen) or, with chunk_mode, until a block
// ends exactly behind the last byte of the input.
template <bool G>
SM_HD int pd_inflate(PdBits& br, PdSink<G>& o, PdWork& w, bool chunk_mode, bool& final_seen)
{
    final_seen = false;
    for (;;) {  // every turn drops at least three bits
        if (chunk_mode && br.at_end()) return PD_OK;
        uint32_t v;
        if (!br.get(3, v)) return PD_E_EOF;
        const bool last = (v & 1u) != 0;
        const uint32_t type = v >> 1;
        int rc;
        if (type == 0u) {
            br.drop(br.cnt & 7u);
            if (!br.get(16, v)) return PD_E_EOF;
            uint32_t nv;
            if (!br.get(16, nv)) return PD_E_EOF;
            if ((v ^ nv) != 0xFFFFu) return PD_E_STORED;
            const uint64_t at = br.byte_pos();  // whole bytes are buffered: the data begins there
            if ((uint64_t)v > br.n - at) return PD_E_EOF;
            rc = o.raw(br.p + at, v);
            br.seek_from_byte(v);
        } else if (type == 1u) {
            pd_fixed(w, o.lane, o.nl);
            rc = pd_codes(br, o, w.lit, w.dist);
        } else if (type == 2u) {
            rc = pd_dynamic(br, w, o.lane, o.nl);
            if (rc == PD_OK) rc = pd_codes(br, o, w.lit, w.dist);
        } else {
            rc = PD_E_BTYPE;
        }
        if (rc) return rc;
        if (last) {
            final_seen = true;
            return PD_OK;
        }
    }
}

// CM = 8, window <= 32 KiB, FCHECK, no FDICT
SM_HD bool pd_zlib_header_ok(uint32_t cmf, uint32_t flg)
{
    return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && ((cmf << 8) | flg) % 31u == 0u && !(flg & 32u);
}

// IDAT chunk k of nidat on its own into `o` (PNGDEC_CAP bytes): its output length and whether it
// is good (the header comment)
template <bool G>
SM_HD void pd_chunk(const uint8_t* data, uint32_t len, uint32_t k, uint32_t nidat, PdSink<G>& o, PdWork& w, PdChunkInfo& ci)
{
    const bool first = k == 0, lastc = k + 1 == nidat;
    ci.out_len = 0, ci.good = 0, ci.a = ci.b = 0;
    const uint32_t d0 = first ? 2u : 0u, tail = lastc ? 4u : 0u;
    if (len < d0 + tail) return;
    if (first && !pd_zlib_header_ok(data[0], data[1])) return;
    PdBits br;
    br.start(data + d0, len - d0 - tail);
    bool fin;
    const int rc = pd_inflate(br, o, w, true, fin);
    ci.out_len = (uint32_t)o.pos;
    if (rc != PD_OK) return;
    ci.good = fin ? (lastc && br.byte_pos() == br.n ? 1u : 0u) : (lastc ? 0u : 1u);
}

// the verdict over an image's chunks; sets im.path and the chunks' places in the stream
SM_HD void pd_place(const PdArgs& a, const uint8_t* f, PdImg& im, PdIdat* idat, const PdChunkInfo* ci)
{
    im.path = PD_PATH_SERIAL;
    if (!im.try_par) return;
    uint64_t sum = 0, asum = 1, bsum = 0;
    for (uint32_t k = 0; k < im.nidat; ++k) {
        if (!ci[k].good) return;
        idat[k].ooff = sum;
        bsum = (bsum + ci[k].b + (uint64_t)ci[k].out_len * asum) % PNG_ADLER;
        asum = (asum + ci[k].a) % PNG_ADLER;
        sum += ci[k].out_len;
    }
    if (sum != a.stream_len) return;
    const PdIdat& l = idat[im.nidat - 1];  // good: at least four bytes
    if (pd_be32(f + l.off + l.len - 4u) != (uint32_t)((bsum << 16) | asum)) return;
    im.path = PD_PATH_PARALLEL;
}

// the whole zlib stream z[0 .. n) into o (the stream buffer); im.adler_want from the trailer
template <bool G>
SM_HD int pd_serial(const uint8_t* z, uint64_t n, PdSink<G>& o, PdWork& w, PdImg& im)
{
    if (n < 2) return PD_E_EOF;
    if (!pd_zlib_header_ok(z[0], z[1])) return PD_E_ZHDR;
    PdBits br;
    br.start(z + 2, n - 2);
    bool fin;
    const int rc = pd_inflate(br, o, w, false, fin);
    if (rc) return rc;
    if (o.pos != o.cap) return PD_E_SHORT;
    const uint64_t at = br.byte_pos();
    if (br.n - at < 4) return PD_E_EOF;
    im.adler_want = pd_be32(br.p + at);
    return PD_OK;
}

// ---------------------------------------------------------------------------------------------
// unfilter and conversion.  A pixel is bpp <= 4 bytes packed in 32 bits, byte k at bits 8k.
SM_HD uint32_t pd_unfilt(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c, int bpp)
{
    if (type == 0) return x;
    uint32_t r = 0;
    for (int k = 0; k < bpp; ++k) {
        const int sh = 8 * k;
        const uint32_t xa = (a >> sh) & 255u, xb = (b >> sh) & 255u, xc = (c >> sh) & 255u;
        uint32_t pred;
        if (type == 1) pred = xa;
        else if (type == 2) pred = xb;
        else if (type == 3) pred = (xa + xb) >> 1;
        else {
            const int p = (int)xa + (int)xb - (int)xc;
            int pa = p - (int)xa, pb = p - (int)xb, pc = p - (int)xc;
            pa = pa < 0 ? -pa : pa, pb = pb < 0 ? -pb : pb, pc = pc < 0 ? -pc : pc;
            pred = (pa <= pb && pa <= pc) ? xa : (pb <= pc ? xb : xc);
        }
        r |= ((((x >> sh) & 255u) + pred) & 255u) << sh;
    }
    return r;
}

// the gray of rectify's bgr2gray (sm_rectify.hpp)
SM_HD uint32_t pd_gray(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

// pixel x of an output row
SM_HD void pd_store(const PdArgs& s, uint32_t px, uint8_t* row, uint32_t x)
{
    const uint32_t b0 = px & 255u, b1 = (px >> 8) & 255u, b2 = (px >> 16) & 255u;
    switch (s.kind) {
    case PD_OUT_U8:
        if (s.out_ch == 3) {
            uint8_t* o = row + 3u * (size_t)x;
            if (s.file_ch == 1) o[0] = o[1] = o[2] = (uint8_t)b0;  // a 16-bit sample >> 8 is its first byte
            else if (s.keep) o[0] = (uint8_t)b0, o[1] = (uint8_t)b1, o[2] = (uint8_t)b2;
            else o[0] = (uint8_t)b2, o[1] = (uint8_t)b1, o[2] = (uint8_t)b0;
        } else {
            row[x] = (uint8_t)(s.file_ch == 1 ? b0 : pd_gray(b2, b1, b0));
        }
        break;
    case PD_OUT_U16:
        reinterpret_cast<uint16_t*>(row)[x] = (uint16_t)(b0 << 8 | b1);
        break;
    case PD_OUT_DISP_I16: {
        const uint32_t v = b0 << 8 | b1;
        reinterpret_cast<int16_t*>(row)[x] = (int16_t)(v ? (int)(v >> 4) : s.inv_i16);
        break;
    }
    default: {
        const uint32_t v = b0 << 8 | b1;
        reinterpret_cast<float*>(row)[x] = v ? (float)v / 256.f : s.inv_f32;
    }
    }
}

// ---------------------------------------------------------------------------------------------
// the CPU twin: one file (a.nimg == 1, every pointer of `a` on the host, a.files the file with
// a.offsets[0] == 0); returns the status, path: the inflate path taken
inline int pngdec_host(PdArgs a, uint32_t& path)
{
    path = PD_PATH_NONE;
    const uint8_t* f = a.files;
    const uint64_t n = a.sizes[0];
    a.max_chunks = (uint32_t)(n / 12 + 1), a.max_file = n;
    std::vector<PdChunk> chunks(a.max_chunks);
    std::vector<PdIdat> idat(a.max_chunks);
    PdImg im{};
    int rc = pd_parse(a, f, n, chunks.data(), idat.data(), im);
    if (rc) return rc;
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = png_crc_table_entry(i);
    for (uint32_t c = 0; c < im.nchunks; ++c) {
        uint32_t reg = 0xFFFFFFFFu;
        const uint8_t* p = f + chunks[c].off;
        const uint64_t m = 4ull + chunks[c].len;
        for (uint64_t i = 0; i < m; ++i) reg = (reg >> 8) ^ table[(reg ^ p[i]) & 255u];
        if (~reg != pd_be32(p + m)) return PD_E_CRC;
    }
    std::vector<uint8_t> stream(a.stream_len);
    std::vector<PdWork> work(1);
    if (im.try_par) {
        std::vector<PdChunkInfo> ci(im.nidat);
        std::vector<uint8_t> slots((size_t)im.nidat * PNGDEC_CAP);
        for (uint32_t k = 0; k < im.nidat; ++k) {
            PdSink<false> o{slots.data() + (size_t)k * PNGDEC_CAP, 0, PNGDEC_CAP, 0, 1};
            pd_chunk(f + idat[k].off, idat[k].len, k, im.nidat, o, work[0], ci[k]);
            uint64_t sa = 0, sb = 0;
            for (uint32_t i = 0; i < ci[k].out_len; ++i) sa += o.out[i], sb += (uint64_t)(ci[k].out_len - i) * o.out[i];
            ci[k].a = (uint32_t)(sa % PNG_ADLER), ci[k].b = (uint32_t)(sb % PNG_ADLER);
        }
        pd_place(a, f, im, idat.data(), ci.data());
        if (im.path == PD_PATH_PARALLEL)
            for (uint32_t k = 0; k < im.nidat; ++k)
                std::memcpy(stream.data() + idat[k].ooff, slots.data() + (size_t)k * PNGDEC_CAP, ci[k].out_len);
    } else {
        im.path = PD_PATH_SERIAL;
    }
    path = im.path;
    if (im.path == PD_PATH_SERIAL) {
        std::vector<uint8_t> z(im.zlen);
        for (uint32_t k = 0; k < im.nidat; ++k) std::memcpy(z.data() + idat[k].zoff, f + idat[k].off, idat[k].len);
        PdSink<false> o{stream.data(), 0, a.stream_len, 0, 1};
        rc = pd_serial(z.data(), z.size(), o, work[0], im);
        if (rc) return rc;
        uint64_t asum = 1, bsum = 0;
        for (uint64_t s0 = 0; s0 < a.stream_len; s0 += PNG_SEG) {
            const uint64_t len = std::min<uint64_t>(PNG_SEG, a.stream_len - s0);
            uint64_t sa = 0, sb = 0;
            for (uint64_t i = 0; i < len; ++i) sa += stream[s0 + i], sb += (len - i) * stream[s0 + i];
            bsum = (bsum + sb % PNG_ADLER + len * asum) % PNG_ADLER;
            asum = (asum + sa) % PNG_ADLER;
        }
        if ((uint32_t)((bsum << 16) | asum) != im.adler_want) return PD_E_ADLER;
    }
    const uint32_t rb = a.rowbytes, npx = (uint32_t)a.W;
    std::vector<uint32_t> rows(2 * (size_t)npx, 0u);
    uint32_t* up = rows.data();
    uint32_t* cur = up + npx;
    for (int y = 0; y < a.H; ++y) {
        const uint8_t* s = stream.data() + (size_t)y * (rb + 1u);
        const int type = s[0];
        if (type > 4) return PD_E_FILTER;
        uint8_t* orow = a.out + (size_t)y * a.row_stride;
        for (uint32_t x = 0; x < npx; ++x) {
            uint32_t v = 0;
            for (int k = 0; k < a.bpp; ++k) v |= (uint32_t)s[1u + x * (uint32_t)a.bpp + (uint32_t)k] << (8 * k);
            cur[x] = pd_unfilt(type, v, x ? cur[x - 1] : 0u, up[x], x ? up[x - 1] : 0u, a.bpp);
        }
        for (uint32_t x = 0; x < npx; ++x) pd_store(a, cur[x], orow, x);
        std::swap(cur, up);
    }
    return PD_OK;
}

// ---------------------------------------------------------------------------------------------
// kernels
#if defined(__HIPCC__)

__global__ void __launch_bounds__(64) k_pngdec_parse(PdArgs a)
{
    const uint32_t img = blockIdx.x;
    if (threadIdx.x != 0) return;
    PdImg im{};
    const int rc = pd_parse(a, a.files + a.offsets[img], a.sizes[img], a.chunks + (size_t)img * a.max_chunks,
                            a.idat + (size_t)img * a.max_chunks, im);
    im.status = (uint32_t)rc;
    if (rc) im.nchunks = im.nidat = 0, im.try_par = 0;
    a.img[img] = im;
}

// chunks blockIdx.x, blockIdx.x + gridDim.x, ... of image blockIdx.y: CRC-32 of type + data
// against the four bytes behind them
__global__ void __launch_bounds__(PNGDEC_BLOCK) k_pngdec_crc(PdArgs a)
{
    __shared__ uint32_t table[256];
    __shared__ uint32_t wc[PNGDEC_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, img = blockIdx.y;
    table[tid & 255u] = png_crc_table_entry(tid & 255u);
    __syncthreads();
    const uint32_t nc = a.img[img].nchunks;
    const uint8_t* f = a.files + a.offsets[img];
    for (uint32_t c = blockIdx.x; c < nc; c += gridDim.x) {  // workgroup-uniform
        const PdChunk ch = a.chunks[(size_t)img * a.max_chunks + c];
        const uint8_t* p = f + ch.off;
        const uint32_t m = ch.len + 4u;  // < 2^32: the file is smaller
        const uint32_t per = (m + PNGDEC_BLOCK - 1) / PNGDEC_BLOCK;
        const uint32_t b0 = (uint64_t)tid * per < m ? tid * per : m, b1 = m - b0 > per ? b0 + per : m;
        uint32_t reg = 0xFFFFFFFFu;  // every slice a finished CRC of its own, joined as in k_png_deflate
        for (uint32_t i = b0; i < b1; ++i) reg = (reg >> 8) ^ table[(reg ^ p[i]) & 255u];
        uint32_t part = 0;
        if (b1 > b0) part = png_crc_mul(png_crc_shift(m - b1), ~reg);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part ^= __shfl_xor(part, o);
        __syncthreads();
        if (lane == 0) wc[wave] = part;
        __syncthreads();
        if (tid == 0) {
            uint32_t crc = 0;
            for (uint32_t w = 0; w < PNGDEC_BLOCK / 64; ++w) crc ^= wc[w];
            if (crc != pd_be32(p + m)) a.img[img].status = PD_E_CRC;
        }
    }
}

struct PdInflateLds {
    alignas(16) uint8_t out[PNGDEC_CAP];
    PdWork w;
};

__global__ void __launch_bounds__(64) k_pngdec_inflate(PdArgs a)
{
    __shared__ PdInflateLds S;
    const uint32_t lane = threadIdx.x, k = blockIdx.x, img = blockIdx.y;
    const PdImg im = a.img[img];
    if (im.status || !im.try_par || k >= im.nidat) return;  // workgroup-uniform
    const PdIdat d = a.idat[(size_t)img * a.max_chunks + k];
    PdSink<false> o{S.out, 0, PNGDEC_CAP, lane, 64};
    PdChunkInfo ci;
    pd_chunk(a.files + a.offsets[img] + d.off, d.len, k, im.nidat, o, S.w, ci);
    __syncthreads();
    const uint32_t n = ci.out_len;
    uint64_t sa = 0, sb = 0;
    for (uint32_t i = lane; i < n; i += 64) sa += S.out[i], sb += (uint64_t)(n - i) * S.out[i];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) sa += __shfl_xor(sa, s), sb += __shfl_xor(sb, s);
    ci.a = (uint32_t)(sa % PNG_ADLER), ci.b = (uint32_t)(sb % PNG_ADLER);
    uint32_t* slot = reinterpret_cast<uint32_t*>(a.slots + ((size_t)img * a.maxpar + k) * PNGDEC_CAP);
    for (uint32_t wi = lane; wi < (n + 3u) / 4u; wi += 64) slot[wi] = reinterpret_cast<const uint32_t*>(S.out)[wi];
    if (lane == 0) a.cinfo[(size_t)img * a.maxpar + k] = ci;
}

__global__ void __launch_bounds__(64) k_pngdec_place(PdArgs a)
{
    const uint32_t img = blockIdx.x;
    if (threadIdx.x != 0) return;
    PdImg im = a.img[img];
    if (im.status) return;
    pd_place(a, a.files + a.offsets[img], im, a.idat + (size_t)img * a.max_chunks, a.cinfo + (size_t)img * a.maxpar);
    a.img[img] = im;
}

__global__ void __launch_bounds__(PNGDEC_BLOCK) k_pngdec_compact(PdArgs a)
{
    const uint32_t tid = threadIdx.x, k = blockIdx.x, img = blockIdx.y;
    const PdImg im = a.img[img];
    if (im.status || im.path != PD_PATH_PARALLEL || k >= im.nidat) return;
    const uint32_t n = a.cinfo[(size_t)img * a.maxpar + k].out_len;
    const uint8_t* slot = a.slots + ((size_t)img * a.maxpar + k) * PNGDEC_CAP;
    uint8_t* dst = a.stream + (size_t)img * a.stream_stride + a.idat[(size_t)img * a.max_chunks + k].ooff;
    for (uint32_t i = tid; i < n; i += PNGDEC_BLOCK) dst[i] = slot[i];  // the sum of the lengths is the stream's
}

__global__ void __launch_bounds__(PNGDEC_BLOCK) k_pngdec_gather(PdArgs a)
{
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    const PdImg im = a.img[img];
    if (im.status || im.path != PD_PATH_SERIAL) return;
    const uint8_t* f = a.files + a.offsets[img];
    uint8_t* z = a.zbuf + (size_t)img * a.zstride;  // zlen <= the file's size <= max_file <= zstride
    for (uint32_t k = blockIdx.x; k < im.nidat; k += gridDim.x) {
        const PdIdat d = a.idat[(size_t)img * a.max_chunks + k];
        for (uint32_t i = tid; i < d.len; i += PNGDEC_BLOCK) z[d.zoff + i] = f[d.off + i];
    }
}

__global__ void __launch_bounds__(64) k_pngdec_inflate_serial(PdArgs a)
{
    __shared__ PdWork w;
    const uint32_t lane = threadIdx.x, img = blockIdx.x;
    PdImg im = a.img[img];
    if (im.status || im.path != PD_PATH_SERIAL) return;
    PdSink<true> o{a.stream + (size_t)img * a.stream_stride, 0, a.stream_len, lane, 64};
    const int rc = pd_serial(a.zbuf + (size_t)img * a.zstride, im.zlen, o, w, im);
    if (lane == 0) {
        a.img[img].adler_want = im.adler_want;
        if (rc) a.img[img].status = (uint32_t)rc;
    }
}

// the Adler partials of 32 KiB piece blockIdx.x of the stream (serial path)
__global__ void __launch_bounds__(PNGDEC_BLOCK) k_pngdec_adler(PdArgs a)
{
    __shared__ unsigned long long wa[PNGDEC_BLOCK / 64], wb[PNGDEC_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, seg = blockIdx.x, img = blockIdx.y;
    const PdImg im = a.img[img];
    if (im.status || im.path != PD_PATH_SERIAL) return;
    const uint64_t s0 = (uint64_t)seg * PNG_SEG;
    const uint32_t n = (uint32_t)(a.stream_len - s0 < PNG_SEG ? a.stream_len - s0 : PNG_SEG);
    const uint8_t* p = a.stream + (size_t)img * a.stream_stride + s0;
    unsigned long long sa = 0, sb = 0;
    for (uint32_t i = tid; i < n; i += PNGDEC_BLOCK) sa += p[i], sb += (unsigned long long)(n - i) * p[i];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) sa += __shfl_xor(sa, s), sb += __shfl_xor(sb, s);
    if (lane == 0) wa[wave] = sa, wb[wave] = sb;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < PNGDEC_BLOCK / 64; ++w) sa += wa[w], sb += wb[w];
        PdChunkInfo ci;
        ci.out_len = n, ci.good = 1, ci.a = (uint32_t)(sa % PNG_ADLER), ci.b = (uint32_t)(sb % PNG_ADLER);
        a.seg[(size_t)img * a.nseg + seg] = ci;
    }
}

__global__ void __launch_bounds__(64) k_pngdec_verify(PdArgs a)
{
    const uint32_t img = blockIdx.x;
    if (threadIdx.x != 0) return;
    const PdImg im = a.img[img];
    if (im.status || im.path != PD_PATH_SERIAL) return;
    uint64_t asum = 1, bsum = 0;
    for (uint32_t s = 0; s < a.nseg; ++s) {
        const PdChunkInfo ci = a.seg[(size_t)img * a.nseg + s];
        bsum = (bsum + ci.b + (uint64_t)ci.out_len * asum) % PNG_ADLER;
        asum = (asum + ci.a) % PNG_ADLER;
    }
    if ((uint32_t)((bsum << 16) | asum) != im.adler_want) a.img[img].status = PD_E_ADLER;
}

// Rows of type None or Sub do not depend on the row above, so the image is cut into row groups
// that run on different workgroups: group g = blockIdx.x begins at the first such row at or after
// row 64 g (group 0 at row 0) and ends where the next non-empty group begins; a group without such
// a row is empty and its rows stay with the group before.  The cut changes no byte: the first row
// of a group never reads the row above it.
// Inside a group, blocks of 64 rows one after the other.  Wave 0 runs the skewed wavefront: lane l
// owns row y0 + l and makes pixel x = t - l at step t; b and c (the pixels above and above left)
// come from lane l - 1, which made them one and two steps earlier; a stays in a register.  Lane 0
// takes b and c from the last row of the block before (a.carry, a row per group).  The steps go
// through LDS in tiles of PNGDEC_TILE: all threads load the tile's filtered pixels (row r: pixels
// T0 - r ...), wave 0 computes, all threads convert and store.
__device__ inline int pd_group_start(const uint8_t* stream, size_t pitch, int H, int from, int* shared_first)
{
    // the first row >= from of type 0 or 1, or H; workgroup-uniform
    const int tid = threadIdx.x;
    if (from <= 0) return 0;
    for (int base = from; base < H; base += PNGDEC_BLOCK) {
        __syncthreads();
        if (tid == 0) *shared_first = H;
        __syncthreads();
        const int y = base + tid;
        if (y < H && stream[(size_t)y * pitch] <= 1) atomicMin(shared_first, y);
        __syncthreads();
        const int f = *shared_first;
        if (f < H) return f;
    }
    return H;
}

__global__ void __launch_bounds__(PNGDEC_BLOCK) k_pngdec_unfilter(PdArgs a)
{
    __shared__ uint32_t tin[64][PNGDEC_TILE + 1], tout[64][PNGDEC_TILE + 1];
    __shared__ uint32_t prevrow[PNGDEC_TILE + 1];  // pixels T0 - 1 .. T0 + TILE - 1 of the row above the block
    __shared__ int types[64];
    __shared__ int first_row;
    __shared__ uint32_t status0;
    const int tid = threadIdx.x, img = blockIdx.y, grp = blockIdx.x;
    // other workgroups of this launch may set the status (a filter type above 4) at any time: one
    // thread reads it, so that the whole workgroup takes the same branch
    if (tid == 0) status0 = a.img[img].status;
    __syncthreads();
    if (status0) return;
    const uint8_t* stream = a.stream + (size_t)img * a.stream_stride;
    uint8_t* out = a.out + (size_t)img * a.img_stride;
    uint32_t* carry = a.carry + ((size_t)img * gridDim.x + grp) * a.W;
    const int W = a.W, bpp = a.bpp;
    const size_t pitch = (size_t)a.rowbytes + 1u;
    const int ybeg = pd_group_start(stream, pitch, a.H, 64 * grp, &first_row);
    if (ybeg >= a.H || ybeg >= 64 * (grp + 1)) return;  // empty: no independent row among this group's 64
    int yend = a.H;
    for (int g = grp + 1; 64 * g < a.H; ++g) {  // the next non-empty group
        const int s = pd_group_start(stream, pitch, a.H, 64 * g, &first_row);
        if (s < 64 * (g + 1) || s >= a.H) {
            yend = s;
            break;
        }
    }
    for (int y0 = ybeg; y0 < yend; y0 += 64) {
        const int rows = yend - y0 < 64 ? yend - y0 : 64;
        __syncthreads();
        if (tid < 64) {
            int t = tid < rows ? stream[(size_t)(y0 + tid) * pitch] : 0;
            if (t > 4) a.img[img].status = PD_E_FILTER, t = 0;
            types[tid] = t;
        }
        uint32_t o1 = 0, o2 = 0;  // wave 0: this lane's pixels of one and two steps ago
        const int nsteps = W + rows - 1;
        for (int T0 = 0; T0 < nsteps; T0 += PNGDEC_TILE) {
            for (int e = tid; e < 64 * PNGDEC_TILE; e += PNGDEC_BLOCK) {
                const int r = e / PNGDEC_TILE, j = e % PNGDEC_TILE, x = T0 + j - r;
                uint32_t v = 0;
                if (r < rows && x >= 0 && x < W) {
                    const uint8_t* p = stream + (size_t)(y0 + r) * pitch + 1u + (size_t)x * bpp;
                    for (int k = 0; k < bpp; ++k) v |= (uint32_t)p[k] << (8 * k);
                }
                tin[r][j] = v;
            }
            if (tid <= PNGDEC_TILE) {
                const int x = T0 + tid - 1;
                prevrow[tid] = (y0 > ybeg && x >= 0 && x < W) ? carry[x] : 0u;
            }
            __syncthreads();
            if (tid < 64) {
                const int type = types[tid];
                for (int j = 0; j < PNGDEC_TILE; ++j) {
                    const int x = T0 + j - tid;
                    uint32_t bb = __shfl_up(o1, 1), cc = __shfl_up(o2, 1);
                    if (tid == 0) bb = prevrow[j + 1], cc = prevrow[j];
                    const uint32_t aa = x > 0 ? o1 : 0u;
                    if (x <= 0) cc = 0u;
                    uint32_t r = pd_unfilt(type, tin[tid][j], aa, bb, cc, bpp);
                    if (x < 0 || x >= W) r = 0u;
                    tout[tid][j] = r;
                    o2 = o1, o1 = r;
                }
            }
            __syncthreads();
            for (int e = tid; e < 64 * PNGDEC_TILE; e += PNGDEC_BLOCK) {
                const int r = e / PNGDEC_TILE, j = e % PNGDEC_TILE, x = T0 + j - r;
                if (r < rows && x >= 0 && x < W) {
                    const uint32_t v = tout[r][j];
                    pd_store(a, v, out + (size_t)(y0 + r) * a.row_stride, (uint32_t)x);
                    if (r == 63) carry[x] = v;
                }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(PNGDEC_BLOCK) k_pngdec_status(PdArgs a, int* status)
{
    const int img = blockIdx.x * PNGDEC_BLOCK + threadIdx.x;
    if (img < a.nimg) status[img] = (int)a.img[img].status;
}

#endif  // __HIPCC__

}  // namespace smk
