// sm_cloud.hpp — the tail of every script of the reference: mask a disparity
// map by a range, take points[mask] and colors[mask] (disparity_calculation.py:302-320,
// disparity_test.py:230-265, try_try.py:90-96, mapTo3D_mc_cnn.py:124 ff.) and write the rows
// '%f %f %f %d %d %d ' of io_functions.write_ply (io_functions.py:28-44).
//
// Extraction: per pixel the mask lo < d < hi (strict; either bound may be absent; a NaN never
// passes a bound), the surviving pixels reprojected by reproject_point (sm_reproject.hpp: the
// arithmetic of k_reproject itself) and written compacted in row-major order with their colours
// swapped BGR -> RGB.
// Formatting: ply_row below, one function for the host and the device, integers only.
//
// Both stages have rows of data-dependent position, so both are count -> scan -> write in plain
// launches: a per-block total (k_cloud_count: passing pixels, k_ply_len: bytes), one exclusive
// scan of the totals in a single workgroup (k_scan_totals, 64-bit sums), and a pass that
// recomputes its block's ranks and writes (k_cloud_scatter, k_ply_write_lds).  No launch waits for
// another workgroup.  Inside a block the mask ranks are a wave64 ballot + popcount and the byte
// offsets a wave scan, both joined across the four waves through LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_reproject.hpp"

namespace smk {

// ---------------------------------------------------------------------------------------------
// The row formatter.  '%f' of a float32 x (Python formats the double of the same value, which
// is exact): |x| = m * 2^e with m < 2^24.
//   e >= 0   x is an integer: m << e (below 2^64 for e <= 40, else 128 bits in 32-bit limbs,
//            divided by 10^9 limb by limb), then ".000000".
//   e < 0    k = -e.  The integer part is m >> k; the six decimals are q = (f * 10^6) >> k of the
//            fraction bits f, rounded to nearest, ties to even, on the remainder against
//            1 << (k - 1); f * 10^6 < 2^44.  q = 10^6 carries into the integer part.  For
//            k >= 45 the value is below half a unit of the sixth decimal: 0.000000.
// The sign is printed for every negative bit pattern (-0.000000 for -0 and underflow) except
// NaN ("nan", never signed); infinities are "inf" / "-inf".
// WRITE = false only measures.  Longest token 47 bytes, longest row 3 * 48 + 3 * 4 + 1 = 157.
#define SM_HD __host__ __device__ inline

constexpr int PLY_MAX_ROW = 157;

SM_HD int ply_digits_u32(uint32_t v)
{
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6
         : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}

// nd decimal digits of v, zero-padded on the left, at out[0 .. nd)
SM_HD void ply_put_digits_u32(uint32_t v, int nd, char* out)
{
    for (int i = nd - 1; i >= 0; --i) {
        const uint32_t q = v / 10u;
        out[i] = (char)('0' + (v - q * 10u));
        v = q;
    }
}

// decimal of v < 2^64 without padding; returns its length
template <bool WRITE>
SM_HD int ply_put_u64(uint64_t v, char* out)
{
    if (v < 4294967296ull) {
        const int nd = ply_digits_u32((uint32_t)v);
        if (WRITE) ply_put_digits_u32((uint32_t)v, nd, out);
        return nd;
    }
    // 10 .. 20 digits: the low nine by one 64-bit division, the rest again below 2^64 / 10^9 < 2^35
    const uint64_t hi = v / 1000000000ull;
    const uint32_t lo = (uint32_t)(v - hi * 1000000000ull);
    int nd;
    if (hi < 4294967296ull) {
        nd = ply_digits_u32((uint32_t)hi);
        if (WRITE) ply_put_digits_u32((uint32_t)hi, nd, out);
    } else {
        const uint64_t hh = hi / 1000000000ull;  // < 2^5
        const uint32_t hl = (uint32_t)(hi - hh * 1000000000ull);
        nd = ply_digits_u32((uint32_t)hh);
        if (WRITE) {
            ply_put_digits_u32((uint32_t)hh, nd, out);
            ply_put_digits_u32(hl, 9, out + nd);
        }
        nd += 9;
    }
    if (WRITE) ply_put_digits_u32(lo, 9, out + nd);
    return nd + 9;
}

// decimal of m << e for 40 < e <= 104 (m < 2^24): 128 bits in four 32-bit limbs, the nine-digit
// groups taken off by dividing by 10^9 limb by limb (every step a 64-by-32-bit division whose
// quotient fits 32 bits).  At least 2^64 > 10^19: three to five groups.
template <bool WRITE>
SM_HD int ply_put_big(uint32_t m, int e, char* out)
{
    uint32_t l0 = 0, l1 = 0, l2 = 0, l3 = 0;
    {
        const int w = e >> 5, b = e & 31;
        const uint64_t v = (uint64_t)m << b;  // < 2^55
        const uint32_t a = (uint32_t)v, c = (uint32_t)(v >> 32);
        if (w == 1) l1 = a, l2 = c;
        else if (w == 2) l2 = a, l3 = c;
        else l3 = a;  // w == 3: b <= 8 (e <= 104), so c == 0
    }
    uint32_t g[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        uint64_t cur = l3;
        l3 = (uint32_t)(cur / 1000000000u), cur = ((cur % 1000000000u) << 32) | l2;
        l2 = (uint32_t)(cur / 1000000000u), cur = ((cur % 1000000000u) << 32) | l1;
        l1 = (uint32_t)(cur / 1000000000u), cur = ((cur % 1000000000u) << 32) | l0;
        l0 = (uint32_t)(cur / 1000000000u);
        g[j] = (uint32_t)(cur % 1000000000u);
    }
    const int top = g[4] ? 4 : g[3] ? 3 : 2;
    const uint32_t gt = top == 4 ? g[4] : top == 3 ? g[3] : g[2];
    const int nt = ply_digits_u32(gt);
    if (WRITE) {
        ply_put_digits_u32(gt, nt, out);
        int pos = nt;
#pragma unroll
        for (int j = 3; j >= 0; --j)
            if (j < top) {
                ply_put_digits_u32(g[j], 9, out + pos);
                pos += 9;
            }
    }
    return nt + 9 * top;
}

// '%f' of the float32 with these bits; returns the token's length
template <bool WRITE>
SM_HD int ply_put_f32(uint32_t bits, char* out)
{
    const uint32_t ex = (bits >> 23) & 0xFFu, fr = bits & 0x7FFFFFu;
    const bool neg = (bits >> 31) != 0;
    if (ex == 255u) {
        if (fr) {
            if (WRITE) out[0] = 'n', out[1] = 'a', out[2] = 'n';
            return 3;
        }
        if (WRITE) {
            if (neg) *out++ = '-';
            out[0] = 'i', out[1] = 'n', out[2] = 'f';
        }
        return 3 + (neg ? 1 : 0);
    }
    int n = 0;
    if (neg) {
        if (WRITE) out[0] = '-';
        n = 1;
    }
    const uint32_t m = ex ? (fr | 0x800000u) : fr;
    const int e = ex ? (int)ex - 150 : -149;
    uint32_t q = 0;
    if (e > 40) {
        n += ply_put_big<WRITE>(m, e, out + n);
    } else if (e >= 0) {
        n += ply_put_u64<WRITE>((uint64_t)m << e, out + n);
    } else {
        const int k = -e;
        uint32_t ip = 0;
        if (k < 45) {
            ip = k < 24 ? m >> k : 0u;
            const uint64_t mask = (1ull << k) - 1ull;
            const uint64_t p = ((uint64_t)m & mask) * 1000000ull;  // < 2^44
            const uint64_t r = p & mask, h = 1ull << (k - 1);
            q = (uint32_t)(p >> k);
            if (r > h || (r == h && (q & 1u))) ++q;
            if (q == 1000000u) q = 0, ++ip;
        }
        const int nd = ply_digits_u32(ip);
        if (WRITE) ply_put_digits_u32(ip, nd, out + n);
        n += nd;
    }
    if (WRITE) {
        out[n] = '.';
        ply_put_digits_u32(q, 6, out + n + 1);
    }
    return n + 7;
}

// one row '%f %f %f %d %d %d ' + '\n'; returns its length (at most PLY_MAX_ROW)
template <bool WRITE>
SM_HD int ply_row(const float* v, const uint8_t* c, char* out)
{
    int n = 0;
    for (int j = 0; j < 3; ++j) {
        uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
        bits = __float_as_uint(v[j]);
#else
        __builtin_memcpy(&bits, v + j, 4);
#endif
        n += ply_put_f32<WRITE>(bits, out + n);
        if (WRITE) out[n] = ' ';
        ++n;
    }
    for (int j = 0; j < 3; ++j) {
        const uint32_t cv = c[j];
        const int nd = cv < 10u ? 1 : cv < 100u ? 2 : 3;
        if (WRITE) {
            ply_put_digits_u32(cv, nd, out + n);
            out[n + nd] = ' ';
        }
        n += nd + 1;
    }
    if (WRITE) out[n] = '\n';
    return n + 1;
}

// ---------------------------------------------------------------------------------------------
constexpr int CLOUD_BLOCK = 256;  // pixels (extraction) or rows (formatting) per workgroup
constexpr int SCAN_BLOCK = 1024;  // block totals one step of k_scan_totals takes

// exclusive 64-bit scan of n 32-bit block totals in ONE workgroup, SCAN_BLOCK totals a step with
// the running sum carried from step to step: offs[0 .. n), the grand total in offs[n] and, when
// given, in *total_out
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_totals(const uint32_t* tot, uint64_t* offs, size_t n,
                                                            uint64_t* total_out)
{
    __shared__ unsigned long long wsum[SCAN_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (size_t base = 0; base < n; base += SCAN_BLOCK) {
        const size_t i = base + tid;
        const unsigned long long v = i < n ? tot[i] : 0u;
        unsigned long long s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(s, o);
            if (lane >= o) s += t;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
            const unsigned long long x = wsum[w];
            if (w < wave) before += x;
            all += x;
        }
        if (i < n) offs[i] = carry + before + s - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        offs[n] = carry;
        if (total_out) *total_out = carry;
    }
}

// per-image counts from the scanned offsets: counts[j] = offs[(j + 1) * seg] - offs[j * seg]
__global__ void k_seg_counts(const uint64_t* offs, int64_t* counts, int nseg, size_t seg)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j < nseg) counts[j] = (int64_t)(offs[(size_t)(j + 1) * seg] - offs[(size_t)j * seg]);
}

struct CloudArgs {
    const void* disp;      // [img][H][W] int16 or float32
    const uint8_t* bgr;    // [img] H rows of bgr_stride bytes, 3 bytes a pixel
    size_t bgr_img_stride;  // bytes between images
    double Q[16];
    double lo, hi;         // the bounds (float32 maps: already rounded to float32)
    const float* lo_dev;   // lo = "min": [img] the maps' own minima, instead of lo
    const float* min_disp;  // [img] (handle_missing)
    uint32_t* tot;         // [img][bpi] passing pixels of every block (k_cloud_count)
    const uint64_t* offs;  // their exclusive scan (k_cloud_scatter)
    float* verts;          // [rows][3]
    uint8_t* colors;       // [rows][3] RGB
    uint64_t cap_rows;     // rows verts / colors hold: a row at or past it is not written
    int H, W, bgr_stride, bpi;
    int has_lo, has_hi, handle_missing, zero_nonfinite;
};

// the block's pixel of this thread: whether it passes the mask, and its disparity
template <typename T>
__device__ inline bool cloud_pass(const CloudArgs& a, size_t npx, size_t p, int img, float& dv)
{
    if (p >= npx) return false;
    dv = disp_value(reinterpret_cast<const T*>(a.disp), (size_t)img * npx + p);
    // in float64 both kinds of map compare exactly: an int16 against the bound itself, a
    // float32 against the bound the host rounded to float32.  A NaN fails either comparison.
    const double d = (double)dv;
    bool ok = true;
    if (a.lo_dev) ok = d > (double)a.lo_dev[img];
    else if (a.has_lo) ok = d > a.lo;
    if (a.has_hi) ok = ok && d < a.hi;
    return ok;
}

template <typename T>
__global__ void __launch_bounds__(CLOUD_BLOCK) k_cloud_count(CloudArgs a)
{
    __shared__ uint32_t wcnt[CLOUD_BLOCK / 64];
    const int tid = threadIdx.x, img = blockIdx.y;
    const size_t npx = (size_t)a.H * a.W;
    float dv;
    const bool pass = cloud_pass<T>(a, npx, (size_t)blockIdx.x * CLOUD_BLOCK + tid, img, dv);
    const unsigned long long bal = __ballot(pass);
    if ((tid & 63) == 0) wcnt[tid >> 6] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (tid == 0) a.tot[(size_t)img * a.bpi + blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

template <typename T>
__global__ void __launch_bounds__(CLOUD_BLOCK) k_cloud_scatter(CloudArgs a)
{
    __shared__ uint32_t wcnt[CLOUD_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y;
    const size_t npx = (size_t)a.H * a.W;
    const size_t p = (size_t)blockIdx.x * CLOUD_BLOCK + tid;
    float dv = 0.f;
    const bool pass = cloud_pass<T>(a, npx, p, img, dv);
    const unsigned long long bal = __ballot(pass);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!pass) return;
    uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += wcnt[w];
    const uint64_t row = a.offs[(size_t)img * a.bpi + blockIdx.x] + rank;
    if (row >= a.cap_rows) return;
    const int y = (int)(p / (size_t)a.W), x = (int)(p - (size_t)y * a.W);
    float o[3];
    reproject_point(a.Q, x, y, (double)dv, a.handle_missing, a.handle_missing ? (double)a.min_disp[img] : 0.0, o);
    if (a.zero_nonfinite) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if ((__float_as_uint(o[j]) & 0x7F800000u) == 0x7F800000u) o[j] = 0.f;  // NaN or +-inf
    }
    float* v = a.verts + 3 * row;
    v[0] = o[0], v[1] = o[1], v[2] = o[2];
    const uint8_t* s = a.bgr + (size_t)img * a.bgr_img_stride + (size_t)y * a.bgr_stride + 3 * (size_t)x;
    uint8_t* c = a.colors + 3 * row;
    c[0] = s[2], c[1] = s[1], c[2] = s[0];
}

struct PlyArgs {
    const float* verts;     // [n][3]
    const uint8_t* colors;  // [n][3]
    const uint64_t* n_dev;  // the row count when only the device knows it (then n is its cap)
    uint64_t n;
    uint32_t* tot;          // [blocks] bytes of every block (k_ply_len)
    const uint64_t* offs;   // their exclusive scan (k_ply_write)
    char* out;
    uint64_t cap_bytes;     // bytes out holds: a row that would end past it is not written
};

__device__ inline uint64_t ply_rows(const PlyArgs& a)
{
    if (!a.n_dev) return a.n;
    const uint64_t n = *a.n_dev;
    return n < a.n ? n : a.n;
}

// bytes of this thread's row and their inclusive sum over the block (LDS: one word per wave)
__device__ inline uint32_t ply_block_scan(uint32_t len, uint32_t* wsum, uint32_t& total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t s = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(s, o);
        if (lane >= o) s += t;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < CLOUD_BLOCK / 64; ++w) {
        const uint32_t x = wsum[w];
        if (w < wave) s += x;
        total += x;
    }
    return s;
}

__global__ void __launch_bounds__(CLOUD_BLOCK) k_ply_len(PlyArgs a)
{
    __shared__ uint32_t wsum[CLOUD_BLOCK / 64];
    const uint64_t n = ply_rows(a), r = (uint64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    const uint32_t len = r < n ? (uint32_t)ply_row<false>(a.verts + 3 * r, a.colors + 3 * r, nullptr) : 0u;
    uint32_t total;
    ply_block_scan(len, wsum, total);
    if (threadIdx.x == 0) a.tot[blockIdx.x] = total;
}

__global__ void __launch_bounds__(CLOUD_BLOCK) k_ply_write(PlyArgs a)
{
    __shared__ uint32_t wsum[CLOUD_BLOCK / 64];
    const uint64_t n = ply_rows(a), r = (uint64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    const float* v = a.verts + 3 * r;
    const uint8_t* c = a.colors + 3 * r;
    const uint32_t len = r < n ? (uint32_t)ply_row<false>(v, c, nullptr) : 0u;
    uint32_t total;
    const uint32_t incl = ply_block_scan(len, wsum, total);
    if (r >= n) return;
    const uint64_t at = a.offs[blockIdx.x] + (incl - len);
    if (at + len > a.cap_bytes) return;
    ply_row<true>(v, c, a.out + at);
}

// the same rows staged in LDS and streamed out in 16-byte stores: the default write pass (the whole
// formatter measured 1.4 to 2.7 times as fast as with k_ply_write, DESIGN.md §4.9;
// SM_TUNE_PLY_STAGE -1 selects k_ply_write).  A block's rows are contiguous in the output; the text is
// laid into LDS at the output address's offset within 16 bytes, so aligned 16-byte pieces of LDS
// are aligned 16-byte pieces of the output.  A block that does not fit the capacity whole writes
// row by row like k_ply_write.
constexpr int PLY_LDS_BYTES = CLOUD_BLOCK * PLY_MAX_ROW + 16;

__global__ void __launch_bounds__(CLOUD_BLOCK) k_ply_write_lds(PlyArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char ply_lds[];
    __shared__ uint32_t wsum[CLOUD_BLOCK / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = ply_rows(a), r = (uint64_t)blockIdx.x * CLOUD_BLOCK + tid;
    const float* v = a.verts + 3 * r;
    const uint8_t* c = a.colors + 3 * r;
    const uint32_t len = r < n ? (uint32_t)ply_row<false>(v, c, nullptr) : 0u;
    uint32_t total;
    const uint32_t incl = ply_block_scan(len, wsum, total);
    const uint64_t base = a.offs[blockIdx.x];
    if (base + total > a.cap_bytes) {  // block-uniform
        if (r < n && base + incl <= a.cap_bytes) ply_row<true>(v, c, a.out + base + (incl - len));
        return;
    }
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(a.out + base) & 15u);
    if (r < n) ply_row<true>(v, c, ply_lds + sh + (incl - len));
    __syncthreads();
    char* g = a.out + base - sh;  // 16-byte aligned; LDS byte q belongs at g[q], q in [sh, end)
    const uint32_t end = sh + total, b0 = (sh + 15u) & ~15u, b1 = end & ~15u;
    if (b1 <= b0) {  // fewer than 31 bytes
        if (tid < total) g[sh + tid] = ply_lds[sh + tid];
        return;
    }
    if (tid >= sh && tid < b0) g[tid] = ply_lds[tid];
    for (uint32_t q = b0 + tid * 16u; q < b1; q += CLOUD_BLOCK * 16u)
        *reinterpret_cast<uint4*>(g + q) = *reinterpret_cast<const uint4*>(ply_lds + q);
    if (tid < end - b1) g[b1 + tid] = ply_lds[b1 + tid];
}

}  // namespace smk
