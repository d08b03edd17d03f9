// sm_nlm.hpp — cv2.fastNlMeansDenoising on uint8 gray images: the one
// OpenCV call of the reference's test flow (disparity_test.py:94-95) in front of the matcher.
// Semantics (a version-scoped restatement of FastNlMeansDenoisingInvoker, NORM_L2, CV_8UC1,
// int accumulators; tests/nlm_np.py is the independent one):
//   th = tws / 2, t = 2 th + 1;  sh = sws / 2, s = 2 sh + 1;  b = th + sh
//   E = the source extended by b on every side, BORDER_REFLECT_101
//   per pixel p, for each of the s*s offsets o:
//     dist = sum over the t*t template q of (E[p+q] - E[p+o+q])^2
//     wgt  = tab[dist >> shift]          (the host's table, nlm_weight_table in sm_api.hip)
//     est += wgt * E[p+o];  wsum += wgt
//   out = (est + wsum / 2) / wsum        (uint32, truncating)
// Kernel: one 512-thread workgroup owns a 64 x 64 tile of output pixels and stages the tile
// plus its b-pixel halo of E in LDS once, the reflection resolved there (so an image smaller
// than b, whose indices reflect several times, is nothing special).  Each of the four 32 x 32
// quadrants has two waves, which share the search rows (dy) between them and add their exact
// integer sums through LDS at the end: a one-frame launch is 240 workgroups, and eight waves
// each put two waves on every SIMD instead of one.  Each lane owns 4 adjacent columns x 4 rows.
// For a fixed offset the squared-difference image is shared by every pixel of the tile and
// dist is its t x t box sum, so the 4 + 2 th
// squared differences of a row segment give the lane's 4 row sums by a sliding sum, and the
// 4 + 2 th row sums of a column its 4 box sums: (4 + 2 th)^2 squared differences for 16
// pixels (6.25 per pixel at t = 7) instead of t^2 = 49.  The lane's own rows of E (the first
// operand of every difference, the same for all offsets) stay in registers; the shifted rows
// come from LDS as aligned dwords, brought to the lane's byte alignment by v_alignbyte_b32
// with a wave-uniform shift.  One barrier after the staging, two around the final sum; no
// atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace smk {

constexpr int NLM_TILE = 64;           // output pixels per workgroup and axis
constexpr int NLM_THREADS = 512;       // 4 quadrants x 2 halves of the search rows
constexpr int NLM_SUM_BYTES = 32 * 256 * 4;  // LDS of the final sum: est + wsum of 16 pixels per lane, 256 lanes
constexpr int NLM_MAX_TH = 4;          // templateWindowSize <= 9
constexpr int NLM_MAX_SH = 17;         // searchWindowSize <= 35
constexpr int NLM_LDS_TAB_MAX = 8192;  // weight-table prefix entries staged in LDS (32 KiB); longer: global reads

struct NlmArgs {
    const uint8_t* src;  // [img] H rows of src_stride bytes
    uint8_t* dst;        // [img][H][W]
    const int32_t* tab;  // the non-zero prefix of the weight table: ntab entries
    size_t img_stride;   // bytes between source images
    int H, W, src_stride;
    int sh;              // search half width
    int shift, ntab;
    int pitch;           // LDS bytes per tile row (nlm_pitch)
};

// dwords a lane reads to cover its 4 + 2 th bytes at any byte alignment
constexpr int nlm_nd(int th) { return (2 * th + 10) / 4; }

// LDS row pitch in bytes: covers the tile row (64 + 2 b) and the aligned dwords the rightmost
// lane reads at the largest offset; = 8 mod 32, so the 4 lane rows of a 32-lane group (4 tile
// rows = pitch dwords apart) fall on disjoint groups of 8 banks
inline int nlm_pitch(int th, int sh)
{
    const int need = std::max(NLM_TILE + 2 * (th + sh), 4 * (15 + (2 * sh) / 4 + nlm_nd(th)));
    return (need - 8 + 31) / 32 * 32 + 8;
}

// tile + table prefix; the final sum reuses the same bytes once every wave is done with them
inline size_t nlm_lds_bytes(int th, int sh, int ntab_lds)
{
    return std::max((size_t)(NLM_TILE + 2 * (th + sh)) * nlm_pitch(th, sh) + (size_t)ntab_lds * 4,
                    (size_t)NLM_SUM_BYTES);
}

// BORDER_REFLECT_101 of index i into [0, n): period 2 (n - 1), as often as needed
__device__ inline int nlm_reflect(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

__device__ inline int nlm_byte(const uint32_t* v, int k) { return (int)((v[k >> 2] >> (8 * (k & 3))) & 255u); }

template <int TH, bool LDSTAB>
__global__ void __launch_bounds__(NLM_THREADS, 4) k_nlm_u8(NlmArgs a)  // 4 waves per SIMD: two workgroups per CU
{
    extern __shared__ uint32_t nlm_lds[];
    constexpr int T2 = 2 * TH;
    constexpr int NB = 4 + T2;         // bytes of a row segment: 4 columns + the template's reach
    constexpr int NR = 4 + T2;         // row segments per lane: 4 rows + the template's reach
    constexpr int NDA = (NB + 3) / 4;  // dwords of an aligned row segment
    constexpr int ND = nlm_nd(TH);     // dwords read for one (NDA < ND)
    const int sh = a.sh, b = TH + sh;
    const int rows = NLM_TILE + 2 * b, width = rows, pw = a.pitch >> 2;
    const int tid = threadIdx.x;

    // ---- stage E[tile + halo], reflection resolved; the pad bytes of a row read 0
    {
        const int gx0 = blockIdx.x * NLM_TILE - b, gy0 = blockIdx.y * NLM_TILE - b;
        const uint8_t* src = a.src + (size_t)blockIdx.z * a.img_stride;
        for (int q = tid; q < rows * pw; q += NLM_THREADS) {
            const int ly = q / pw, lx = (q - ly * pw) * 4;
            const uint8_t* row = src + (size_t)nlm_reflect(gy0 + ly, a.H) * a.src_stride;
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lx + k < width) v |= (uint32_t)row[nlm_reflect(gx0 + lx + k, a.W)] << (8 * k);
            nlm_lds[q] = v;
        }
    }
    const int32_t* tab = a.tab;
    if (LDSTAB) {
        int32_t* lt = reinterpret_cast<int32_t*>(nlm_lds + rows * pw);
        for (int q = tid; q < a.ntab; q += NLM_THREADS) lt[q] = a.tab[q];
        tab = lt;
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int quad = wave & 3, half = wave >> 2;    // the wave's quadrant and its half of the search rows
    const int cg = (quad & 1) * 8 + (lane & 7);     // the lane's column group: tile columns 4 cg .. 4 cg + 3
    const int y = (quad >> 1) * 32 + (lane >> 3) * 4;  // its tile rows y .. y + 3
    // row segment j of the lane, unshifted: LDS row y + b - TH + j = y + sh + j, bytes from
    // column 4 cg + b - TH = 4 cg + sh; shifted by (dy, dx): row + dy, column + dx
    uint32_t A[NR][NDA];
    {
        const uint32_t* arow = nlm_lds + (y + sh) * pw + cg + (sh >> 2);
        const int sa = sh & 3;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            uint32_t r[ND];
#pragma unroll
            for (int k = 0; k < ND; ++k) r[k] = arow[j * pw + k];
#pragma unroll
            for (int k = 0; k < NDA; ++k) A[j][k] = __builtin_amdgcn_alignbyte(r[k + 1], r[k], sa);
        }
    }

    uint32_t est[4][4], wsum[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) est[i][c] = wsum[i][c] = 0;
    const int ntab = a.ntab, shift = a.shift;

    // search rows oy = sh + dy: 0 .. sh for the first half, sh + 1 .. 2 sh for the second
    const int oy0 = half ? sh + 1 : 0, oy1 = half ? 2 * sh : sh;
    for (int oy = oy0; oy <= oy1; ++oy) {
        const uint32_t* brow0 = nlm_lds + (y + oy) * pw + cg;
        for (int ox = 0; ox <= 2 * sh; ++ox) {  // ox = sh + dx
            const uint32_t* brow = brow0 + (ox >> 2);
            const int sb = ox & 3;
            uint32_t dist[4][4], mid[4], cen[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                mid[c] = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) dist[i][c] = 0;
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                uint32_t r[ND], B[NDA];
#pragma unroll
                for (int k = 0; k < ND; ++k) r[k] = brow[j * pw + k];
#pragma unroll
                for (int k = 0; k < NDA; ++k) B[k] = __builtin_amdgcn_alignbyte(r[k + 1], r[k], sb);
                // E[p + o] of the lane's 4 pixels of output row j - TH: bytes TH .. TH + 3
                if (j >= TH && j < TH + 4) {
                    if constexpr ((TH & 3) == 0)
                        cen[j - TH] = B[TH >> 2];
                    else
                        cen[j - TH] = __builtin_amdgcn_alignbyte(B[(TH >> 2) + 1], B[TH >> 2], TH & 3);
                }
                // squared differences of the segment, then the 4 row sums by a sliding sum
                uint32_t D[NB], R[4];
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    const int d = nlm_byte(A[j], k) - nlm_byte(B, k);
                    D[k] = (uint32_t)__mul24(d, d);
                }
                R[0] = 0;
#pragma unroll
                for (int k = 0; k <= T2; ++k) R[0] += D[k];
#pragma unroll
                for (int c = 1; c < 4; ++c) R[c] = R[c - 1] - D[c - 1] + D[c + T2];
                // row j belongs to the box of output row i when i <= j <= i + 2 th: rows inside
                // every box are added once (mid)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (j >= 3 && j <= T2) {
                        mid[c] += R[c];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (j >= i && j <= i + T2) dist[i][c] += R[c];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int idx = (int)((dist[i][c] + mid[c]) >> shift);
                    const uint32_t t = (uint32_t)tab[min(idx, ntab - 1)];
                    const uint32_t w = idx < ntab ? t : 0u;  // past the non-zero prefix: weight 0
                    est[i][c] += __umul24(w, (cen[i] >> (8 * c)) & 255u);  // w <= fpm < 2^24
                    wsum[i][c] += w;
                }
        }
    }

    // the second half's sums join the first's through LDS, over the tile and the table: every
    // wave has left the offset loop at the first barrier.  Word k of lane l at k * 256 + l.
    __syncthreads();
    uint32_t* sum = nlm_lds + (tid & 255);
    if (half) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sum[(i * 4 + c) * 256] = est[i][c];
                sum[(16 + i * 4 + c) * 256] = wsum[i][c];
            }
    }
    __syncthreads();
    if (half) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            est[i][c] += sum[(i * 4 + c) * 256];
            wsum[i][c] += sum[(16 + i * 4 + c) * 256];
        }

    uint8_t* dst = a.dst + (size_t)blockIdx.z * a.H * a.W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gy = blockIdx.y * NLM_TILE + y + i;
        if (gy >= a.H) break;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int gx = blockIdx.x * NLM_TILE + 4 * cg + c;
            if (gx < a.W) dst[(size_t)gy * a.W + gx] = (uint8_t)((est[i][c] + wsum[i][c] / 2) / wsum[i][c]);
        }
    }
}

template <bool LDSTAB>
inline void nlm_launch(int th, dim3 grid, size_t lds, hipStream_t s, const NlmArgs& a)
{
    switch (th) {
    case 0: hipLaunchKernelGGL((k_nlm_u8<0, LDSTAB>), grid, dim3(NLM_THREADS), lds, s, a); break;
    case 1: hipLaunchKernelGGL((k_nlm_u8<1, LDSTAB>), grid, dim3(NLM_THREADS), lds, s, a); break;
    case 2: hipLaunchKernelGGL((k_nlm_u8<2, LDSTAB>), grid, dim3(NLM_THREADS), lds, s, a); break;
    case 3: hipLaunchKernelGGL((k_nlm_u8<3, LDSTAB>), grid, dim3(NLM_THREADS), lds, s, a); break;
    default: hipLaunchKernelGGL((k_nlm_u8<4, LDSTAB>), grid, dim3(NLM_THREADS), lds, s, a); break;
    }
}

}  // namespace smk
