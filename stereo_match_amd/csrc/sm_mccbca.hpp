// sm_mccbca.hpp — cross-based cost aggregation of MC-CNN's stereo method (Žbontar & LeCun, JMLR
// 2016, §4.1 restated): the matching cost averaged over a support region that
// follows the edges of both images.  On the device and as a plain C++ twin that share every
// arithmetic function below; every operation is a float32 add, subtract, compare or divide in a
// fixed order, nothing is contracted (the pragma below and -ffp-contract=off) and the division is
// correctly rounded, so both give the same values.
//
//   volume   C[d][y][x] float32, D planes, delta = m + d; a cell exists where x - delta is a column.
//   images   t: float32 [H][W], an image through the grey-level table of §4.18 (mcs_table: a
//            constant image is all zeros).
//   arms     n_s(p), s one of left, right, up, down: the largest n <= L1 - 1 with p + k s inside the
//            image and |t(p) - t(p + k s)| < tau1 for every k = 1 .. n.  Four bytes a pixel.
//   one step a cell that does not exist is copied.  Else, with x_b = x - delta:
//            l = min(la(x, y), lb(x_b, y)), r, u, w likewise from the right, up and down arms;
//            S(x, y, d) = C[d][y][x - l] + ... + C[d][y][x + r], ascending, from the first term;
//            n_h = l + r + 1;
//            T = S(x, y - u, d) + ... + S(x, y + w, d), ascending, from the first term;
//            N = the sum of n_h over the same rows;  C'(x, y, d) = T / float(N).
//
// Kernels: k_mcb_arms, one thread per pixel; k_mcb_agg, one launch per step: a workgroup takes a
// tile of 64 columns x TY rows of one plane with a halo of L1 - 1 cells on every side into LDS,
// writes S and n_h of every tile row (halo rows too) into LDS, and after one barrier sums them
// down the columns and divides.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "sm_mcsgm.hpp"  // mcs_normalise_host, MCS_MAXW; sm_mccnn.hpp: mc_clamp_min_disparity

#pragma clang fp contract(off)

namespace smk {

constexpr int MCB_MAXL = 32;   // L1 at most: an arm fits a byte, N <= 63^2 is exact in float32
constexpr int MCB_MAXI = 16;   // iterations of one call
constexpr int MCB_TX = 64;     // columns of a tile: a wave's lanes
constexpr int MCB_BLOCK = 256;
constexpr size_t MCB_LDS = 65536;

// LDS of a tile of ty rows with a halo of h: the costs, S and n_h
__host__ __device__ inline size_t mcb_lds_bytes(int ty, int h)
{
    const size_t rows = (size_t)ty + 2 * h;
    return rows * (MCB_TX + 2 * h) * 4 + rows * MCB_TX * 4 + rows * MCB_TX;
}

// rows of a tile: 32 while the tile, its halo and its sums fit 64 KiB of LDS (L1 <= 26), else 16
inline int mcb_tile_rows(int h) { return mcb_lds_bytes(32, h) <= MCB_LDS ? 32 : 16; }

// ---- arithmetic shared by the kernels and the twin

// the arm of pixel (x, y) of t along (sx, sy)
__host__ __device__ inline int mcb_arm(const float* t, int H, int W, int y, int x, int sx, int sy, int L1, float tau1)
{
    const float tp = t[(size_t)y * W + x];
    int n = 0;
    for (int k = 1; k < L1; k++) {
        const int xx = x + k * sx, yy = y + k * sy;
        if (xx < 0 || xx >= W || yy < 0 || yy >= H) break;
        float d = tp - t[(size_t)yy * W + xx];
        d = d < 0.0f ? -d : d;
        if (!(d < tau1)) break;
        n = k;
    }
    return n;
}

// the four arms of a pixel in one word: left, right << 8, up << 16, down << 24
__host__ __device__ inline uint32_t mcb_arms_pixel(const float* t, int H, int W, int y, int x, int L1, float tau1)
{
    return (uint32_t)mcb_arm(t, H, W, y, x, -1, 0, L1, tau1) | (uint32_t)mcb_arm(t, H, W, y, x, 1, 0, L1, tau1) << 8 |
           (uint32_t)mcb_arm(t, H, W, y, x, 0, -1, L1, tau1) << 16 | (uint32_t)mcb_arm(t, H, W, y, x, 0, 1, L1, tau1) << 24;
}

// the shorter arm of two packed words, side 0 .. 3
__host__ __device__ inline int mcb_min_arm(uint32_t pa, uint32_t pb, int side)
{
    const int a = (int)(pa >> (8 * side)) & 255, b = (int)(pb >> (8 * side)) & 255;
    return a < b ? a : b;
}

// p[0] + p[stride] + ... + p[(cnt - 1) stride], ascending, from the first term (cnt >= 1)
__host__ __device__ inline float mcb_sum(const float* p, int stride, int cnt)
{
    float s = p[0];
    for (int k = 1; k < cnt; k++) s = s + p[(size_t)k * stride];
    return s;
}

// ---- the twin

// packed arms [H][W] of a normalised image
inline void mcb_arms_host(const float* t, int H, int W, int L1, float tau1, uint32_t* arms)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) arms[(size_t)y * W + x] = mcb_arms_pixel(t, H, W, y, x, L1, tau1);
}

// the arms of n images as uint8 [n][4][H][W]: left, right, up, down
inline void mccbca_arms_host(const uint8_t* g, int n, size_t image_stride, int H, int W, size_t row_stride, int L1, float tau1,
                             uint8_t* out)
{
    const size_t npix = (size_t)H * W;
    std::vector<float> t(npix);
    for (int img = 0; img < n; img++) {
        mcs_normalise_host(g + (size_t)img * image_stride, H, W, row_stride, t.data());
        uint8_t* o = out + (size_t)img * 4 * npix;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const uint32_t p = mcb_arms_pixel(t.data(), H, W, y, x, L1, tau1);
                for (int s = 0; s < 4; s++) o[(size_t)s * npix + (size_t)y * W + x] = (uint8_t)(p >> (8 * s));
            }
    }
}

// one step of one image: C -> out, both [D][H][W]; S and nh: scratch planes [H][W]
inline void mcb_step_host(const float* C, const uint32_t* pa, const uint32_t* pb, int H, int W, int D, long long m, float* out,
                          float* S, uint8_t* nh)
{
    const size_t plane = (size_t)H * W;
    for (int d = 0; d < D; d++) {
        const float* c = C + (size_t)d * plane;
        float* o = out + (size_t)d * plane;
        const long long delta = m + d;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const long long xb = x - delta;
                if (xb < 0 || xb >= W) continue;
                const size_t p = (size_t)y * W + x;
                const uint32_t a = pa[p], b = pb[(size_t)y * W + (size_t)xb];
                const int l = mcb_min_arm(a, b, 0), r = mcb_min_arm(a, b, 1);
                S[p] = mcb_sum(c + p - l, 1, l + r + 1);
                nh[p] = (uint8_t)(l + r + 1);
            }
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const long long xb = x - delta;
                const size_t p = (size_t)y * W + x;
                if (xb < 0 || xb >= W) {
                    o[p] = c[p];
                    continue;
                }
                const uint32_t a = pa[p], b = pb[(size_t)y * W + (size_t)xb];
                const int u = mcb_min_arm(a, b, 2), w = mcb_min_arm(a, b, 3);
                const float T = mcb_sum(S + p - (size_t)u * W, W, u + w + 1);
                int N = 0;
                for (int k = -u; k <= w; k++) N += nh[(ptrdiff_t)p + (ptrdiff_t)k * W];
                o[p] = T / (float)N;
            }
    }
}

// n volumes [D][H][W] with their images, iters steps each
inline void mccbca_aggregate_host(const float* vol, const uint8_t* a, const uint8_t* b, int n, size_t image_stride, int H, int W,
                                  size_t row_stride, int D, int minD, int L1, float tau1, int iters, float* agg)
{
    const size_t npix = (size_t)H * W, cells = npix * D;
    const long long m = mc_clamp_min_disparity(minD, W, D);
    std::vector<float> t(npix), S(npix), tmp(iters > 1 ? cells : 0);
    std::vector<uint32_t> pa(npix), pb(npix);
    std::vector<uint8_t> nh(npix);
    for (int img = 0; img < n; img++) {
        mcs_normalise_host(a + (size_t)img * image_stride, H, W, row_stride, t.data());
        mcb_arms_host(t.data(), H, W, L1, tau1, pa.data());
        mcs_normalise_host(b + (size_t)img * image_stride, H, W, row_stride, t.data());
        mcb_arms_host(t.data(), H, W, L1, tau1, pb.data());
        const float* src = vol + (size_t)img * cells;
        float* out = agg + (size_t)img * cells;
        for (int it = 0; it < iters; it++) {
            float* dst = (iters - 1 - it) % 2 == 0 ? out : tmp.data();
            mcb_step_host(src, pa.data(), pb.data(), H, W, D, m, dst, S.data(), nh.data());
            src = dst;
        }
    }
}

#if defined(__HIPCC__)
// ---- kernels

struct McbArmsArgs {
    const float* t;     // [H][W]
    int H, W, L1;
    float tau1;
    uint32_t* packed;   // [H][W], or null
    uint8_t* planar;    // [4][H][W], or null
};

__global__ __launch_bounds__(MCB_BLOCK) void k_mcb_arms(McbArmsArgs a)
{
    const unsigned p = blockIdx.x * MCB_BLOCK + threadIdx.x, npix = (unsigned)a.H * (unsigned)a.W;
    if (p >= npix) return;
    const int y = (int)(p / (unsigned)a.W), x = (int)(p - (unsigned)y * (unsigned)a.W);
    const uint32_t w = mcb_arms_pixel(a.t, a.H, a.W, y, x, a.L1, a.tau1);
    if (a.packed) a.packed[p] = w;
    if (a.planar)
        for (int s = 0; s < 4; s++) a.planar[(size_t)s * npix + p] = (uint8_t)(w >> (8 * s));
}

struct McbAggArgs {
    const float* C;      // [D][H][W]
    float* out;          // [D][H][W]
    const uint32_t* pa;  // packed arms of the view's own image [H][W]
    const uint32_t* pb;  // of the other image
    int H, W, D, m;      // m clamped (mc_clamp_min_disparity)
    int h, ty;           // L1 - 1; rows of a tile (mcb_tile_rows)
};

// Tile (column blockIdx.y, row blockIdx.x: H may need more than 65535 tiles) of plane blockIdx.z.  LDS: s_c, the costs of rows y0 - h ..
// y0 + ty + h - 1 and columns x0 - h .. x0 + 63 + h (0 outside the image: never summed, an arm ends
// at the border); s_s and s_n, S and n_h of the tile's columns in the same rows.  A wave works on
// one row at a time, its lanes on neighbouring columns: the horizontal sums read s_c along a row
// and the vertical sums read s_s down a column with the lanes side by side, so both are free of
// bank conflicts up to the lanes' different arms.
__global__ __launch_bounds__(MCB_BLOCK) void k_mcb_agg(McbAggArgs a)
{
    extern __shared__ __align__(16) float s_mcb[];
    const int h = a.h, rows = a.ty + 2 * h, cw = MCB_TX + 2 * h;
    float* s_c = s_mcb;                                    // [rows][cw]
    float* s_s = s_c + (size_t)rows * cw;                  // [rows][64]
    uint8_t* s_n = (uint8_t*)(s_s + (size_t)rows * MCB_TX);  // [rows][64]
    const int tid = threadIdx.x, x0 = blockIdx.y * MCB_TX, y0 = blockIdx.x * a.ty, d = blockIdx.z;
    const size_t plane = (size_t)a.H * a.W;
    const float* C = a.C + (size_t)d * plane;

    for (unsigned i = tid; i < (unsigned)(rows * cw); i += MCB_BLOCK) {
        const unsigned r = i / (unsigned)cw, c = i - r * (unsigned)cw;
        const int gy = y0 - h + (int)r, gx = x0 - h + (int)c;
        s_c[i] = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? C[(size_t)gy * a.W + gx] : 0.0f;
    }
    __syncthreads();

    const int c = tid & (MCB_TX - 1), gx = x0 + c;
    const int xb = gx - (a.m + d);  // |m| <= W + D: no overflow
    const bool exists = gx < a.W && xb >= 0 && xb < a.W;
    for (int r = tid / MCB_TX; r < rows; r += MCB_BLOCK / MCB_TX) {
        const int gy = y0 - h + r;
        if (!exists || gy < 0 || gy >= a.H) continue;
        const uint32_t pa = a.pa[(size_t)gy * a.W + gx], pb = a.pb[(size_t)gy * a.W + xb];
        const int l = mcb_min_arm(pa, pb, 0), rr = mcb_min_arm(pa, pb, 1);
        s_s[r * MCB_TX + c] = mcb_sum(s_c + (size_t)r * cw + (c + h - l), 1, l + rr + 1);
        s_n[r * MCB_TX + c] = (uint8_t)(l + rr + 1);
    }
    __syncthreads();

    for (int r = tid / MCB_TX; r < a.ty; r += MCB_BLOCK / MCB_TX) {
        const int gy = y0 + r;
        if (gx >= a.W || gy >= a.H) continue;
        const size_t p = (size_t)gy * a.W + gx;
        float v = s_c[(size_t)(r + h) * cw + c + h];
        if (exists) {
            const uint32_t pa = a.pa[p], pb = a.pb[(size_t)gy * a.W + xb];
            const int u = mcb_min_arm(pa, pb, 2), w = mcb_min_arm(pa, pb, 3);
            const int first = (r + h - u) * MCB_TX + c;
            const float T = mcb_sum(s_s + first, MCB_TX, u + w + 1);
            int N = 0;
            for (int k = 0; k <= u + w; k++) N += s_n[first + k * MCB_TX];
            v = T / (float)N;
        }
        a.out[(size_t)d * plane + p] = v;
    }
}
#endif  // __HIPCC__

}  // namespace smk
