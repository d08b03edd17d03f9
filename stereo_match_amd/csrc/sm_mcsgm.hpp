// sm_mcsgm.hpp — MC-CNN's stereo method after the matching cost (Žbontar & LeCun, JMLR 2016, §4
// restated): the float32 four-path semi-global matching whose penalties depend on
// the intensity steps of both images, the left-right interpolation, the sub-pixel step, the 5x5
// median and the bilateral filter.  On the device and as a plain C++ twin that share every
// arithmetic function below, so both give the same values; every operation is a float32 add,
// subtract, multiply, divide, compare or select, and nothing is contracted into a fused
// multiply-add (the pragma below and -ffp-contract=off).
//
//   volume      V[d][y][x] float32, D planes, delta = m + d; NaN marks a cell that does not exist.
//   images      ta, tb: float32 [H][W], the view's own / the other image through the 256-entry
//               grey-level table of sm_mccnn.hpp (mc_table); a constant image (one pixel, too)
//               has the table 0, so every intensity step is 0 (this package's rule).
//   path r      L_r(p, d) = NaN where V(p, d) is NaN; V(p, d) where the predecessor q = p - r is
//               outside the image or every L_r(q, .) is NaN; else (V(p, d) - M) + e with
//               M = min of the non-NaN L_r(q, .), e = min of M + P2, L_r(q, d), L_r(q, d - 1) + P1,
//               L_r(q, d + 1) + P1 (absent terms are NaN and lose every comparison).
//   penalties   D1 = |ta(p) - ta(q)|, D2 = |tb(x - delta, y) - tb(x - delta - r_x, y - r_y)|, 0
//               where either column is outside [0, W).  Class (D1 >= sgm_D) + (D2 >= sgm_D):
//               0 (pi1, pi2), 1 (pi1 / Q1, pi2 / Q1), 2 (pi1 / Q2, pi2 / Q2); the vertical
//               paths divide P1 by sgm_V once more.  mcs_penalties computes the nine numbers
//               once on the host.
//   result      A = ((L0 + L1) + (L2 + L3)) * 0.25f, r0 from the left, r1 from the right, r2 from
//               above, r3 from below.
//
// Kernels: k_mcs_vert runs r2 and r3 (a workgroup = a strip of 32 columns x 8 chunks of planes,
// the previous row's L of a thread's chunk in registers, chunk edges and minima through LDS, one
// barrier per row); k_mcs_horz runs r0, then r1 and the sum (a wave per image row, lanes across
// the planes, tiles of 16 columns transposed through LDS, the minimum by DPP row operations).
// The image-sized stages are one thread per pixel around the mcs_*_pixel functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "sm_mccnn.hpp"  // mc_table, MC_MAXD, MC_MAXPIX, mc_clamp_min_disparity

#pragma clang fp contract(off)

namespace smk {

constexpr int MCS_MAXW = 4096;       // columns of an aggregated volume (two rows of steps sit in LDS)
constexpr int MCS_MAXR = 48;         // radius of the bilateral window
constexpr int MCS_MAXOFF = 1 << 23;  // |minDisparity|, minDisparity + D of the disparity step: float(delta) is exact
constexpr int MCS_CORRECT = 0, MCS_MISMATCH = 1, MCS_OCCLUDED = 2;

struct McsPen {
    float p1h[3], p1v[3], p2[3];  // by class: P1 of r0 / r1, P1 of r2 / r3, P2
    float thr;                    // sgm_D
};

// the penalty constants, float32 with correctly rounded divisions (host only)
inline McsPen mcs_penalties(float pi1, float pi2, float q1, float q2, float v, float d)
{
    McsPen p;
    const float div[3] = {1.0f, q1, q2};
    for (int c = 0; c < 3; c++) {
        p.p1h[c] = c ? pi1 / div[c] : pi1;
        p.p2[c] = c ? pi2 / div[c] : pi2;
        p.p1v[c] = p.p1h[c] / v;
    }
    p.thr = d;
    return p;
}

inline int mcs_blur_radius(float sigma) { return (int)std::ceil(3.0 * (double)sigma); }

// the (2R+1)^2 bilateral weights, row-major, computed in double
inline void mcs_blur_weights(float sigma, int R, float* w)
{
    const double s2 = 2.0 * (double)sigma * (double)sigma;
    for (int dy = -R; dy <= R; dy++)
        for (int dx = -R; dx <= R; dx++) w[(dy + R) * (2 * R + 1) + dx + R] = (float)std::exp(-(double)(dx * dx + dy * dy) / s2);
}

// the grey-level table of the stereo method: mc_table, all zeros for a constant image
inline void mcs_table(uint64_t sx, uint64_t sxx, uint64_t npix, float* tab)
{
    if (!mc_table(sx, sxx, npix, tab))
        for (int g = 0; g < 256; g++) tab[g] = 0.0f;
}

// ---- arithmetic shared by the kernels and the twin

__host__ __device__ inline float mcs_nan() { return __builtin_nanf(""); }

// NaN-ignoring minimum; NaN only when both are
__host__ __device__ inline float mcs_min(float a, float b) { return (b < a || a != a) ? b : a; }

__host__ __device__ inline int mcs_class(float d1, float d2, float thr) { return (d1 >= thr ? 1 : 0) + (d2 >= thr ? 1 : 0); }

__host__ __device__ inline float mcs_pick(const float* p, int cls) { return cls == 0 ? p[0] : cls == 1 ? p[1] : p[2]; }

// one cell with a live predecessor: lq, lqm, lqp = L(q, d), L(q, d - 1), L(q, d + 1) (NaN: absent)
__host__ __device__ inline float mcs_cell(float v, float M, float lq, float lqm, float lqp, float P1, float P2)
{
    float e = M + P2;
    e = lq < e ? lq : e;
    float t = lqm + P1;
    e = t < e ? t : e;
    t = lqp + P1;
    e = t < e ? t : e;
    return (v - M) + e;
}

__host__ __device__ inline float mcs_sum4(float l0, float l1, float l2, float l3) { return ((l0 + l1) + (l2 + l3)) * 0.25f; }

// ---- the image-sized stages, one pixel each (H x W maps are packed)

// winner-take-all of one pixel: m + j, or m - 1; right view: the disparity -(m_R + j) = m + D - 1 - j
__host__ __device__ inline int mcs_wta_pixel(const float* A, size_t plane, size_t pix, int D, int m, bool right)
{
    float best = mcs_nan();
    int j = -1;
    for (int d = 0; d < D; d++) {
        const float c = A[(size_t)d * plane + pix];
        if (c < best || (best != best && c == c)) best = c, j = d;
    }
    return j < 0 ? m - 1 : right ? m + D - 1 - j : m + j;
}

__host__ __device__ inline bool mcs_consistent(const int* dr_row, int W, int x, int delta, int m)
{
    const int xr = x - delta;
    if (xr < 0 || xr >= W) return false;
    const int r = dr_row[xr];
    if (r == m - 1) return false;
    const int diff = delta - r;
    return diff >= -1 && diff <= 1;
}

__host__ __device__ inline int mcs_status_pixel(const int* dl, const int* dr, int W, int D, int m, int y, int x)
{
    const int* dr_row = dr + (size_t)y * W;
    const int delta = dl[(size_t)y * W + x];
    if (delta == m - 1) return MCS_OCCLUDED;  // no plane at all
    if (mcs_consistent(dr_row, W, x, delta, m)) return MCS_CORRECT;
    for (int d = 0; d < D; d++)
        if (mcs_consistent(dr_row, W, x, m + d, m)) return MCS_MISMATCH;
    return MCS_OCCLUDED;
}

__host__ __device__ inline int mcs_fill_pixel(const int* dl, const int* st, int H, int W, int y, int x)
{
    const size_t row = (size_t)y * W;
    const int s = st[row + x], own = dl[row + x];
    if (s == MCS_CORRECT) return own;
    if (s == MCS_OCCLUDED) {
        for (int xx = x - 1; xx >= 0; xx--)
            if (st[row + xx] == MCS_CORRECT) return dl[row + xx];
        for (int xx = x + 1; xx < W; xx++)
            if (st[row + xx] == MCS_CORRECT) return dl[row + xx];
        return own;
    }
    const int dxs[16] = {1, -1, 0, 0, 1, 1, -1, -1, 1, 1, -1, -1, 2, 2, -2, -2};
    const int dys[16] = {0, 0, 1, -1, 1, -1, 1, -1, 2, -2, 2, -2, 1, -1, 1, -1};
    int vals[16], n = 0;
    for (int k = 0; k < 16; k++) {
        int xx = x + dxs[k], yy = y + dys[k];
        while (xx >= 0 && xx < W && yy >= 0 && yy < H) {
            if (st[(size_t)yy * W + xx] == MCS_CORRECT) {
                // insertion keeps vals sorted
                const int v = dl[(size_t)yy * W + xx];
                int i = n++;
                for (; i > 0 && vals[i - 1] > v; i--) vals[i] = vals[i - 1];
                vals[i] = v;
                break;
            }
            xx += dxs[k], yy += dys[k];
        }
    }
    return n ? vals[n / 2] : own;
}

__host__ __device__ inline float mcs_subpixel_pixel(const float* A, size_t plane, size_t pix, int D, int m, int delta)
{
    const float out = (float)delta;
    if (delta == m - 1) return out;
    const int j = delta - m;
    if (j <= 0 || j >= D - 1) return out;
    const float cm = A[(size_t)(j - 1) * plane + pix], c = A[(size_t)j * plane + pix], cp = A[(size_t)(j + 1) * plane + pix];
    if (cm != cm || c != c || cp != cp) return out;
    const float den = 2.0f * ((cp - 2.0f * c) + cm);
    if (den == 0.0f) return out;
    return out - (cp - cm) / den;
}

// 5x5 median over the valid (filled != m - 1) in-image values
__host__ __device__ inline float mcs_median_pixel(const float* sub, const int* filled, int H, int W, int m, int y, int x)
{
    if (filled[(size_t)y * W + x] == m - 1) return sub[(size_t)y * W + x];
    float vals[25];
    int n = 0;
    for (int dy = -2; dy <= 2; dy++)
        for (int dx = -2; dx <= 2; dx++) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W || filled[(size_t)yy * W + xx] == m - 1) continue;
            const float v = sub[(size_t)yy * W + xx];
            int i = n++;
            for (; i > 0 && vals[i - 1] > v; i--) vals[i] = vals[i - 1];
            vals[i] = v;
        }
    return vals[n / 2];
}

// w: the (2R+1)^2 weights
__host__ __device__ inline float mcs_bilateral_pixel(const float* med, const int* filled, const float* ta, const float* w,
                                                     int R, float blur_t, int H, int W, int m, int y, int x)
{
    if (filled[(size_t)y * W + x] == m - 1) return med[(size_t)y * W + x];
    const float tp = ta[(size_t)y * W + x];
    float num = 0.0f, den = 0.0f;
    for (int dy = -R; dy <= R; dy++) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -R; dx <= R; dx++) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const size_t q = (size_t)yy * W + xx;
            if (filled[q] == m - 1) continue;
            float dt = tp - ta[q];
            dt = dt < 0.0f ? -dt : dt;
            if (!(dt < blur_t)) continue;
            const float wt = w[(dy + R) * (2 * R + 1) + dx + R];
            const float prod = wt * med[q];
            num = num + prod;
            den = den + wt;
        }
    }
    return num / den;
}

// ---- the twin

// ta of one image (rows row_stride bytes apart) into packed float32 [H][W]
inline void mcs_normalise_host(const uint8_t* g, int H, int W, size_t row_stride, float* t)
{
    uint64_t sx = 0, sxx = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const uint64_t v = g[(size_t)y * row_stride + x];
            sx += v, sxx += v * v;
        }
    float tab[256];
    mcs_table(sx, sxx, (uint64_t)H * W, tab);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) t[(size_t)y * W + x] = tab[g[(size_t)y * row_stride + x]];
}

inline float mcs_step(const float* t, int W, int y0, long long x0, int y1, long long x1)
{
    if (x0 < 0 || x0 >= W || x1 < 0 || x1 >= W) return 0.0f;
    const float d = t[(size_t)y0 * W + (size_t)x0] - t[(size_t)y1 * W + (size_t)x1];
    return d < 0.0f ? -d : d;
}

// r0 (rx = 1) or r1 (rx = -1) of one image into L [D][H][W]: a row at a time, transposed to
// [x][d] so that the chain over x reads its planes side by side
inline void mcs_path_h_host(const float* V, const float* ta, const float* tb, int H, int W, int D, long long m,
                            const McsPen& pen, int rx, float* L)
{
    const size_t plane = (size_t)H * W;
    std::vector<float> vt((size_t)W * D), lt((size_t)W * D);
    for (int y = 0; y < H; y++) {
        for (int d = 0; d < D; d++)
            for (int x = 0; x < W; x++) vt[(size_t)x * D + d] = V[(size_t)d * plane + (size_t)y * W + x];
        float M = mcs_nan();
        for (int s = 0; s < W; s++) {
            const int x = rx > 0 ? s : W - 1 - s, xq = x - rx;
            const float* v = &vt[(size_t)x * D];
            float* l = &lt[(size_t)x * D];
            float Mp = mcs_nan();
            if (s == 0 || M != M) {
                for (int d = 0; d < D; d++) l[d] = v[d];
            } else {
                const float* lq = &lt[(size_t)xq * D];
                const float d1 = mcs_step(ta, W, y, x, y, xq);
                for (int d = 0; d < D; d++) {
                    const long long xb = (long long)x - (m + d);
                    const int cls = mcs_class(d1, mcs_step(tb, W, y, xb, y, xb - rx), pen.thr);
                    l[d] = mcs_cell(v[d], M, lq[d], d > 0 ? lq[d - 1] : mcs_nan(), d + 1 < D ? lq[d + 1] : mcs_nan(),
                                    mcs_pick(pen.p1h, cls), mcs_pick(pen.p2, cls));
                }
            }
            for (int d = 0; d < D; d++) Mp = mcs_min(Mp, l[d]);
            M = Mp;
        }
        for (int d = 0; d < D; d++)
            for (int x = 0; x < W; x++) L[(size_t)d * plane + (size_t)y * W + x] = lt[(size_t)x * D + d];
    }
}

// r2 (ry = 1) or r3 (ry = -1): a row at a time, the predecessors read from the row written before
inline void mcs_path_v_host(const float* V, const float* ta, const float* tb, int H, int W, int D, long long m,
                            const McsPen& pen, int ry, float* L)
{
    const size_t plane = (size_t)H * W;
    std::vector<float> M(W, mcs_nan()), Mn(W);
    for (int s = 0; s < H; s++) {
        const int y = ry > 0 ? s : H - 1 - s, yq = y - ry;
        for (int x = 0; x < W; x++) Mn[x] = mcs_nan();
        for (int d = 0; d < D; d++) {
            const float* v = V + (size_t)d * plane + (size_t)y * W;
            float* l = L + (size_t)d * plane + (size_t)y * W;
            for (int x = 0; x < W; x++) {
                if (s == 0 || M[x] != M[x]) {
                    l[x] = v[x];
                } else {
                    const float* lq = L + (size_t)d * plane + (size_t)yq * W + x;
                    const long long xb = (long long)x - (m + d);
                    const int cls = mcs_class(mcs_step(ta, W, y, x, yq, x), mcs_step(tb, W, y, xb, yq, xb), pen.thr);
                    l[x] = mcs_cell(v[x], M[x], *lq, d > 0 ? *(lq - plane) : mcs_nan(), d + 1 < D ? *(lq + plane) : mcs_nan(),
                                    mcs_pick(pen.p1v, cls), mcs_pick(pen.p2, cls));
                }
                Mn[x] = mcs_min(Mn[x], l[x]);
            }
        }
        M.swap(Mn);
    }
}

// A of one image; t0, t1: two scratch volumes
inline void mcs_aggregate_image_host(const float* V, const float* ta, const float* tb, int H, int W, int D, long long m,
                                     const McsPen& pen, float* A, float* t0, float* t1)
{
    const size_t cells = (size_t)D * H * W;
    mcs_path_h_host(V, ta, tb, H, W, D, m, pen, 1, A);
    mcs_path_h_host(V, ta, tb, H, W, D, m, pen, -1, t0);
    for (size_t i = 0; i < cells; i++) A[i] = A[i] + t0[i];
    mcs_path_v_host(V, ta, tb, H, W, D, m, pen, 1, t0);
    mcs_path_v_host(V, ta, tb, H, W, D, m, pen, -1, t1);
    for (size_t i = 0; i < cells; i++) A[i] = (A[i] + (t0[i] + t1[i])) * 0.25f;
}

// n volumes [D][H][W] with their images into agg; iters = sgm_i
inline void mcsgm_aggregate_host(const float* vol, const uint8_t* a, const uint8_t* b, int n, size_t image_stride, int H, int W,
                                 size_t row_stride, int D, int minD, const McsPen& pen, int iters, float* agg)
{
    const size_t npix = (size_t)H * W, cells = npix * D;
    const long long m = mc_clamp_min_disparity(minD, W, D);
    std::vector<float> ta(npix), tb(npix), t0(cells), t1(cells), tmp(iters > 1 ? cells : 0);
    for (int img = 0; img < n; img++) {
        mcs_normalise_host(a + (size_t)img * image_stride, H, W, row_stride, ta.data());
        mcs_normalise_host(b + (size_t)img * image_stride, H, W, row_stride, tb.data());
        const float* src = vol + (size_t)img * cells;
        float* out = agg + (size_t)img * cells;
        for (int it = 0; it < iters; it++) {
            float* dst = (iters - 1 - it) % 2 == 0 ? out : tmp.data();
            mcs_aggregate_image_host(src, ta.data(), tb.data(), H, W, D, m, pen, dst, t0.data(), t1.data());
            src = dst;
        }
    }
}

struct McsMaps {  // the stages of one image, packed [H][W]
    int *wta_l, *wta_r, *status, *filled;
    float *sub, *med, *out;
};

inline void mcs_disparity_image_host(const float* AL, const float* AR, const float* ta, int H, int W, int D, int m, int R,
                                     const float* w, float blur_t, const McsMaps& o)
{
    const size_t plane = (size_t)H * W;
    for (size_t p = 0; p < plane; p++) {
        o.wta_l[p] = mcs_wta_pixel(AL, plane, p, D, m, false);
        o.wta_r[p] = mcs_wta_pixel(AR, plane, p, D, m, true);
    }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) o.status[(size_t)y * W + x] = mcs_status_pixel(o.wta_l, o.wta_r, W, D, m, y, x);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) o.filled[(size_t)y * W + x] = mcs_fill_pixel(o.wta_l, o.status, H, W, y, x);
    for (size_t p = 0; p < plane; p++) o.sub[p] = mcs_subpixel_pixel(AL, plane, p, D, m, o.filled[p]);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) o.med[(size_t)y * W + x] = mcs_median_pixel(o.sub, o.filled, H, W, m, y, x);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            o.out[(size_t)y * W + x] = mcs_bilateral_pixel(o.med, o.filled, ta, w, R, blur_t, H, W, m, y, x);
}

// the disparity maps of n images; maps: where the stages go ([n][H][W] each; out is the result,
// any other member may be null)
inline void mcsgm_disparity_host(const float* agg_l, const float* agg_r, const uint8_t* a, int n, size_t image_stride, int H,
                                 int W, size_t row_stride, int D, int m, float blur_sigma, float blur_t, const McsMaps& maps)
{
    const size_t npix = (size_t)H * W, cells = npix * D;
    const int R = mcs_blur_radius(blur_sigma);
    std::vector<float> w((size_t)(2 * R + 1) * (2 * R + 1)), ta(npix), fs[2];
    std::vector<int> is[4];
    mcs_blur_weights(blur_sigma, R, w.data());
    int* const given_i[4] = {maps.wta_l, maps.wta_r, maps.status, maps.filled};
    float* const given_f[2] = {maps.sub, maps.med};
    for (int k = 0; k < 4; k++)
        if (!given_i[k]) is[k].resize(npix);
    for (int k = 0; k < 2; k++)
        if (!given_f[k]) fs[k].resize(npix);
    for (int img = 0; img < n; img++) {
        const size_t o = (size_t)img * npix;
        mcs_normalise_host(a + (size_t)img * image_stride, H, W, row_stride, ta.data());
        int* pi[4];
        float* pf[2];
        for (int k = 0; k < 4; k++) pi[k] = given_i[k] ? given_i[k] + o : is[k].data();
        for (int k = 0; k < 2; k++) pf[k] = given_f[k] ? given_f[k] + o : fs[k].data();
        mcs_disparity_image_host(agg_l + (size_t)img * cells, agg_r + (size_t)img * cells, ta.data(), H, W, D, m, R, w.data(), blur_t,
                                 McsMaps{pi[0], pi[1], pi[2], pi[3], pf[0], pf[1], maps.out + o});
    }
}

#if defined(__HIPCC__) && !defined(SM_MCSGM_NO_KERNELS)  // sm_mccbca.hpp's unit takes the host functions only
// ---- kernels

constexpr int MCS_BLOCK = 256;

struct McsNormArgs {
    const uint8_t* gray;  // one image
    size_t row_stride;
    int H, W;
    const float* tab;  // its 256 grey levels
    float* t;          // [H][W]
};

__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_norm(McsNormArgs a)
{
    __shared__ float tab[256];
    tab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();
    const unsigned i = blockIdx.x * MCS_BLOCK + threadIdx.x;
    if (i >= (unsigned)a.H * (unsigned)a.W) return;
    const unsigned y = i / (unsigned)a.W, x = i - y * (unsigned)a.W;
    a.t[i] = tab[a.gray[(size_t)y * a.row_stride + x]];
}

struct McsSumArgs {
    const uint8_t* gray;
    size_t image_stride, row_stride;
    int H, W;
    unsigned long long* sums;  // [img][2]: Sx, Sxx (zeroed before the launch)
};

// exact integer sums of every image: blockIdx.y the image, the blocks stride over its pixels
__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_sums(McsSumArgs a)
{
    const uint8_t* g = a.gray + (size_t)blockIdx.y * a.image_stride;
    const unsigned npix = (unsigned)a.H * (unsigned)a.W;
    unsigned long long sx = 0, sxx = 0;
    for (unsigned i = blockIdx.x * MCS_BLOCK + threadIdx.x; i < npix; i += gridDim.x * MCS_BLOCK) {
        const unsigned y = i / (unsigned)a.W, x = i - y * (unsigned)a.W;
        const unsigned long long v = g[(size_t)y * a.row_stride + x];
        sx += v, sxx += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_down(sx, o);
        sxx += __shfl_down(sxx, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&a.sums[2 * blockIdx.y], sx);
        atomicAdd(&a.sums[2 * blockIdx.y + 1], sxx);
    }
}

struct McsAggArgs {
    const float* V;   // [D][H][W]
    const float* ta;  // [H][W]
    const float* tb;
    float* A;         // [D][H][W]: L0, then the result (k_mcs_horz)
    float* L2;        // [D][H][W]: r2 (from above), written by k_mcs_vert, read by k_mcs_horz
    float* L3;        // r3 (from below)
    int H, W, D, m;   // m clamped (mc_clamp_min_disparity)
    McsPen pen;
};

constexpr int MCS_VX = 32;                   // columns of a vertical strip
constexpr int MCS_VC = MCS_BLOCK / MCS_VX;   // chunks of planes
constexpr int MCS_VK = MC_MAXD / MCS_VC;     // planes of a chunk at most
constexpr int MCS_VSEG = MC_MAXD + MCS_VX;   // columns of b a strip can meet (D + 31 used)

// r2 (blockIdx.y == 0, rows downwards) and r3 (1, upwards) of a strip of 32 columns.  Thread
// (tx, tc) owns planes tc * cpc .. of column x0 + tx and keeps the previous row's L of them in
// registers.  Per row the workgroup exchanges through LDS (two copies, by row parity, so one
// barrier a row is enough): the first and last L of every chunk, the chunk minima, and the
// steps of b over the D + 31 columns the strip's cells look at.
__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_vert(McsAggArgs a)
{
    __shared__ float s_first[2][MCS_VC][MCS_VX], s_last[2][MCS_VC][MCS_VX], s_min[2][MCS_VC][MCS_VX];
    __shared__ float s_db[2][MCS_VSEG];
    const int tid = threadIdx.x, tx = tid & (MCS_VX - 1), tc = tid / MCS_VX;
    const int x0 = blockIdx.x * MCS_VX, x = x0 + tx;
    const bool up = blockIdx.y != 0, live = x < a.W;
    const int cpc = (a.D + MCS_VC - 1) / MCS_VC, d0 = tc * cpc;
    const int cnt = max(0, min(cpc, a.D - d0));
    const size_t plane = (size_t)a.H * a.W;
    float* out = up ? a.L3 : a.L2;
    const int seg0 = x0 - a.m - (a.D - 1), nseg = a.D + MCS_VX - 1;  // entry i of s_db is column seg0 + i of b

    float L[MCS_VK], v[MCS_VK];
#pragma unroll
    for (int k = 0; k < MCS_VK; k++) L[k] = mcs_nan();
    float ta_prev = 0.0f, tb_prev[2] = {0.0f, 0.0f};

    for (int s = 0; s < a.H; s++) {
        const int y = up ? a.H - 1 - s : s, par = s & 1;
        const size_t pix = (size_t)y * a.W + x;
#pragma unroll
        for (int k = 0; k < MCS_VK; k++) v[k] = (live && k < cnt) ? a.V[(size_t)(d0 + k) * plane + pix] : mcs_nan();
        // what the row needs from the other threads
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int i = tid + h * MCS_BLOCK, xb = seg0 + i;
            if (i < nseg) {
                const bool in = xb >= 0 && xb < a.W;
                const float t = in ? a.tb[(size_t)y * a.W + xb] : 0.0f;
                const float df = t - tb_prev[h];
                s_db[par][i] = in ? (df < 0.0f ? -df : df) : 0.0f;
                tb_prev[h] = t;
            }
        }
        {
            float mn = mcs_nan(), last = mcs_nan();
#pragma unroll
            for (int k = 0; k < MCS_VK; k++)
                if (k < cnt) mn = mcs_min(mn, L[k]), last = L[k];
            s_first[par][tc][tx] = L[0];
            s_last[par][tc][tx] = last;
            s_min[par][tc][tx] = mn;
        }
        __syncthreads();
        float M = mcs_nan();
#pragma unroll
        for (int c = 0; c < MCS_VC; c++) M = mcs_min(M, s_min[par][c][tx]);
        const float ta_cur = live ? a.ta[pix] : 0.0f;
        if (s > 0 && M == M) {
            float d1 = ta_cur - ta_prev;
            d1 = d1 < 0.0f ? -d1 : d1;
            float lqm = (tc > 0 && cnt > 0) ? s_last[par][tc - 1][tx] : mcs_nan();
            const float nxt = (tc + 1 < MCS_VC && d0 + cnt < a.D) ? s_first[par][tc + 1][tx] : mcs_nan();
#pragma unroll
            for (int k = 0; k < MCS_VK; k++) {
                if (k < cnt) {
                    const float lq = L[k];
                    float lqp = nxt;
                    if (k + 1 < MCS_VK && k + 1 < cnt) lqp = L[k + 1 < MCS_VK ? k + 1 : k];
                    const float d2 = s_db[par][tx + (a.D - 1 - (d0 + k))];
                    const int cls = mcs_class(d1, d2, a.pen.thr);
                    L[k] = mcs_cell(v[k], M, lq, lqm, lqp, mcs_pick(a.pen.p1v, cls), mcs_pick(a.pen.p2, cls));
                    lqm = lq;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < MCS_VK; k++) L[k] = v[k];
        }
        ta_prev = ta_cur;
        if (live) {
#pragma unroll
            for (int k = 0; k < MCS_VK; k++)
                if (k < cnt) out[(size_t)(d0 + k) * plane + pix] = L[k];
        }
    }
}

constexpr int MCS_HX = 16;           // columns of a tile of the horizontal paths
constexpr int MCS_HS = MCS_HX + 1;   // floats between the planes of the LDS tile (odd: a wave's planes hit 32 banks)

// one step of the wave minimum: lanes the DPP control gives no source see NaN, which mcs_min ignores
template <int CTRL>
__device__ inline float mcs_dpp_min(float r)
{
    const int t = __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, mcs_nan()), __builtin_bit_cast(int, r), CTRL, 0xf, 0xf, false);
    return mcs_min(r, __builtin_bit_cast(float, t));
}

__device__ inline float mcs_readlane(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// NaN-ignoring minimum of a wave, the same in every lane: quads, rows of 16, then the rows' last
// lanes handed on (row_bcast), after which lane 63 holds the minimum of all 64
__device__ inline float mcs_wave_min(float r)
{
    r = mcs_dpp_min<0xb1>(r);   // quad_perm [1,0,3,2]
    r = mcs_dpp_min<0x4e>(r);   // quad_perm [2,3,0,1]
    r = mcs_dpp_min<0x114>(r);  // row_shr 4
    r = mcs_dpp_min<0x118>(r);  // row_shr 8
    r = mcs_dpp_min<0x142>(r);  // row_bcast 15
    r = mcs_dpp_min<0x143>(r);  // row_bcast 31
    return mcs_readlane(r, 63);
}

// r0, then r1 and the sum of the four paths, of image row blockIdx.x: one wave, lane l owns
// planes l + 64 j (j < NJ).  A tile of 16 columns x 64 NJ planes goes through LDS: loaded with
// 64-byte row segments (the next tile's loads are in flight while this one runs), read and
// overwritten column by column by the lanes that own the planes, and flushed the way it came:
// r0 stores L0 into A, r1 stores ((L0 + L1) + (L2 + L3)) / 4 there.  s_ga / s_gb: the steps
// |t(i) - t(i - 1)| of the two image rows, 0 at i = 0 and i = W.
template <int NJ>
__global__ __launch_bounds__(64) void k_mcs_horz(McsAggArgs a)
{
    extern __shared__ __align__(16) float s_mem[];
    float* tile = s_mem;                        // [64 NJ][MCS_HS]
    float* s_ga = tile + 64 * NJ * MCS_HS;      // [W + 1]
    float* s_gb = s_ga + (a.W + 1);             // [W + 1]
    constexpr int NLD = MCS_HX * NJ;            // loads of a tile per lane: planes 4 i + (lane >> 4), column lane & 15
    const int lane = threadIdx.x, y = blockIdx.x;
    const size_t plane = (size_t)a.H * a.W, rowoff = (size_t)y * a.W;
    const int ldd = lane >> 4, lxx = lane & 15;

    for (int i = lane; i <= a.W; i += 64) {
        float ga = 0.0f, gb = 0.0f;
        if (i >= 1 && i < a.W) {
            ga = a.ta[rowoff + i] - a.ta[rowoff + i - 1];
            gb = a.tb[rowoff + i] - a.tb[rowoff + i - 1];
            ga = ga < 0.0f ? -ga : ga;
            gb = gb < 0.0f ? -gb : gb;
        }
        s_ga[i] = ga, s_gb[i] = gb;
    }

    const int ntiles = (a.W + MCS_HX - 1) / MCS_HX;
    for (int dir = 0; dir < 2; dir++) {
        float pre[NLD], Lq[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++) Lq[j] = mcs_nan();
        float M = mcs_nan();
        auto fetch = [&](int t) {
            const int xc = t * MCS_HX + lxx;
#pragma unroll
            for (int i = 0; i < NLD; i++) {
                const int d = 4 * i + ldd;
                pre[i] = (d < a.D && xc < a.W) ? a.V[(size_t)d * plane + rowoff + xc] : mcs_nan();
            }
        };
        fetch(dir ? ntiles - 1 : 0);
        for (int ti = 0; ti < ntiles; ti++) {
            const int t = dir ? ntiles - 1 - ti : ti, x0 = t * MCS_HX;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NLD; i++) tile[(4 * i + ldd) * MCS_HS + lxx] = pre[i];
            __syncthreads();
            if (ti + 1 < ntiles) fetch(dir ? t - 1 : t + 1);
            for (int si = 0; si < MCS_HX; si++) {
                const int xx = dir ? MCS_HX - 1 - si : si, x = x0 + xx;
                if (x >= a.W) continue;
                float v[NJ], Ln[NJ];
#pragma unroll
                for (int j = 0; j < NJ; j++) v[j] = tile[(lane + 64 * j) * MCS_HS + xx];
                const bool first = dir ? x == a.W - 1 : x == 0;
                if (first || M != M) {
#pragma unroll
                    for (int j = 0; j < NJ; j++) Ln[j] = v[j];
                } else {
                    const float d1 = s_ga[x + dir];
#pragma unroll
                    for (int j = 0; j < NJ; j++) {
                        float lqm = __shfl_up(Lq[j], 1), lqp = __shfl_down(Lq[j], 1);
                        const float wrap_m = j > 0 ? mcs_readlane(Lq[j > 0 ? j - 1 : 0], 63) : mcs_nan();
                        const float wrap_p = j + 1 < NJ ? mcs_readlane(Lq[j + 1 < NJ ? j + 1 : j], 0) : mcs_nan();
                        if (lane == 0) lqm = wrap_m;
                        if (lane == 63) lqp = wrap_p;
                        const int xb = x - a.m - (lane + 64 * j);
                        const float d2 = (xb >= 0 && xb < a.W) ? s_gb[xb + dir] : 0.0f;
                        const int cls = mcs_class(d1, d2, a.pen.thr);
                        Ln[j] = mcs_cell(v[j], M, Lq[j], lqm, lqp, mcs_pick(a.pen.p1h, cls), mcs_pick(a.pen.p2, cls));
                    }
                }
                float mn = mcs_nan();
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    Lq[j] = Ln[j];
                    mn = mcs_min(mn, Ln[j]);
                    tile[(lane + 64 * j) * MCS_HS + xx] = Ln[j];
                }
                M = mcs_wave_min(mn);
            }
            __syncthreads();
            const int xc = x0 + lxx;
#pragma unroll
            for (int i = 0; i < NLD; i++) {
                const int d = 4 * i + ldd;
                if (d < a.D && xc < a.W) {
                    const size_t o = (size_t)d * plane + rowoff + xc;
                    const float l = tile[d * MCS_HS + lxx];
                    a.A[o] = dir ? mcs_sum4(a.A[o], l, a.L2[o], a.L3[o]) : l;
                }
            }
        }
    }
}

struct McsDispArgs {
    const float* AL;  // [D][H][W]
    const float* AR;
    const float* ta;  // [H][W]
    const float* w;   // (2R+1)^2 bilateral weights
    int H, W, D, m, R;
    float blur_t;
    McsMaps o;
};

__device__ inline bool mcs_pixel(const McsDispArgs& a, unsigned& p, int& y, int& x)
{
    p = blockIdx.x * MCS_BLOCK + threadIdx.x;
    if (p >= (unsigned)a.H * (unsigned)a.W) return false;
    y = (int)(p / (unsigned)a.W), x = (int)(p - (unsigned)y * (unsigned)a.W);
    return true;
}

__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_wta(McsDispArgs a)
{
    unsigned p;
    int y, x;
    if (!mcs_pixel(a, p, y, x)) return;
    const size_t plane = (size_t)a.H * a.W;
    a.o.wta_l[p] = mcs_wta_pixel(a.AL, plane, p, a.D, a.m, false);
    a.o.wta_r[p] = mcs_wta_pixel(a.AR, plane, p, a.D, a.m, true);
}

__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_status(McsDispArgs a)
{
    unsigned p;
    int y, x;
    if (!mcs_pixel(a, p, y, x)) return;
    a.o.status[p] = mcs_status_pixel(a.o.wta_l, a.o.wta_r, a.W, a.D, a.m, y, x);
}

__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_fill(McsDispArgs a)
{
    unsigned p;
    int y, x;
    if (!mcs_pixel(a, p, y, x)) return;
    a.o.filled[p] = mcs_fill_pixel(a.o.wta_l, a.o.status, a.H, a.W, y, x);
}

__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_subpixel(McsDispArgs a)
{
    unsigned p;
    int y, x;
    if (!mcs_pixel(a, p, y, x)) return;
    a.o.sub[p] = mcs_subpixel_pixel(a.AL, (size_t)a.H * a.W, p, a.D, a.m, a.o.filled[p]);
}

__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_median(McsDispArgs a)
{
    unsigned p;
    int y, x;
    if (!mcs_pixel(a, p, y, x)) return;
    a.o.med[p] = mcs_median_pixel(a.o.sub, a.o.filled, a.H, a.W, a.m, y, x);
}

// the weight table in LDS; a workgroup is 32 x 8 pixels, so its taps share cache lines
__global__ __launch_bounds__(MCS_BLOCK) void k_mcs_bilateral(McsDispArgs a)
{
    extern __shared__ __align__(16) float s_w[];
    const int nw = (2 * a.R + 1) * (2 * a.R + 1);
    for (int i = threadIdx.x; i < nw; i += MCS_BLOCK) s_w[i] = a.w[i];
    __syncthreads();
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= a.W || y >= a.H) return;
    a.o.out[(size_t)y * a.W + x] = mcs_bilateral_pixel(a.o.med, a.o.filled, a.ta, s_w, a.R, a.blur_t, a.H, a.W, a.m, y, x);
}
#endif  // __HIPCC__

}  // namespace smk
