// sm_filter.hpp — the two host image filters left in the reference's scripts:
//   k_gauss2d_f64  scipy.ndimage.gaussian_filter(mode='reflect') on float64 images, both axes in
//                  one kernel; image_measure (disparity_test.py:54-66) is two launches of it,
//                  the BGR->gray conversion fused into the first one's tile load and the unsharp
//                  expression a + alpha * (a - b) into the second one's row pass
//   k_pyr_down_u8  cv2.pyrDown on uint8, 1 or 3 channels, default size and border
// Semantics (tests/filters_np.py is the independent restatement):
//  gauss, per filtered axis with the half kernel w[0..r] (centre first; the host computes it
//   with scipy's own numpy expressions), for output index i on a line of length n:
//     t = a[i] * w[0];  for j = r, r-1, ..., 1:  t = t + (a[refl(i-j)] + a[refl(i+j)]) * w[j]
//   every product and sum rounded to float64 (FP contraction off: an FMA would differ from
//   scipy in the last bit); refl(k) = k mod 2n, then 2n-1-k when >= n (scipy's 'reflect', valid
//   for any r, r >= n included); axis 0 over the whole image first, then axis 1 on that
//   result.  r = 0 with w[0] = 1 is the identity.
//  pyrDown: dst[y,x,c] = (sum_{i,j=-2..2} k[i] k[j] src[r101(2y+i,H)][r101(2x+j,W)][c] + 128) >> 8,
//   k = (1,4,6,4,1), r101 = BORDER_REFLECT_101; dH = (H+1)/2, dW = (W+1)/2.
// Gaussian kernel: a 256-thread workgroup owns a 64 x 32 tile of output pixels.  The axis-0
// result is needed on the tile's columns plus an rx-wide halo on both sides (the axis-0 result
// at a reflected column is the axis-0 result of the mirrored column, so the halo is computed
// from reflected source columns).  That region is worked through in strips of 64 columns: a
// strip's source rows (32 + 2 ry of them, reflection resolved, gray conversion applied) are
// staged in LDS, each lane runs the column pass for 8 rows of one column and leaves the
// result in a second LDS array [32][64 + 2 rx]; when every strip is done the row pass reads
// that array and writes the tile.  Strips bound the staging array, so one code path serves
// every radius up to GF_MAX_R: 62 KiB of LDS at r = 20 (sigma 5), 128 KiB at r = 64.  Lanes
// of a wave read consecutive doubles in both passes (ds_read_b64, conflict-free); the weights
// come from the kernel arguments with a wave-uniform index (scalar loads).  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sm_rectify.hpp"  // bgr2gray

namespace smk {

constexpr int GF_TW = 64, GF_TH = 32;  // output tile: columns x rows
constexpr int GF_THREADS = 256;        // 64 columns x 4 groups of GF_ROWS rows
constexpr int GF_ROWS = GF_TH / (GF_THREADS / GF_TW);
constexpr int GF_CW = 64;              // columns staged per strip of the column pass
constexpr int GF_MAX_R = 64;           // largest half width: sigma < 16.125 at truncate 4

struct GaussArgs {
    const void* src;        // [img] H rows: float64, or uint8 BGR (k_gauss2d_f64<true, .>)
    double* dst;            // [img] H rows of dst_stride doubles
    size_t src_img_stride;  // doubles (bytes for BGR) between source images
    size_t dst_img_stride;  // doubles between destination images
    int H, W;
    int src_stride;         // doubles (bytes for BGR) between source rows
    int dst_stride;
    int ry, rx;
    double alpha;           // UNSHARP only
    double wy[GF_MAX_R + 1], wx[GF_MAX_R + 1];  // half kernels, centre first
};

inline size_t gauss_lds_bytes(int ry, int rx)
{
    return ((size_t)(GF_TH + 2 * ry) * GF_CW + (size_t)GF_TH * (GF_TW + 2 * rx)) * sizeof(double);
}

// scipy's 'reflect' (half-sample symmetric) of index k into [0, n): period 2 n, as often as needed
__device__ inline int gf_reflect(int k, int n)
{
    if ((unsigned)k < (unsigned)n) return k;
    const int p = 2 * n;
    k %= p;
    if (k < 0) k += p;
    return k < n ? k : p - 1 - k;
}

template <bool BGR, bool UNSHARP>
__global__ void __launch_bounds__(GF_THREADS) k_gauss2d_f64(GaussArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ double gf_lds[];
    const int ry = a.ry, rx = a.rx;
    const int SR = GF_TH + 2 * ry;  // staged source rows
    const int MW = GF_TW + 2 * rx;  // columns the column pass is needed on
    double* S = gf_lds;             // [SR][GF_CW]
    double* M = gf_lds + SR * GF_CW;  // [GF_TH][MW]
    const int tid = threadIdx.x, lx = tid & (GF_TW - 1), y0 = (tid / GF_TW) * GF_ROWS;
    const int gx0 = blockIdx.x * GF_TW - rx, gy0 = blockIdx.y * GF_TH - ry;
    const uint8_t* src8 = reinterpret_cast<const uint8_t*>(a.src) + (size_t)blockIdx.z * a.src_img_stride;
    const double* src = reinterpret_cast<const double*>(a.src) + (size_t)blockIdx.z * a.src_img_stride;

    for (int c0 = 0; c0 < MW; c0 += GF_CW) {
        const int cw = min(GF_CW, MW - c0);
        // ---- stage the strip's source rows, reflection resolved (lane = column: coalesced rows)
        if (lx < cw) {
            const int gx = gf_reflect(gx0 + c0 + lx, a.W);
            for (int ly = tid / GF_CW; ly < SR; ly += GF_THREADS / GF_CW) {
                const size_t row = (size_t)gf_reflect(gy0 + ly, a.H) * a.src_stride;
                double v;
                if (BGR) {
                    const uint8_t* p = src8 + row + 3 * (size_t)gx;
                    v = (double)bgr2gray(p[0], p[1], p[2]);
                } else {
                    v = src[row + gx];
                }
                S[ly * GF_CW + lx] = v;
            }
        }
        __syncthreads();
        // ---- axis 0: GF_ROWS rows of column c0 + lx
        if (lx < cw) {
            const double* p = S + (y0 + ry) * GF_CW + lx;
            double t[GF_ROWS];
            const double w0 = a.wy[0];
#pragma unroll
            for (int i = 0; i < GF_ROWS; ++i) t[i] = p[i * GF_CW] * w0;
            for (int j = ry; j >= 1; --j) {
                const double wj = a.wy[j];
#pragma unroll
                for (int i = 0; i < GF_ROWS; ++i) t[i] = t[i] + (p[(i - j) * GF_CW] + p[(i + j) * GF_CW]) * wj;
            }
#pragma unroll
            for (int i = 0; i < GF_ROWS; ++i) M[(y0 + i) * MW + c0 + lx] = t[i];
        }
        __syncthreads();  // M complete after the last strip; S free for the next one
    }

    // ---- axis 1: GF_ROWS rows of tile column lx
    const double* q = M + y0 * MW + rx + lx;
    double t[GF_ROWS];
    const double w0 = a.wx[0];
#pragma unroll
    for (int i = 0; i < GF_ROWS; ++i) t[i] = q[i * MW] * w0;
    for (int j = rx; j >= 1; --j) {
        const double wj = a.wx[j];
#pragma unroll
        for (int i = 0; i < GF_ROWS; ++i) t[i] = t[i] + (q[i * MW - j] + q[i * MW + j]) * wj;
    }
    const int gx = blockIdx.x * GF_TW + lx;
    if (gx >= a.W) return;
    double* dst = a.dst + (size_t)blockIdx.z * a.dst_img_stride;
#pragma unroll
    for (int i = 0; i < GF_ROWS; ++i) {
        const int gy = blockIdx.y * GF_TH + y0 + i;
        if (gy >= a.H) break;
        double v = t[i];
        if (UNSHARP) {  // image_measure: src + alpha * (src - blurred), three roundings
            const double s = src[(size_t)gy * a.src_stride + gx];
            const double d = s - v;
            const double e = a.alpha * d;
            v = s + e;
        }
        dst[(size_t)gy * a.dst_stride + gx] = v;
    }
}

// ---- pyrDown

struct PyrArgs {
    const uint8_t* src;  // [img] H rows of src_stride bytes, CN interleaved channels
    uint8_t* dst;        // [img] dH rows of dst_stride bytes
    size_t src_img_stride, dst_img_stride;  // bytes
    int H, W, dH, dW;
    int src_stride, dst_stride;
    int vec;             // every destination row 4-byte aligned: dword stores
};

// BORDER_REFLECT_101 of index p into [0, n) (cv::borderInterpolate's loop)
__device__ inline int pyr_reflect101(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// Each lane owns 4 adjacent bytes of a destination row (4 gray pixels, or 4 channel values of
// the interleaved BGR row); a row per blockIdx.y.  The five source rows are resolved once per
// lane; each byte is the 5 x 5 integer sum, rows first.
template <int CN>
__global__ void __launch_bounds__(256) k_pyr_down_u8(PyrArgs a)
{
    const int nb = a.dW * CN;  // bytes of a destination row
    const int b0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (b0 >= nb) return;
    const int y = blockIdx.y;
    const uint8_t* img = a.src + (size_t)blockIdx.z * a.src_img_stride;
    const uint8_t* rows[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) rows[i] = img + (size_t)pyr_reflect101(2 * y + i - 2, a.H) * a.src_stride;
    uint32_t out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = min(b0 + k, nb - 1);  // the tail's spare bytes repeat the last one (not stored)
        const int x = b / CN, c = b - x * CN;
        int s = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int o = pyr_reflect101(2 * x + j - 2, a.W) * CN + c;
            const int col = rows[0][o] + rows[4][o] + 4 * (rows[1][o] + rows[3][o]) + 6 * rows[2][o];
            s += (j == 0 || j == 4 ? 1 : j == 2 ? 6 : 4) * col;
        }
        out[k] = (uint32_t)(s + 128) >> 8;
    }
    uint8_t* d = a.dst + (size_t)blockIdx.z * a.dst_img_stride + (size_t)y * a.dst_stride + b0;
    if (a.vec && b0 + 4 <= nb) {
        *reinterpret_cast<uint32_t*>(d) = out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (b0 + k < nb) d[k] = (uint8_t)out[k];
    }
}

}  // namespace smk
