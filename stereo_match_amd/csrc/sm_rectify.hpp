// sm_rectify.hpp — the rectification front end on the GPU: the
// reference's rectify_opencv (disparity_calculation.py:131-210) and the two cvtColor
// calls after it (:286-287).
//   k_rectify_map  cv2.initUndistortRectifyMap(K, dist, R, P, size, CV_32FC1)
//   k_remap_u8     cv2.remap(src, mapx, mapy, INTER_LINEAR) on uint8, 1 or 3 channels,
//                  constant-0 border, with cvtColor(COLOR_BGR2GRAY) of the result fused in
//   k_bgr2gray     cvtColor(COLOR_BGR2GRAY) alone
// Semantics (version-scoped restatements; tests/rectify_np.py is the independent one):
//  map, per destination pixel (row i, column j), float64 with FP contraction off:
//   X = iR00*j + (iR01*i + iR02), Y and Wd likewise;  w = 1/Wd;  x = X*w;  y = Y*w
//   x2 = x*x; y2 = y*y; r2 = x2 + y2; xy2 = (2*x)*y;  kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
//   xd = x*kr + p1*xy2 + p2*(r2 + 2*x2);  yd = y*kr + p1*(r2 + 2*y2) + p2*xy2
//   mapx = (float)(fx*xd + cx);  mapy = (float)(fy*yd + cy)
//  remap, per pixel: a map value m with !(|m| < 2^24) gives 0; else s = rint(m*32) (half to
//   even), ix = s >> 5, f = s & 31 (5-bit fixed point); the four taps (ix,iy) (ix+1,iy)
//   (ix,iy+1) (ix+1,iy+1) read 0 outside the source; per channel
//   (a00*p00 + a01*p01 + a10*p10 + a11*p11 + 512) >> 10 with a00 = (32-fx)(32-fy) ... in int32
//  gray: (1868*B + 9617*G + 4899*R + 8192) >> 14 of the rounded uint8 BGR.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smk {

struct RectMapArgs {
    double iR[9];
    double k1, k2, p1, p2, k3;
    double fx, fy, cx, cy;
    float* mapx;  // [H][W]
    float* mapy;
    int H, W;
};

__global__ void __launch_bounds__(256) k_rectify_map(RectMapArgs a)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= a.W) return;
    const double* R = a.iR;
    const double X = R[0] * j + (R[1] * i + R[2]);
    const double Y = R[3] * j + (R[4] * i + R[5]);
    const double Wd = R[6] * j + (R[7] * i + R[8]);
    const double w = 1.0 / Wd;
    const double x = X * w, y = Y * w;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, xy2 = (2 * x) * y;
    const double kr = 1 + ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2;
    const double xd = x * kr + a.p1 * xy2 + a.p2 * (r2 + 2 * x2);
    const double yd = y * kr + a.p1 * (r2 + 2 * y2) + a.p2 * xy2;
    const size_t o = (size_t)i * a.W + j;
    a.mapx[o] = (float)(a.fx * xd + a.cx);
    a.mapy[o] = (float)(a.fy * yd + a.cy);
}

constexpr int REMAP_IPT = 4;  // images of a batch one thread serves with one read of its map values

struct RemapArgs {
    const uint8_t* src;  // [img] srcH rows of src_stride bytes, CN interleaved bytes per pixel
    const float* mapx;   // [H][W], shared by the batch
    const float* mapy;
    uint8_t* dst;        // [img][H][W][CN] or null
    uint8_t* gray;       // [img][H][W] or null (CN == 3)
    size_t img_stride;   // bytes between source images
    int nimg, srcH, srcW, src_stride, H, W;
    int Wq;              // quads per destination row: (W + 3) / 4
    int vec;             // W % 4 == 0 and every pointer aligned: 16-byte map loads, dword stores
};

// one destination pixel's taps: byte offset of (ix, iy) in the source image, the four
// weights, and which of the two columns / rows lie inside the source
struct RemapTap {
    long long off;
    int a00, a01, a10, a11;
    bool x0, x1, y0, y1;
};

__device__ inline RemapTap remap_tap(float mx, float my, int srcH, int srcW, int src_stride, int cn)
{
    RemapTap t;
    if (!(fabsf(mx) < 16777216.f) || !(fabsf(my) < 16777216.f)) {
        t.off = 0;
        t.a00 = t.a01 = t.a10 = t.a11 = 0;
        t.x0 = t.x1 = t.y0 = t.y1 = false;
        return t;
    }
    const int sx = (int)rintf(mx * 32.f), sy = (int)rintf(my * 32.f);
    const int ix = sx >> 5, iy = sy >> 5, fx = sx & 31, fy = sy & 31;
    t.a00 = (32 - fx) * (32 - fy);
    t.a01 = fx * (32 - fy);
    t.a10 = (32 - fx) * fy;
    t.a11 = fx * fy;
    t.x0 = ix >= 0 && ix < srcW;
    t.x1 = ix + 1 >= 0 && ix + 1 < srcW;
    t.y0 = iy >= 0 && iy < srcH;
    t.y1 = iy + 1 >= 0 && iy + 1 < srcH;
    t.off = (long long)iy * src_stride + (long long)ix * cn;  // dereferenced only where the tap is inside
    return t;
}

__device__ inline int remap_blend(const uint8_t* s, const RemapTap& t, int src_stride, int cn, int c)
{
    const uint8_t* p = s + t.off + c;
    const int p00 = (t.x0 && t.y0) ? p[0] : 0;
    const int p01 = (t.x1 && t.y0) ? p[cn] : 0;
    const int p10 = (t.x0 && t.y1) ? p[src_stride] : 0;
    const int p11 = (t.x1 && t.y1) ? p[src_stride + cn] : 0;
    return (t.a00 * p00 + t.a01 * p01 + t.a10 * p10 + t.a11 * p11 + 512) >> 10;
}

__device__ inline int bgr2gray(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

// Each lane owns 4 horizontally adjacent destination pixels (a wave: 256 consecutive pixels
// of the flattened [row][quad] order, one row's unless it wraps), computes their taps once
// and serves up to REMAP_IPT images of the batch with them.
template <int CN, bool GRAY>
__global__ void __launch_bounds__(256) k_remap_u8(RemapArgs a)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.H * a.Wq) return;
    const int row = q / a.Wq, x0 = (q - row * a.Wq) * 4;
    const size_t px = (size_t)row * a.W + x0;
    float mx[4], my[4];
    if (a.vec) {
        const float4 vx = *reinterpret_cast<const float4*>(a.mapx + px);
        const float4 vy = *reinterpret_cast<const float4*>(a.mapy + px);
        mx[0] = vx.x, mx[1] = vx.y, mx[2] = vx.z, mx[3] = vx.w;
        my[0] = vy.x, my[1] = vy.y, my[2] = vy.z, my[3] = vy.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = x0 + k < a.W;
            mx[k] = in ? a.mapx[px + k] : 0.f;
            my[k] = in ? a.mapy[px + k] : 0.f;
        }
    }
    RemapTap t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = remap_tap(mx[k], my[k], a.srcH, a.srcW, a.src_stride, CN);

    const size_t npx = (size_t)a.H * a.W;
    const int img0 = blockIdx.y * REMAP_IPT;
    for (int img = img0; img < img0 + REMAP_IPT && img < a.nimg; ++img) {
        const uint8_t* s = a.src + (size_t)img * a.img_stride;
        uint8_t v[4][CN];
        uint8_t g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < CN; ++c) v[k][c] = (uint8_t)remap_blend(s, t[k], a.src_stride, CN, c);
            if (GRAY) g[k] = (uint8_t)bgr2gray(v[k][0], v[k][CN > 1 ? 1 : 0], v[k][CN > 2 ? 2 : 0]);
        }
        if (a.vec) {
            if (GRAY && a.gray)
                *reinterpret_cast<uint32_t*>(a.gray + img * npx + px) =
                    (uint32_t)g[0] | (uint32_t)g[1] << 8 | (uint32_t)g[2] << 16 | (uint32_t)g[3] << 24;
            if (a.dst) {
                uint32_t* d = reinterpret_cast<uint32_t*>(a.dst + (img * npx + px) * CN);
                const uint8_t* b = &v[0][0];
#pragma unroll
                for (int wd = 0; wd < CN; ++wd)
                    d[wd] = (uint32_t)b[4 * wd] | (uint32_t)b[4 * wd + 1] << 8 | (uint32_t)b[4 * wd + 2] << 16 |
                            (uint32_t)b[4 * wd + 3] << 24;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (x0 + k >= a.W) break;
                if (GRAY && a.gray) a.gray[img * npx + px + k] = g[k];
                if (a.dst) {
#pragma unroll
                    for (int c = 0; c < CN; ++c) a.dst[(img * npx + px + k) * CN + c] = v[k][c];
                }
            }
        }
    }
}

struct GrayArgs {
    const uint8_t* src;  // [img] H rows of src_stride bytes, BGR
    uint8_t* gray;       // [img][H][W]
    size_t img_stride;
    int H, W, src_stride;
};

__global__ void __launch_bounds__(256) k_bgr2gray(GrayArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, img = blockIdx.z;
    if (x >= a.W) return;
    const uint8_t* p = a.src + (size_t)img * a.img_stride + (size_t)y * a.src_stride + 3 * (size_t)x;
    a.gray[((size_t)img * a.H + y) * a.W + x] = (uint8_t)bgr2gray(p[0], p[1], p[2]);
}

}  // namespace smk
