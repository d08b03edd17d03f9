// sm_mccnn.hpp — the MC-CNN *fast* matching cost (Žbontar & LeCun): two gray images to a
// float32 cost volume, on the device and as a plain C++ twin.
//
//   normalise   per image (x - mean) / std, std the unbiased one.  From the exact integer sums
//               Sx, Sxx over the N pixels:  q = N Sxx - Sx^2  (exact, N < 2^24),
//               std = sqrt(double(q) / double(N (N - 1))),
//               value(g) = float((double(g N - Sx) / double(N)) / std)  for the 256 grey levels:
//               conversions, divisions and one square root only, so nothing can be contracted
//               and one table of 256 floats serves host and device.  q == 0: a constant image.
//   layer i     L convolutions 3x3, zero padding 1, 64 feature maps, ReLU after all but the last.
//               out[co] = chain over k of fmaf(in[tap, ci], w[co, ci, tap], acc), acc = b[co],
//               k = tap * Cin + ci: tap-major (ky, then kx), channel-minor.  A padded tap
//               contributes fmaf(0, w, acc).  ReLU is v > 0 ? v : +0.
//   unit norm   s = chain of fmaf(f_c, f_c, s) from 0, c = 0..63; f_c / sqrtf(s), both correctly
//               rounded; s == 0 gives 64 zeros (this package's rule).
//   join        plane d at (y, x) = -(chain of fmaf(A_c, B_c, s) from 0, c = 0..63) with B at
//               x - (m + d); NaN where that column lies outside [0, W).
//
// Feature maps are channel-last [H][W][64] float32.  Layers 1.. run as implicit GEMMs on the
// f32-input matrix instruction 32x32x2 (M = 8 x 32 pixels per workgroup, N = 64, K = 576),
// whose result is bit for bit the k-ordered fmaf chain, so the chain order above is the contract
// between the kernels and the twin.  The packed weights (mc_pack_*) are what the kernels stage:
// layer 0 [tap][co]; layers 1.. [tap][ci][co ^ 32 (ci & 1)], the LDS image of one tap per 16 KB
// (the swizzle keeps the two k rows an instruction reads in different banks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace smk {

constexpr int MC_C = 64;          // feature maps of every layer
constexpr int MC_MAXL = 6;        // layers
constexpr int MC_MAXD = 256;      // planes of a volume
constexpr int MC_W0 = 9 * MC_C;   // packed floats of layer 0
constexpr int MC_TAP = MC_C * MC_C;  // packed floats of one tap of a later layer
constexpr int MC_WL = 9 * MC_TAP;    // packed floats of a later layer
constexpr size_t MC_MAXPIX = (size_t(1) << 24) - 1;  // N Sxx and Sx^2 stay below 2^64

inline size_t mc_pack_floats(int L) { return (size_t)MC_W0 + (size_t)(L - 1) * MC_WL; }

// w[0] is [64][1][3][3], w[i] is [64][64][3][3]; dst holds mc_pack_floats(L)
inline void mc_pack_weights(int L, const float* const* w, float* dst)
{
    for (int tap = 0; tap < 9; tap++)
        for (int co = 0; co < MC_C; co++) dst[tap * MC_C + co] = w[0][co * 9 + tap];
    for (int i = 1; i < L; i++) {
        float* p = dst + MC_W0 + (size_t)(i - 1) * MC_WL;
        for (int tap = 0; tap < 9; tap++)
            for (int ci = 0; ci < MC_C; ci++)
                for (int co = 0; co < MC_C; co++)
                    p[tap * MC_TAP + ci * MC_C + (co ^ (32 * (ci & 1)))] = w[i][((size_t)co * MC_C + ci) * 9 + tap];
    }
}

// the 256 normalised grey levels of an image with sums sx, sxx over npix pixels; false: constant
inline bool mc_table(uint64_t sx, uint64_t sxx, uint64_t npix, float* tab)
{
    const uint64_t q = npix * sxx - sx * sx;
    if (q == 0) return false;
    const double sd = std::sqrt((double)q / (double)(npix * (npix - 1)));
    for (int g = 0; g < 256; g++) {
        const int64_t num = (int64_t)((uint64_t)g * npix) - (int64_t)sx;
        tab[g] = (float)(((double)num / (double)npix) / sd);
    }
    return true;
}

// ---- the twin: plain loops, explicit fmaf.  The same body is built twice, once for CPUs with
// FMA units (the loops over co vectorise) and once for any x86-64 (libm's fmaf): both are the
// exact fused operation.
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define SM_MC_FMA_TARGET __attribute__((target("avx2,fma")))
#else
#define SM_MC_FMA_TARGET
#endif

__attribute__((always_inline)) inline void mc_conv_pixel_host(const float* in, int cin, int H, int W, int y, int x,
                                                              const float* wp, const float* b, bool relu, float* out)
{
    float acc[MC_C];
    for (int co = 0; co < MC_C; co++) acc[co] = b[co];
    for (int tap = 0; tap < 9; tap++) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float* px = inside ? in + ((size_t)yy * W + xx) * cin : nullptr;
        for (int ci = 0; ci < cin; ci++) {
            const float v = inside ? px[ci] : 0.0f;
            const float* wr = wp + ((size_t)tap * cin + ci) * MC_C;
            const int sw = cin == 1 ? 0 : 32 * (ci & 1);
            if (sw)
                for (int co = 0; co < MC_C; co++) acc[co] = __builtin_fmaf(v, wr[co ^ 32], acc[co]);
            else
                for (int co = 0; co < MC_C; co++) acc[co] = __builtin_fmaf(v, wr[co], acc[co]);
        }
    }
    for (int co = 0; co < MC_C; co++) out[co] = relu ? (acc[co] > 0.0f ? acc[co] : 0.0f) : acc[co];
}

__attribute__((always_inline)) inline void mc_unit_host(float* f)
{
    float s = 0.0f;
    for (int c = 0; c < MC_C; c++) s = __builtin_fmaf(f[c], f[c], s);
    const float r = std::sqrt(s);
    for (int c = 0; c < MC_C; c++) f[c] = s == 0.0f ? 0.0f : f[c] / r;
}

__attribute__((always_inline)) inline void mc_features_image_body(int L, const float* wp, const float* bias,
                                                                  const float* plane, int H, int W, float* ping,
                                                                  float* pong, float* feat)
{
    const float* in = plane;
    for (int i = 0; i < L; i++) {
        float* out = i == L - 1 ? feat : (i & 1) ? pong : ping;
        const float* w = i == 0 ? wp : wp + MC_W0 + (size_t)(i - 1) * MC_WL;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                float* o = out + ((size_t)y * W + x) * MC_C;
                mc_conv_pixel_host(in, i == 0 ? 1 : MC_C, H, W, y, x, w, bias + i * MC_C, i < L - 1, o);
                if (i == L - 1) mc_unit_host(o);
            }
        in = out;
    }
}

__attribute__((always_inline)) inline void mc_join_body(const float* fa, const float* fb, int H, int W, int D,
                                                        long long m, float* vol)
{
    for (int d = 0; d < D; d++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const long long xb = (long long)x - (m + d);
                float v = std::nanf("");
                if (xb >= 0 && xb < W) {
                    const float* a = fa + ((size_t)y * W + x) * MC_C;
                    const float* b = fb + ((size_t)y * W + (size_t)xb) * MC_C;
                    float s = 0.0f;
                    for (int c = 0; c < MC_C; c++) s = __builtin_fmaf(a[c], b[c], s);
                    v = -s;
                }
                vol[((size_t)d * H + y) * W + x] = v;
            }
}

SM_MC_FMA_TARGET inline void mc_features_image_fma(int L, const float* wp, const float* bias, const float* plane, int H,
                                                   int W, float* ping, float* pong, float* feat)
{
    mc_features_image_body(L, wp, bias, plane, H, W, ping, pong, feat);
}
inline void mc_features_image_any(int L, const float* wp, const float* bias, const float* plane, int H, int W,
                                  float* ping, float* pong, float* feat)
{
    mc_features_image_body(L, wp, bias, plane, H, W, ping, pong, feat);
}
SM_MC_FMA_TARGET inline void mc_join_fma(const float* fa, const float* fb, int H, int W, int D, long long m, float* vol)
{
    mc_join_body(fa, fb, H, W, D, m, vol);
}
inline void mc_join_any(const float* fa, const float* fb, int H, int W, int D, long long m, float* vol)
{
    mc_join_body(fa, fb, H, W, D, m, vol);
}

inline bool mc_cpu_has_fma()
{
#if defined(__x86_64__)
    return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
#else
    return false;
#endif
}

// features of n images (rows row_stride, images image_stride bytes apart) into feat [n][H][W][64];
// wp / bias: the packed weights and the L x 64 biases.  Returns the index of the first constant
// image, or -1 when all went well.
inline int mccnn_features_host(int L, const float* wp, const float* bias, const uint8_t* gray, int n, size_t image_stride,
                               int H, int W, size_t row_stride, float* feat)
{
    const size_t npix = (size_t)H * W;
    std::vector<float> plane(npix), ping(L > 1 ? npix * MC_C : 0), pong(L > 2 ? npix * MC_C : 0);
    const bool fma = mc_cpu_has_fma();
    for (int img = 0; img < n; img++) {
        const uint8_t* g = gray + (size_t)img * image_stride;
        uint64_t sx = 0, sxx = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const uint64_t v = g[(size_t)y * row_stride + x];
                sx += v, sxx += v * v;
            }
        float tab[256];
        if (!mc_table(sx, sxx, npix, tab)) return img;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) plane[(size_t)y * W + x] = tab[g[(size_t)y * row_stride + x]];
        float* f = feat + (size_t)img * npix * MC_C;
        if (fma)
            mc_features_image_fma(L, wp, bias, plane.data(), H, W, ping.data(), pong.data(), f);
        else
            mc_features_image_any(L, wp, bias, plane.data(), H, W, ping.data(), pong.data(), f);
    }
    return -1;
}

// a column offset beyond these bounds leaves every cell NaN, as the bound itself does
inline int mc_clamp_min_disparity(long long m, int W, int D)
{
    const long long lo = -((long long)W + D), hi = W;
    return (int)(m < lo ? lo : m > hi ? hi : m);
}

inline void mccnn_join_host(const float* fa, const float* fb, int n, int H, int W, int D, int minD, float* vol)
{
    const size_t fimg = (size_t)H * W * MC_C, vimg = (size_t)D * H * W;
    const int m = mc_clamp_min_disparity(minD, W, D);
    const bool fma = mc_cpu_has_fma();
    for (int img = 0; img < n; img++) {
        if (fma)
            mc_join_fma(fa + img * fimg, fb + img * fimg, H, W, D, m, vol + img * vimg);
        else
            mc_join_any(fa + img * fimg, fb + img * fimg, H, W, D, m, vol + img * vimg);
    }
}

#if defined(__HIPCC__) && !defined(SM_MCCNN_NO_KERNELS)  // sm_mcsgm.hpp's unit takes the host functions only
// ---- kernels

constexpr int MC_BLOCK = 256;
constexpr int MC_TW = 32, MC_TH = 8;                  // the pixel tile of a convolution workgroup
constexpr int MC_HW = MC_TW + 2, MC_HH = MC_TH + 2;   // with its halo
constexpr int MC_PS = 66;                             // floats between the pixels of the LDS tile (banks 2 i + c)
constexpr int MC_JX = 128, MC_JD = 64;                // join: columns per workgroup, planes per staged chunk
constexpr int MC_JS = 68;                             // floats between the pixels of the join's LDS row

typedef float mc_f16 __attribute__((ext_vector_type(16)));

struct McSumArgs {
    const uint8_t* gray;
    size_t image_stride, row_stride;
    int H, W;
    unsigned long long* sums;  // [img][2]: Sx, Sxx (zeroed before the launch)
};

// exact integer sums of every image: blockIdx.y the image, the blocks stride over its pixels
__global__ __launch_bounds__(MC_BLOCK) void k_mc_sums(McSumArgs a)
{
    const uint8_t* g = a.gray + (size_t)blockIdx.y * a.image_stride;
    const unsigned npix = (unsigned)a.H * (unsigned)a.W;
    unsigned long long sx = 0, sxx = 0;
    for (unsigned i = blockIdx.x * MC_BLOCK + threadIdx.x; i < npix; i += gridDim.x * MC_BLOCK) {
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

struct McL0Args {
    const uint8_t* gray;  // one image
    size_t row_stride;
    int H, W;
    const float* tab;     // its 256 normalised grey levels
    const float* w;       // [tap][co]
    const float* b;
    float* out;           // [H][W][64]
    int relu;
};

// layer 0 (K = 9) on the VALU: a thread computes 4 feature maps of a pixel
__global__ __launch_bounds__(MC_BLOCK) void k_mc_layer0(McL0Args a)
{
    __shared__ float tab[256];
    tab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();
    const unsigned idx = blockIdx.x * MC_BLOCK + threadIdx.x;
    const unsigned pix = idx >> 4, q = idx & 15;
    if (pix >= (unsigned)a.H * (unsigned)a.W) return;
    const int y = (int)(pix / (unsigned)a.W), x = (int)(pix - (unsigned)y * (unsigned)a.W);
    const float4 bb = *(const float4*)(a.b + 4 * q);
    float acc[4] = {bb.x, bb.y, bb.z, bb.w};
    for (int tap = 0; tap < 9; tap++) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        float v = 0.0f;
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) v = tab[a.gray[(size_t)yy * a.row_stride + xx]];
        const float4 w = *(const float4*)(a.w + tap * MC_C + 4 * q);
        acc[0] = __builtin_fmaf(v, w.x, acc[0]);
        acc[1] = __builtin_fmaf(v, w.y, acc[1]);
        acc[2] = __builtin_fmaf(v, w.z, acc[2]);
        acc[3] = __builtin_fmaf(v, w.w, acc[3]);
    }
    if (a.relu)
        for (int j = 0; j < 4; j++) acc[j] = acc[j] > 0.0f ? acc[j] : 0.0f;
    *(float4*)(a.out + (size_t)pix * MC_C + 4 * q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

struct McUnitArgs {
    float* f;  // [npix][64], in place
    unsigned npix;
};

// the unit-norm step on its own (a one-layer network; later layers normalise in their epilogue)
__global__ __launch_bounds__(MC_BLOCK) void k_mc_unit(McUnitArgs a)
{
    const unsigned pix = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (pix >= a.npix) return;
    float* f = a.f + (size_t)pix * MC_C;
    float s = 0.0f;
    for (int c = 0; c < MC_C; c++) s = __builtin_fmaf(f[c], f[c], s);
    const float r = __builtin_sqrtf(s);
    for (int c = 0; c < MC_C; c++) f[c] = s == 0.0f ? 0.0f : (f[c] / r);
}

struct McConvArgs {
    const float* in;  // [H][W][64]
    float* out;       // [H][W][64]
    const float* w;   // [tap][ci][co ^ 32 (ci & 1)]
    const float* b;
    int H, W;
};

// One 3x3, 64 -> 64 layer as an implicit GEMM on mfma_f32_32x32x2f32.  A workgroup: 8 rows x 32
// columns of pixels, its 10 x 34 halo tile in LDS (zeros outside the image) and one tap's
// weights at a time, double-buffered.  A wave: two rows (two M tiles of 32 pixels) x the two
// halves of the 64 outputs = four independent accumulators.  An instruction's A operand is
// in[pixel lane & 31][ci = 2 s + (lane >> 5)], its B operand w[ci][co = lane & 31 (+ 32)]; it
// adds k = 2 s, then k = 2 s + 1, so 32 of them per tap over the nine taps are the chain.  The
// accumulators start at the bias.  LAST: no ReLU; the tile goes back through LDS, a thread per
// pixel runs the norm chain, and all write f / sqrt(s).
template <bool LAST>
__global__ __launch_bounds__(MC_BLOCK) void k_mc_conv(McConvArgs a)
{
    __shared__ float tile[MC_HH * MC_HW * MC_PS];
    __shared__ float wbuf[2][MC_TAP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int x0 = blockIdx.x * MC_TW, y0 = blockIdx.y * MC_TH;

    for (int i = tid; i < MC_HH * MC_HW * 16; i += MC_BLOCK) {
        const int p = i >> 4, q = i & 15;
        const int ty = p / MC_HW, tx = p - ty * MC_HW;
        const int gy = y0 + ty - 1, gx = x0 + tx - 1;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = *(const float4*)(a.in + ((size_t)gy * a.W + gx) * MC_C + 4 * q);
        float2* t = (float2*)(tile + p * MC_PS + 4 * q);
        t[0] = make_float2(v.x, v.y);
        t[1] = make_float2(v.z, v.w);
    }
    for (int i = tid; i < MC_TAP / 4; i += MC_BLOCK) ((float4*)wbuf[0])[i] = ((const float4*)a.w)[i];

    mc_f16 acc[2][2];
    for (int n = 0; n < 2; n++) {
        const float bv = a.b[j + 32 * n];
        for (int m = 0; m < 2; m++)
            for (int r = 0; r < 16; r++) acc[m][n][r] = bv;
    }
    __syncthreads();

    for (int tap = 0; tap < 9; tap++) {
        float4 nxt[MC_TAP / 4 / MC_BLOCK];
        if (tap + 1 < 9)
            for (int i = 0; i < MC_TAP / 4 / MC_BLOCK; i++)
                nxt[i] = ((const float4*)(a.w + (size_t)(tap + 1) * MC_TAP))[tid + i * MC_BLOCK];
        const float* wb = wbuf[tap & 1];
        const int ky = tap / 3, kx = tap - 3 * ky;
        const float* a0 = tile + ((2 * wv + ky) * MC_HW + j + kx) * MC_PS + h;
        const float* a1 = a0 + MC_HW * MC_PS;
        const float* b0 = wb + h * MC_C + (j ^ (32 * h));  // co = j of row ci = 2 s + h (swizzled by ci & 1 = h)
        const float* b1 = wb + h * MC_C + (j ^ (32 * h) ^ 32);  // co = j + 32
#pragma unroll 8
        for (int s = 0; s < 32; s++) {
            const float av0 = a0[2 * s], av1 = a1[2 * s];
            const float bv0 = b0[2 * s * MC_C], bv1 = b1[2 * s * MC_C];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv1, acc[1][1], 0, 0, 0);
        }
        if (tap + 1 < 9)
            for (int i = 0; i < MC_TAP / 4 / MC_BLOCK; i++) ((float4*)wbuf[(tap + 1) & 1])[tid + i * MC_BLOCK] = nxt[i];
        __syncthreads();
    }

    // C/D: column (co) = lane & 31, row (pixel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if (!LAST) {
        for (int m = 0; m < 2; m++) {
            const int gy = y0 + 2 * wv + m;
            if (gy >= a.H) continue;
            for (int r = 0; r < 16; r++) {
                const int gx = x0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (gx >= a.W) continue;
                float* o = a.out + ((size_t)gy * a.W + gx) * MC_C + j;
                for (int n = 0; n < 2; n++) {
                    const float v = acc[m][n][r];
                    o[32 * n] = v > 0.0f ? v : 0.0f;
                }
            }
        }
    } else {
        // every wave is past its last read of the tile (the barrier that ended tap 8)
        for (int m = 0; m < 2; m++)
            for (int r = 0; r < 16; r++) {
                const int p = (2 * wv + m) * MC_TW + (r & 3) + 8 * (r >> 2) + 4 * h;
                for (int n = 0; n < 2; n++) tile[p * MC_PS + j + 32 * n] = acc[m][n][r];
            }
        __syncthreads();
        {
            const float* f = tile + tid * MC_PS;
            float s = 0.0f;
            for (int c = 0; c < MC_C; c++) s = __builtin_fmaf(f[c], f[c], s);
            tile[tid * MC_PS + MC_C] = s;
        }
        __syncthreads();
        for (int i = tid; i < MC_TH * MC_TW * 16; i += MC_BLOCK) {
            const int p = i >> 4, q = i & 15;
            const int gy = y0 + p / MC_TW, gx = x0 + p % MC_TW;
            if (gy >= a.H || gx >= a.W) continue;
            const float* f = tile + p * MC_PS + 4 * q;
            const float s = tile[p * MC_PS + MC_C];
            const float r = __builtin_sqrtf(s);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s != 0.0f) v = make_float4((f[0] / r), (f[1] / r), (f[2] / r), (f[3] / r));
            *(float4*)(a.out + ((size_t)gy * a.W + gx) * MC_C + 4 * q) = v;
        }
    }
}

struct McJoinArgs {
    const float* fa;  // [n][H][W][64]
    const float* fb;
    float* vol;       // [n][D][H][W]
    int H, W, D, m;   // m clamped (mc_clamp_min_disparity)
};

// The join: grid (column tiles of 128, H, n).  A thread keeps A[y][x][0..63] in registers; B's
// row segment of a chunk of 64 planes sits in LDS (68-float pixel stride: 16-byte reads of 16
// lanes hit 64 different banks); every plane's store is a full-width row segment.
__global__ __launch_bounds__(MC_JX) void k_mc_join(McJoinArgs a)
{
    __shared__ float sb[(MC_JX + MC_JD - 1) * MC_JS];
    const int tid = threadIdx.x, y = blockIdx.y, x0 = blockIdx.x * MC_JX, x = x0 + tid;
    const size_t row = ((size_t)blockIdx.z * a.H + y) * a.W;
    float av[MC_C];
    if (x < a.W) {
        const float4* p = (const float4*)(a.fa + (row + x) * MC_C);
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const float4 v = p[q];
            av[4 * q] = v.x, av[4 * q + 1] = v.y, av[4 * q + 2] = v.z, av[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < MC_C; c++) av[c] = 0.0f;
    }
    float* vol = a.vol + (size_t)blockIdx.z * a.D * a.H * a.W + (size_t)y * a.W;
    const size_t plane = (size_t)a.H * a.W;
    for (int d0 = 0; d0 < a.D; d0 += MC_JD) {
        const int xb_lo = x0 - (a.m + d0 + MC_JD - 1);  // local pixel 0; the thread's pixel for plane d0 + dd is tid + 63 - dd
        __syncthreads();
        for (int i = tid; i < (MC_JX + MC_JD - 1) * 16; i += MC_JX) {
            const int p = i >> 4, q = i & 15, xb = xb_lo + p;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (xb >= 0 && xb < a.W) v = *(const float4*)(a.fb + (row + xb) * MC_C + 4 * q);
            *(float4*)(sb + p * MC_JS + 4 * q) = v;
        }
        __syncthreads();
        const int nd = min(MC_JD, a.D - d0);
        for (int dd = 0; dd < nd; dd++) {
            const float4* b = (const float4*)(sb + (tid + MC_JD - 1 - dd) * MC_JS);
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const float4 v = b[q];
                s = __builtin_fmaf(av[4 * q], v.x, s);
                s = __builtin_fmaf(av[4 * q + 1], v.y, s);
                s = __builtin_fmaf(av[4 * q + 2], v.z, s);
                s = __builtin_fmaf(av[4 * q + 3], v.w, s);
            }
            const int xb = x - (a.m + d0 + dd);
            if (x < a.W) vol[(size_t)(d0 + dd) * plane + x] = (xb >= 0 && xb < a.W) ? -s : __builtin_nanf("");
        }
    }
}
#endif  // __HIPCC__ && !SM_MCCNN_NO_KERNELS

}  // namespace smk
