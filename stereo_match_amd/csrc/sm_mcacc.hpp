// sm_mcacc.hpp — the MC-CNN *accurate* matching cost (Žbontar & LeCun, §3.2): two gray images to a
// float32 cost volume through a 112-map feature net and a fully connected scorer, on the device and
// as a plain C++ twin.
//
//   normalise   sm_mccnn.hpp's grey-level table (mc_table), unchanged.
//   layer i     L convolutions 3x3, zero padding 1, 112 feature maps, ReLU after every one, no
//               unit-length step.  out[co] = chain over k of fmaf(in[tap, ci], w[co, ci, tap], acc),
//               acc = b[co], k = tap * Cin + ci ascending; a padded tap contributes fmaf(0, w, acc).
//   projection  the scorer's first layer, split so that its work is per pixel:
//               PL[p][u] = chain from fb0[u] of fmaf(fL[p][c], fw0[u][c], .), c = 0..111
//               PR[p][u] = chain from 0      of fmaf(fR[p][c], fw0[u][112 + c], .)
//   cell        left column xl against right column xr of row y:
//               h1[u] = relu(PL[y, xl, u] + PR[y, xr, u])                       (one float add)
//               h_i[u] = relu(chain from fb_i[u] of fmaf(h_{i-1}[k], fw_i[u][k], .)), i = 1..F-1
//               z = chain from fb_F[0] of fmaf(h_{F-1}[k], fw_F[0][k], .)
//   volume      plane d at (y, x) = -ac_sigmoid(z) (raw: -z) for a's column x against b's column
//               x - (m + d); NaN where that column lies outside [0, W).
//
// Every chain is one fmaf chain in ascending k: the f32 matrix instruction 32x32x2 is bit for bit
// that chain, so there is no split-K anywhere.  Packed weights: layer 0 [tap][112]; layers 1..
// [k][128] (k = tap * 112 + ci, the 16 maps past 111 are zeros and their outputs are dropped);
// biases [L][128]; the scorer transposed to [k][u] (ac_pack_fc).
#pragma once
// the grey-level table, the offset clamp and the FMA dispatch of the fast net; its kernels belong to
// sm_api_mccnn.hip's unit alone
#ifndef SM_MCCNN_NO_KERNELS
#define SM_MCCNN_NO_KERNELS
#endif
#include "sm_mccnn.hpp"

#pragma clang fp contract(off)

namespace smk {

constexpr int AC_C = 112;         // feature maps of every layer
constexpr int AC_CP = 128;        // padded to whole 32-column blocks of the matrix instruction
constexpr int AC_MAXL = 6;        // convolutions
constexpr int AC_MAXF = 4;        // hidden fully connected layers
constexpr int AC_MAXU = 384;      // units of a hidden layer (a multiple of 32)
constexpr int AC_W0 = 9 * AC_C;   // packed floats of layer 0
constexpr int AC_WL = 9 * AC_C * AC_CP;  // packed floats of a later layer

inline size_t ac_pack_conv_floats(int L) { return (size_t)AC_W0 + (size_t)(L - 1) * AC_WL; }

// w[0] is [112][1][3][3], w[i] is [112][112][3][3], b[i] is [112]; wp holds ac_pack_conv_floats(L),
// bp holds L * 128
inline void ac_pack_conv(int L, const float* const* w, const float* const* b, float* wp, float* bp)
{
    for (int tap = 0; tap < 9; tap++)
        for (int co = 0; co < AC_C; co++) wp[tap * AC_C + co] = w[0][co * 9 + tap];
    for (int i = 1; i < L; i++) {
        float* p = wp + AC_W0 + (size_t)(i - 1) * AC_WL;
        for (int tap = 0; tap < 9; tap++)
            for (int ci = 0; ci < AC_C; ci++)
                for (int co = 0; co < AC_CP; co++)
                    p[((size_t)tap * AC_C + ci) * AC_CP + co] = co < AC_C ? w[i][((size_t)co * AC_C + ci) * 9 + tap] : 0.0f;
    }
    for (int i = 0; i < L; i++)
        for (int co = 0; co < AC_CP; co++) bp[i * AC_CP + co] = co < AC_C ? b[i][co] : 0.0f;
}

// The packed scorer: [112][U] left half of fw0, [112][U] right half, F - 1 matrices [U][U]
// (all [k][u]), the last unit's [U], then the biases fb_0 .. fb_{F-1} ([U] each) and fb_F.
struct AcFc {
    int F = 0, U = 0;
    size_t pl() const { return 0; }
    size_t pr() const { return (size_t)AC_C * U; }
    size_t hid(int i) const { return (size_t)2 * AC_C * U + (size_t)(i - 1) * U * U; }  // i = 1 .. F - 1
    size_t last() const { return hid(F); }
    size_t bias(int i) const { return last() + U + (size_t)i * U; }  // i = 0 .. F (fb_F is one float)
    size_t floats() const { return bias(F) + 1; }
};

// fw[0] [U][224], fw[1..F-1] [U][U], fw[F] [1][U]; fb[i] [U], fb[F] [1]
inline void ac_pack_fc(const AcFc& fc, const float* const* fw, const float* const* fb, float* dst)
{
    const int U = fc.U, F = fc.F;
    for (int c = 0; c < AC_C; c++)
        for (int u = 0; u < U; u++) {
            dst[fc.pl() + (size_t)c * U + u] = fw[0][(size_t)u * 2 * AC_C + c];
            dst[fc.pr() + (size_t)c * U + u] = fw[0][(size_t)u * 2 * AC_C + AC_C + c];
        }
    for (int i = 1; i < F; i++)
        for (int k = 0; k < U; k++)
            for (int u = 0; u < U; u++) dst[fc.hid(i) + (size_t)k * U + u] = fw[i][(size_t)u * U + k];
    for (int k = 0; k < U; k++) dst[fc.last() + k] = fw[F][k];
    for (int i = 0; i < F; i++)
        for (int u = 0; u < U; u++) dst[fc.bias(i) + u] = fb[i][u];
    dst[fc.bias(F)] = fb[F][0];
}

// ---- the sigmoid: fmaf, float / int conversions, bit operations, comparisons and one correctly
// rounded divide; no library call, so host and device cannot differ.
//   NaN -> NaN.  t = -z clamped to [-80, 80]; n = trunc(t log2(e) +- 1/2); r = t - n ln 2 in two
//   fmaf steps (Cody-Waite, ln 2 = 0.693359375 - 2.12194440e-4); exp(r) = 1 + r + r^2 p(r), p the
//   degree-5 polynomial of Cephes' expf; e = exp(r) 2^n by adding n to the exponent field (the
//   result is normal for |t| <= 80); s = 1 / (1 + e).
//   s(+-0) = 0.5; s(z >= 80) = s(+inf) = 1; s(z <= -80) = s(-inf) = s(-80) = 1.8e-35, not 0.
__host__ __device__ inline float ac_sigmoid(float z)
{
    if (!(z == z)) return z;
    float t = -z;
    t = t < -80.0f ? -80.0f : t;
    t = t > 80.0f ? 80.0f : t;
    uint32_t tb, hb = 0x3F000000u;
    __builtin_memcpy(&tb, &t, 4);
    hb |= tb & 0x80000000u;
    float half;
    __builtin_memcpy(&half, &hb, 4);
    const int n = (int)__builtin_fmaf(t, 1.44269504088896341f, half);
    const float nf = (float)n;
    float r = __builtin_fmaf(nf, -0.693359375f, t);
    r = __builtin_fmaf(nf, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float r2 = __builtin_fmaf(r, r, 0.0f);
    float e = __builtin_fmaf(p, r2, r);
    e = __builtin_fmaf(e, 1.0f, 1.0f);
    uint32_t eb;
    __builtin_memcpy(&eb, &e, 4);
    eb += (uint32_t)n << 23;
    __builtin_memcpy(&e, &eb, 4);
    return 1.0f / __builtin_fmaf(e, 1.0f, 1.0f);
}

// ---- precision "bf16" (DESIGN.md §4.21): only the scorer's hidden layers 1 .. F-1 change.
//   ac_bf16(x)  the upper 16 bits of x rounded to nearest, ties to even; subnormals the same way (no
//               flush); +-inf kept; a finite value past bf16's largest becomes +-inf; a NaN becomes
//               a quiet NaN with its sign.  bf(x) = ac_bf16_float(ac_bf16(x)).
//   h1          as above, in f32 (the feature net and the projections PL / PR do not change).
//   h_i[u]      relu(fb_i[u] + sum over k of bf(h_{i-1}[k]) * bf(fw_i[u][k])), i = 1 .. F-1: every
//               product is exact in f32, the sum is accumulated in f32 from the f32 bias, h_i stays
//               f32 until it is rounded as the next layer's operand.  Twin: the f32 additions in
//               ascending k.  Device: the order and internal rounding of v_mfma_f32_32x32x16_bf16,
//               which are not documented -- the one place where the two may differ.
//   z           f32 arithmetic on the unrounded h_{F-1} and the f32 fw_F from fb_F: the twin an
//               ascending fmaf chain, the device any order.  Sigmoid, sign, NaN border, raw,
//               a_is_left and the layout as above.  F = 1 has no hidden layer and follows the same
//               rules.
//   weights     the hidden layers' are rounded once; one that is not finite or rounds to +-inf is an
//               error in this mode.
// Integer operands with |fb| + sum |terms| < 2^24 make every sum exact in any order: device ==
// twin, bit for bit.
__host__ __device__ inline uint16_t ac_bf16(float x)
{
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((b >> 16) | 0x0040u);
    return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}

__host__ __device__ inline float ac_bf16_float(uint16_t v)
{
    const uint32_t b = (uint32_t)v << 16;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

// the first hidden layer (1 .. F-1) with a weight that is not finite or rounds to +-inf, or 0
inline int ac_fc_bf16_bad(int F, int U, const float* const* fw)
{
    for (int i = 1; i < F; i++)
        for (size_t j = 0; j < (size_t)U * U; j++)
            if ((ac_bf16(fw[i][j]) & 0x7F80u) == 0x7F80u) return i;
    return 0;
}

// the packed scorer (ac_pack_fc) with its hidden matrices replaced by their bf16 values: the twin's
inline void ac_round_fc(const AcFc& fc, float* fcp)
{
    for (size_t j = fc.hid(1); j < fc.last(); j++) fcp[j] = ac_bf16_float(ac_bf16(fcp[j]));
}

// The hidden matrices as the device reads them: [layer][t][q][lane][8] bf16, the A fragment of
// mfma_f32_32x32x16_bf16 for output tile t (units 32 t ..) and k-step q.  Lane l = (r = l & 31,
// h = l >> 5), element j: fw[32 t + r][ac_bf16_unit(q, h, j)].  The k order is the one an
// accumulator tile implies when its registers 8 s .. 8 s + 7 become the next k-step's operand.
constexpr int ac_bf16_unit(int q, int h, int j) { return 16 * q + 8 * (j >> 2) + 4 * h + (j & 3); }

inline size_t ac_pack_fc_bf16_count(int F, int U) { return (size_t)(F - 1) * U * U; }

inline void ac_pack_fc_bf16(int F, int U, const float* const* fw, uint16_t* dst)
{
    const int NU = U / 32, NQ = U / 16;
    for (int i = 1; i < F; i++)
        for (int t = 0; t < NU; t++)
            for (int q = 0; q < NQ; q++)
                for (int l = 0; l < 64; l++)
                    for (int j = 0; j < 8; j++)
                        *dst++ = ac_bf16(fw[i][(size_t)(32 * t + (l & 31)) * U + ac_bf16_unit(q, l >> 5, j)]);
}

// ---- the twin: plain loops, explicit fmaf, built for CPUs with FMA units and for any x86-64
// (sm_mccnn.hpp).

__attribute__((always_inline)) inline void ac_conv_pixel_host(const float* in, int cin, int H, int W, int y, int x,
                                                              const float* wp, const float* b, float* out)
{
    const int ws = cin == 1 ? AC_C : AC_CP;
    float acc[AC_C];
    for (int co = 0; co < AC_C; co++) acc[co] = b[co];
    for (int tap = 0; tap < 9; tap++) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float* px = inside ? in + ((size_t)yy * W + xx) * cin : nullptr;
        for (int ci = 0; ci < cin; ci++) {
            const float v = inside ? px[ci] : 0.0f;
            const float* wr = wp + ((size_t)tap * cin + ci) * ws;
            for (int co = 0; co < AC_C; co++) acc[co] = __builtin_fmaf(v, wr[co], acc[co]);
        }
    }
    for (int co = 0; co < AC_C; co++) out[co] = acc[co] > 0.0f ? acc[co] : 0.0f;
}

__attribute__((always_inline)) inline void ac_features_image_body(int L, const float* wp, const float* bias,
                                                                  const float* plane, int H, int W, float* ping,
                                                                  float* pong, float* feat)
{
    const float* in = plane;
    for (int i = 0; i < L; i++) {
        float* out = i == L - 1 ? feat : (i & 1) ? pong : ping;
        const float* w = i == 0 ? wp : wp + AC_W0 + (size_t)(i - 1) * AC_WL;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                ac_conv_pixel_host(in, i == 0 ? 1 : AC_C, H, W, y, x, w, bias + i * AC_CP, out + ((size_t)y * W + x) * AC_C);
        in = out;
    }
}

// out[p][u] = chain from bias[u] (0 without one) of fmaf(feat[p][c], wt[c][u], .)
__attribute__((always_inline)) inline void ac_project_body(const float* feat, size_t npix, int U, const float* wt,
                                                           const float* bias, float* out)
{
    for (size_t p = 0; p < npix; p++) {
        float* o = out + p * U;
        for (int u = 0; u < U; u++) o[u] = bias ? bias[u] : 0.0f;
        for (int c = 0; c < AC_C; c++) {
            const float v = feat[p * AC_C + c];
            const float* wr = wt + (size_t)c * U;
            for (int u = 0; u < U; u++) o[u] = __builtin_fmaf(v, wr[u], o[u]);
        }
    }
}

// the cells of one image from its two projection maps (pa: a's own, pb: the other image's)
__attribute__((always_inline)) inline void ac_score_body(const AcFc& fc, const float* fcp, const float* pa,
                                                         const float* pb, int H, int W, int D, long long m, bool raw,
                                                         float* vol)
{
    const int U = fc.U, F = fc.F;
    float h[AC_MAXU], acc[AC_MAXU];
    for (int d = 0; d < D; d++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const long long xb = (long long)x - (m + d);
                float v = std::nanf("");
                if (xb >= 0 && xb < W) {
                    const float* a = pa + ((size_t)y * W + x) * U;
                    const float* b = pb + ((size_t)y * W + (size_t)xb) * U;
                    for (int u = 0; u < U; u++) {
                        const float s = a[u] + b[u];
                        h[u] = s > 0.0f ? s : 0.0f;
                    }
                    for (int i = 1; i < F; i++) {
                        const float* wt = fcp + fc.hid(i);
                        const float* bi = fcp + fc.bias(i);
                        for (int u = 0; u < U; u++) acc[u] = bi[u];
                        for (int k = 0; k < U; k++) {
                            const float hv = h[k];
                            const float* wr = wt + (size_t)k * U;
                            for (int u = 0; u < U; u++) acc[u] = __builtin_fmaf(hv, wr[u], acc[u]);
                        }
                        for (int u = 0; u < U; u++) h[u] = acc[u] > 0.0f ? acc[u] : 0.0f;
                    }
                    const float* wl = fcp + fc.last();
                    float z = fcp[fc.bias(F)];
                    for (int k = 0; k < U; k++) z = __builtin_fmaf(h[k], wl[k], z);
                    v = raw ? -z : -ac_sigmoid(z);
                }
                vol[((size_t)d * H + y) * W + x] = v;
            }
}

// precision "bf16": fcp is ac_round_fc's, so a hidden weight is its bf16 value already
__attribute__((always_inline)) inline void ac_score16_body(const AcFc& fc, const float* fcp, const float* pa,
                                                           const float* pb, int H, int W, int D, long long m, bool raw,
                                                           float* vol)
{
    const int U = fc.U, F = fc.F;
    float h[AC_MAXU], acc[AC_MAXU];
    for (int d = 0; d < D; d++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const long long xb = (long long)x - (m + d);
                float v = std::nanf("");
                if (xb >= 0 && xb < W) {
                    const float* a = pa + ((size_t)y * W + x) * U;
                    const float* b = pb + ((size_t)y * W + (size_t)xb) * U;
                    for (int u = 0; u < U; u++) {
                        const float s = a[u] + b[u];
                        h[u] = s > 0.0f ? s : 0.0f;
                    }
                    for (int i = 1; i < F; i++) {
                        const float* wt = fcp + fc.hid(i);
                        const float* bi = fcp + fc.bias(i);
                        for (int u = 0; u < U; u++) acc[u] = bi[u];
                        for (int k = 0; k < U; k++) {
                            const float hv = ac_bf16_float(ac_bf16(h[k]));
                            const float* wr = wt + (size_t)k * U;
                            for (int u = 0; u < U; u++) {
                                const float p = hv * wr[u];  // exact; no contraction in this header
                                acc[u] = acc[u] + p;
                            }
                        }
                        for (int u = 0; u < U; u++) h[u] = acc[u] > 0.0f ? acc[u] : 0.0f;
                    }
                    const float* wl = fcp + fc.last();
                    float z = fcp[fc.bias(F)];
                    for (int k = 0; k < U; k++) z = __builtin_fmaf(h[k], wl[k], z);
                    v = raw ? -z : -ac_sigmoid(z);
                }
                vol[((size_t)d * H + y) * W + x] = v;
            }
}

SM_MC_FMA_TARGET inline void ac_features_image_fma(int L, const float* wp, const float* bias, const float* plane, int H,
                                                   int W, float* ping, float* pong, float* feat)
{
    ac_features_image_body(L, wp, bias, plane, H, W, ping, pong, feat);
}
inline void ac_features_image_any(int L, const float* wp, const float* bias, const float* plane, int H, int W,
                                  float* ping, float* pong, float* feat)
{
    ac_features_image_body(L, wp, bias, plane, H, W, ping, pong, feat);
}
SM_MC_FMA_TARGET inline void ac_project_fma(const float* feat, size_t npix, int U, const float* wt, const float* bias,
                                            float* out)
{
    ac_project_body(feat, npix, U, wt, bias, out);
}
inline void ac_project_any(const float* feat, size_t npix, int U, const float* wt, const float* bias, float* out)
{
    ac_project_body(feat, npix, U, wt, bias, out);
}
SM_MC_FMA_TARGET inline void ac_score_fma(const AcFc& fc, const float* fcp, const float* pa, const float* pb, int H,
                                          int W, int D, long long m, bool raw, float* vol)
{
    ac_score_body(fc, fcp, pa, pb, H, W, D, m, raw, vol);
}
inline void ac_score_any(const AcFc& fc, const float* fcp, const float* pa, const float* pb, int H, int W, int D,
                         long long m, bool raw, float* vol)
{
    ac_score_body(fc, fcp, pa, pb, H, W, D, m, raw, vol);
}

SM_MC_FMA_TARGET inline void ac_score16_fma(const AcFc& fc, const float* fcp, const float* pa, const float* pb, int H,
                                            int W, int D, long long m, bool raw, float* vol)
{
    ac_score16_body(fc, fcp, pa, pb, H, W, D, m, raw, vol);
}
inline void ac_score16_any(const AcFc& fc, const float* fcp, const float* pa, const float* pb, int H, int W, int D,
                           long long m, bool raw, float* vol)
{
    ac_score16_body(fc, fcp, pa, pb, H, W, D, m, raw, vol);
}

// features of n images (rows row_stride, images image_stride bytes apart) into feat [n][H][W][112];
// wp / bias: ac_pack_conv's.  Returns the index of the first constant image, or -1.
inline int mcacc_features_host(int L, const float* wp, const float* bias, const uint8_t* gray, int n, size_t image_stride,
                               int H, int W, size_t row_stride, float* feat)
{
    const size_t npix = (size_t)H * W;
    std::vector<float> plane(npix), ping(L > 1 ? npix * AC_C : 0), pong(L > 2 ? npix * AC_C : 0);
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
        float* f = feat + (size_t)img * npix * AC_C;
        if (fma)
            ac_features_image_fma(L, wp, bias, plane.data(), H, W, ping.data(), pong.data(), f);
        else
            ac_features_image_any(L, wp, bias, plane.data(), H, W, ping.data(), pong.data(), f);
    }
    return -1;
}

// the volume [n][D][H][W] of feature maps [n][H][W][112]; a_is_left: fa feeds PL (and fb PR)
// bf16: fcp is ac_round_fc's and the cells follow precision "bf16"
inline void mcacc_join_host(const AcFc& fc, const float* fcp, const float* fa, const float* fb, int n, int H, int W,
                            int D, int minD, bool a_is_left, bool raw, float* vol, bool bf16 = false)
{
    const size_t npix = (size_t)H * W, fimg = npix * AC_C, vimg = (size_t)D * npix;
    const int m = mc_clamp_min_disparity(minD, W, D);
    const bool fma = mc_cpu_has_fma();
    std::vector<float> pa(npix * fc.U), pb(npix * fc.U);
    for (int img = 0; img < n; img++) {
        for (int side = 0; side < 2; side++) {
            const bool left = (side == 0) == a_is_left;
            const float* f = (side == 0 ? fa : fb) + img * fimg;
            const float* wt = fcp + (left ? fc.pl() : fc.pr());
            const float* bias = left ? fcp + fc.bias(0) : nullptr;
            float* out = side == 0 ? pa.data() : pb.data();
            if (fma)
                ac_project_fma(f, npix, fc.U, wt, bias, out);
            else
                ac_project_any(f, npix, fc.U, wt, bias, out);
        }
        if (bf16 && fma)
            ac_score16_fma(fc, fcp, pa.data(), pb.data(), H, W, D, m, raw, vol + img * vimg);
        else if (bf16)
            ac_score16_any(fc, fcp, pa.data(), pb.data(), H, W, D, m, raw, vol + img * vimg);
        else if (fma)
            ac_score_fma(fc, fcp, pa.data(), pb.data(), H, W, D, m, raw, vol + img * vimg);
        else
            ac_score_any(fc, fcp, pa.data(), pb.data(), H, W, D, m, raw, vol + img * vimg);
    }
}

#if defined(__HIPCC__) && !defined(SM_MCACC_NO_KERNELS)
// ---- kernels

typedef float ac_f16 __attribute__((ext_vector_type(16)));

constexpr int AC_BLOCK = 256;
constexpr int AC_Q = AC_C / 4;                        // float4 groups of a pixel's features
constexpr int AC_TW = 32, AC_TH = 2;                  // the pixel tile of a convolution workgroup
constexpr int AC_HW = AC_TW + 2, AC_HH = AC_TH + 2;   // with its halo
constexpr int AC_PS = 114;                            // floats between the pixels of the LDS tile (57 odd: banks 50 j + h)
constexpr int AC_DM = 128, AC_DN = 128, AC_DK = 16;   // dense layer: rows, columns, k per staged chunk
constexpr int AC_AS = 18;                             // floats between the rows of the A chunk (9 odd)
constexpr int AC_BS = 160;                            // floats between the k rows of the B chunk (32 mod 64)
constexpr int AC_FK = 32, AC_FS = 33;                 // final unit: k per staged chunk, floats between its rows

struct AcSumArgs {
    const uint8_t* gray;
    size_t image_stride, row_stride;
    int H, W;
    unsigned long long* sums;  // [img][2]: Sx, Sxx (zeroed before the launch)
};

// exact integer sums of every image (sm_mccnn.hpp's k_mc_sums, which lives in that unit alone):
// blockIdx.y the image, the blocks stride over its pixels
__global__ __launch_bounds__(AC_BLOCK) void k_ac_sums(AcSumArgs a)
{
    const uint8_t* g = a.gray + (size_t)blockIdx.y * a.image_stride;
    const unsigned npix = (unsigned)a.H * (unsigned)a.W;
    unsigned long long sx = 0, sxx = 0;
    for (unsigned i = blockIdx.x * AC_BLOCK + threadIdx.x; i < npix; i += gridDim.x * AC_BLOCK) {
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

struct AcL0Args {
    const uint8_t* gray;  // one image
    size_t row_stride;
    int H, W;
    const float* tab;     // its 256 normalised grey levels
    const float* w;       // [tap][112]
    const float* b;
    float* out;           // [H][W][112]
};

// layer 0 (K = 9) on the VALU: a thread computes 4 feature maps of a pixel
__global__ __launch_bounds__(AC_BLOCK) void k_ac_layer0(AcL0Args a)
{
    __shared__ float tab[256];
    tab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();
    const unsigned idx = blockIdx.x * AC_BLOCK + threadIdx.x;
    const unsigned pix = idx / AC_Q, q = idx - pix * AC_Q;
    if (pix >= (unsigned)a.H * (unsigned)a.W) return;
    const int y = (int)(pix / (unsigned)a.W), x = (int)(pix - (unsigned)y * (unsigned)a.W);
    const float4 bb = *(const float4*)(a.b + 4 * q);
    float acc[4] = {bb.x, bb.y, bb.z, bb.w};
    for (int tap = 0; tap < 9; tap++) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        float v = 0.0f;
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) v = tab[a.gray[(size_t)yy * a.row_stride + xx]];
        const float4 w = *(const float4*)(a.w + tap * AC_C + 4 * q);
        acc[0] = __builtin_fmaf(v, w.x, acc[0]);
        acc[1] = __builtin_fmaf(v, w.y, acc[1]);
        acc[2] = __builtin_fmaf(v, w.z, acc[2]);
        acc[3] = __builtin_fmaf(v, w.w, acc[3]);
    }
    for (int j = 0; j < 4; j++) acc[j] = acc[j] > 0.0f ? acc[j] : 0.0f;
    *(float4*)(a.out + (size_t)pix * AC_C + 4 * q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

struct AcConvArgs {
    const float* in;  // [H][W][112]
    float* out;       // [H][W][112]
    const float* w;   // [k][128]
    const float* b;   // [128]
    int H, W;
};

// One 3x3, 112 -> 112 layer as an implicit GEMM on mfma_f32_32x32x2f32.  A workgroup: 2 rows x 32
// columns of pixels, its 4 x 34 halo tile with all 112 maps in LDS (zeros outside the image; 62 KB,
// two workgroups per CU).  A wave: one row (M = 32 pixels) x one half of the 128 padded outputs =
// two accumulators.  An instruction's A operand is in[pixel lane & 31][ci = 2 s + (lane >> 5)] from
// the tile, its B operand w[k][co = lane & 31 (+ 32)] straight from the packed weights (128-byte
// rows, the same for every workgroup: they stay in the caches); it adds k = 2 s, then 2 s + 1, so
// 56 of them per tap over the nine taps are the chain.  The accumulators start at the bias.
__global__ __launch_bounds__(AC_BLOCK) void k_ac_conv(AcConvArgs a)
{
    __shared__ float tile[AC_HH * AC_HW * AC_PS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int row = wv >> 1, nh = wv & 1;
    const int x0 = blockIdx.x * AC_TW, y0 = blockIdx.y * AC_TH;

    for (int i = tid; i < AC_HH * AC_HW * AC_Q; i += AC_BLOCK) {
        const int p = i / AC_Q, q = i - p * AC_Q;
        const int ty = p / AC_HW, tx = p - ty * AC_HW;
        const int gy = y0 + ty - 1, gx = x0 + tx - 1;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = *(const float4*)(a.in + ((size_t)gy * a.W + gx) * AC_C + 4 * q);
        float2* t = (float2*)(tile + p * AC_PS + 4 * q);
        t[0] = make_float2(v.x, v.y);
        t[1] = make_float2(v.z, v.w);
    }
    ac_f16 acc[2];
    for (int n = 0; n < 2; n++) {
        const float bv = a.b[64 * nh + 32 * n + j];
        for (int r = 0; r < 16; r++) acc[n][r] = bv;
    }
    __syncthreads();

    for (int tap = 0; tap < 9; tap++) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        const float* ap = tile + ((row + ky) * AC_HW + j + kx) * AC_PS + h;
        const float* bp = a.w + ((size_t)tap * AC_C + h) * AC_CP + 64 * nh + j;
#pragma unroll 8
        for (int s = 0; s < AC_C / 2; s++) {
            const float av = ap[2 * s];
            const float bv0 = bp[2 * s * AC_CP], bv1 = bp[2 * s * AC_CP + 32];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv1, acc[1], 0, 0, 0);
        }
    }

    // C/D: column (co) = lane & 31, row (pixel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int gy = y0 + row;
    if (gy >= a.H) return;
    for (int r = 0; r < 16; r++) {
        const int gx = x0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (gx >= a.W) continue;
        float* o = a.out + ((size_t)gy * a.W + gx) * AC_C;
        for (int n = 0; n < 2; n++) {
            const int co = 64 * nh + 32 * n + j;
            const float v = acc[n][r];
            if (co < AC_C) o[co] = v > 0.0f ? v : 0.0f;
        }
    }
}

struct AcDenseArgs {
    const float* in;    // [M][K]
    const float* wt;    // [K][N]
    const float* bias;  // [N], or null: the chains start at 0
    float* out;         // [M][N]
    unsigned M;
    int K, N;           // K a multiple of 16, N of 32
};

// out = act(in x wt + bias) on mfma_f32_32x32x2f32: the projections (M = pixels, K = 112) and the
// scorer's hidden layers (M = cells of a chunk, K = N = U).  A workgroup: 128 rows x 128 columns,
// k in chunks of 16 through LDS, double-buffered (the next chunk waits in registers while this one
// is multiplied).  A wave: 64 x 64 = 2 x 2 accumulators, each the whole chain of its outputs in
// ascending k.  Rows past M and columns past N are staged as zeros and not stored.
template <bool RELU>
__global__ __launch_bounds__(AC_BLOCK) void k_ac_dense(AcDenseArgs a)
{
    __shared__ float As[2][AC_DM * AC_AS];
    __shared__ float Bs[2][AC_DK * AC_BS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int wm = wv >> 1, wn = wv & 1;
    const unsigned m0 = blockIdx.x * AC_DM;
    const int n0 = blockIdx.y * AC_DN;

    // staging: thread t moves A rows (t >> 2) and (t >> 2) + 64, floats 4 (t & 3) ..; B rows (t >> 5)
    // and (t >> 5) + 8, floats 4 (t & 31) ..
    const int ar = tid >> 2, aq = tid & 3, br = tid >> 5, bq = tid & 31;
    const bool bin = n0 + 4 * bq < a.N;
    float4 ra[2], rb[2];
    auto fetch = [&](int k0) {
        for (int i = 0; i < 2; i++) {
            const unsigned m = m0 + ar + 64 * i;
            ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (m < a.M) ra[i] = *(const float4*)(a.in + (size_t)m * a.K + k0 + 4 * aq);
            rb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (bin) rb[i] = *(const float4*)(a.wt + (size_t)(k0 + br + 8 * i) * a.N + n0 + 4 * bq);
        }
    };
    auto stash = [&](int buf) {
        for (int i = 0; i < 2; i++) {
            float2* t = (float2*)(As[buf] + (ar + 64 * i) * AC_AS + 4 * aq);
            t[0] = make_float2(ra[i].x, ra[i].y);
            t[1] = make_float2(ra[i].z, ra[i].w);
            *(float4*)(Bs[buf] + (br + 8 * i) * AC_BS + 4 * bq) = rb[i];
        }
    };

    ac_f16 acc[2][2];
    for (int n = 0; n < 2; n++) {
        const int col = n0 + 64 * wn + 32 * n + j;
        const float bv = (a.bias && col < a.N) ? a.bias[col] : 0.0f;
        for (int m = 0; m < 2; m++)
            for (int r = 0; r < 16; r++) acc[m][n][r] = bv;
    }
    fetch(0);
    stash(0);
    __syncthreads();

    const int nchunks = a.K / AC_DK;
    for (int c = 0; c < nchunks; c++) {
        if (c + 1 < nchunks) fetch((c + 1) * AC_DK);
        const float* a0 = As[c & 1] + (64 * wm + j) * AC_AS + h;
        const float* a1 = a0 + 32 * AC_AS;
        const float* b0 = Bs[c & 1] + h * AC_BS + 64 * wn + j;
#pragma unroll
        for (int s = 0; s < AC_DK / 2; s++) {
            const float av0 = a0[2 * s], av1 = a1[2 * s];
            const float bv0 = b0[2 * s * AC_BS], bv1 = b0[2 * s * AC_BS + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv1, acc[1][1], 0, 0, 0);
        }
        if (c + 1 < nchunks) stash((c + 1) & 1);  // the buffer chunk c - 1 was read from, before the last barrier
        __syncthreads();
    }

    // C/D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    for (int m = 0; m < 2; m++)
        for (int r = 0; r < 16; r++) {
            const unsigned gm = m0 + 64 * wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (gm >= a.M) continue;
            float* o = a.out + (size_t)gm * a.N;
            for (int n = 0; n < 2; n++) {
                const int col = n0 + 64 * wn + 32 * n + j;
                if (col >= a.N) continue;
                const float v = acc[m][n][r];
                o[col] = RELU ? (v > 0.0f ? v : 0.0f) : v;
            }
        }
}

struct AcCellArgs {
    const float* pa;   // [H][W][U] the projection of a's features
    const float* pb;   // [H][W][U] of b's
    float* h1;         // [cells][U]
    size_t c0;         // first cell of the chunk, in volume order (d, y, x)
    unsigned cells;
    int H, W, U, m;    // m clamped (mc_clamp_min_disparity)
};

// the scorer's first layer for a chunk of cells: h1 = relu(pa[y, x] + pb[y, x - (m + d)]); a thread
// makes 4 units of a cell (zeros for a cell outside the image, whose plane value will be NaN)
__global__ __launch_bounds__(AC_BLOCK) void k_ac_h1(AcCellArgs a)
{
    const unsigned uq = (unsigned)a.U / 4;
    const unsigned idx = blockIdx.x * AC_BLOCK + threadIdx.x;
    const unsigned cell = idx / uq, q = idx - cell * uq;
    if (cell >= a.cells) return;
    const size_t c = a.c0 + cell, plane = (size_t)a.H * a.W;
    const int d = (int)(c / plane);
    const unsigned pix = (unsigned)(c - (size_t)d * plane);
    const int y = (int)(pix / (unsigned)a.W), x = (int)(pix - (unsigned)y * (unsigned)a.W);
    const int xb = x - (a.m + d);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (xb >= 0 && xb < a.W) {
        const float4 p = *(const float4*)(a.pa + (size_t)pix * a.U + 4 * q);
        const float4 r = *(const float4*)(a.pb + ((size_t)y * a.W + xb) * a.U + 4 * q);
        const float s0 = p.x + r.x, s1 = p.y + r.y, s2 = p.z + r.z, s3 = p.w + r.w;
        v = make_float4(s0 > 0.0f ? s0 : 0.0f, s1 > 0.0f ? s1 : 0.0f, s2 > 0.0f ? s2 : 0.0f, s3 > 0.0f ? s3 : 0.0f);
    }
    *(float4*)(a.h1 + (size_t)cell * a.U + 4 * q) = v;
}

struct AcFinalArgs {
    const float* h;    // [cells][U] the last hidden layer of the chunk
    const float* w;    // [U] the last unit
    const float* b;    // its bias
    float* vol;        // the image's volume [D][H][W]
    size_t c0;
    unsigned cells;
    int H, W, U, m, raw;
};

// The last unit (K = U, N = 1), the sigmoid and the NaN border: a thread per cell.  The block's
// 256 x 32 piece of h goes through LDS (128-byte row reads, 33-float rows: a thread then reads its
// own row without bank conflicts) so the chain runs in ascending k; the cells are consecutive in
// volume order, so the stores are full-width row segments.
__global__ __launch_bounds__(AC_BLOCK) void k_ac_final(AcFinalArgs a)
{
    __shared__ float hs[AC_BLOCK * AC_FS];
    const int tid = threadIdx.x;
    const unsigned cb = blockIdx.x * AC_BLOCK;
    float z = a.b[0];
    for (int k0 = 0; k0 < a.U; k0 += AC_FK) {
        __syncthreads();
        for (int i = tid; i < AC_BLOCK * AC_FK; i += AC_BLOCK) {
            const unsigned cl = (unsigned)i >> 5, kk = (unsigned)i & 31;
            hs[cl * AC_FS + kk] = cb + cl < a.cells ? a.h[(size_t)(cb + cl) * a.U + k0 + kk] : 0.0f;
        }
        __syncthreads();
        const float* hr = hs + tid * AC_FS;
#pragma unroll 8
        for (int kk = 0; kk < AC_FK; kk++) z = __builtin_fmaf(hr[kk], a.w[k0 + kk], z);
    }
    const unsigned cell = cb + tid;
    if (cell >= a.cells) return;
    const size_t c = a.c0 + cell, plane = (size_t)a.H * a.W;
    const int d = (int)(c / plane);
    const unsigned pix = (unsigned)(c - (size_t)d * plane);
    const int x = (int)(pix % (unsigned)a.W);
    const int xb = x - (a.m + d);
    a.vol[c] = (xb >= 0 && xb < a.W) ? (a.raw ? -z : -ac_sigmoid(z)) : __builtin_nanf("");
}

// ---- precision "bf16": the whole scorer of a tile of cells in one kernel
typedef __bf16 ac_b8 __attribute__((ext_vector_type(8)));

constexpr int AC_GX = 32;  // cells of a wave: 32 consecutive columns of one row of one plane
constexpr int AC_GD = 4;   // planes of a workgroup: wave w takes plane 4 blockIdx + w of the same columns

struct AcFusedArgs {
    const float* pa;      // [H][W][U] the projection of a's features
    const float* pb;      // [H][W][U] of b's
    const uint16_t* wq;   // ac_pack_fc_bf16's
    const float* bias;    // fb_0 .. fb_{F-1}, [U] each (fb_0 is in the projection already)
    const float* wl;      // [U] the output unit
    const float* bl;      // its bias
    float* vol;           // the image's volume [D][H][W]
    int H, W, D, F, m, raw;
};

__device__ inline ac_b8 ac_pack_b8(const float* v)
{
    uint32_t p[4];
    for (int j = 0; j < 4; j++) p[j] = (uint32_t)ac_bf16(v[2 * j]) | ((uint32_t)ac_bf16(v[2 * j + 1]) << 16);
    return __builtin_bit_cast(ac_b8, make_uint4(p[0], p[1], p[2], p[3]));
}

// Transposed products on mfma_f32_32x32x16_bf16: X[unit][cell] = W[unit][k] H[k][cell], the weights
// the A operand, the activations the B operand.  A wave owns 32 cells (the columns of X, one per
// lane & 31) through every layer: a result tile has its units in the 16 registers, which is what the
// next layer sums over, so registers 8 s .. 8 s + 7 of tile t, rounded, are the B fragment of k-step
// 2 t + s with no lane movement and no LDS (the k order inside a step is ac_bf16_unit's, and the
// packed weights follow it).  h1 is loaded in that order too.  The activations of a cell never
// leave the registers: 2 NU fragments in, 2 NU out, two accumulator tiles; one wave per SIMD.  The
// A fragments are 1 KB coalesced reads of the packed weights, the same sequence in every wave of
// the chip (L2; the four waves of a workgroup run the same columns at four consecutive planes, so
// PL is read once per workgroup and PR's rows overlap in all but three columns).  The last hidden
// layer is not rounded: it goes straight into the output unit's partial sums, which the two lane
// halves of a cell add at the end.
template <int NU>
__global__ __launch_bounds__(AC_BLOCK) void k_ac_fused16(AcFusedArgs a)
{
    constexpr int U = 32 * NU, NQ = 2 * NU, TT = NU % 2 == 0 ? 2 : 1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int ndg = (a.D + AC_GD - 1) / AC_GD;
    const int dg = (int)(blockIdx.x % (unsigned)ndg), xt = (int)(blockIdx.x / (unsigned)ndg);
    const int d = AC_GD * dg + wv, x = AC_GX * xt + c;
    if (d >= a.D) return;  // the whole wave; no barrier below
    const int xb = x - (a.m + d);
    const bool inx = x < a.W, ok = inx && xb >= 0 && xb < a.W;

    for (int y = blockIdx.y; y < a.H; y += gridDim.y) {
        ac_b8 hb[NQ];
        float z = 0.0f;
        {
            const float* pa = a.pa + ((size_t)y * a.W + (ok ? x : 0)) * U + 4 * h;
            const float* pb = a.pb + ((size_t)y * a.W + (ok ? xb : 0)) * U + 4 * h;
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                float v[8];
#pragma unroll
                for (int g = 0; g < 2; g++) {
                    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r = p;
                    if (ok) {
                        p = *(const float4*)(pa + 16 * q + 8 * g);
                        r = *(const float4*)(pb + 16 * q + 8 * g);
                    }
                    const float s0 = p.x + r.x, s1 = p.y + r.y, s2 = p.z + r.z, s3 = p.w + r.w;
                    v[4 * g + 0] = s0 > 0.0f ? s0 : 0.0f;
                    v[4 * g + 1] = s1 > 0.0f ? s1 : 0.0f;
                    v[4 * g + 2] = s2 > 0.0f ? s2 : 0.0f;
                    v[4 * g + 3] = s3 > 0.0f ? s3 : 0.0f;
                }
                if (a.F == 1) {
#pragma unroll
                    for (int g = 0; g < 2; g++) {
                        const float4 w = *(const float4*)(a.wl + 16 * q + 8 * g + 4 * h);
                        z = __builtin_fmaf(v[4 * g + 0], w.x, z);
                        z = __builtin_fmaf(v[4 * g + 1], w.y, z);
                        z = __builtin_fmaf(v[4 * g + 2], w.z, z);
                        z = __builtin_fmaf(v[4 * g + 3], w.w, z);
                    }
                }
                hb[q] = ac_pack_b8(v);
            }
        }

        for (int i = 1; i < a.F; i++) {
            const ac_b8* wq = (const ac_b8*)(a.wq + (size_t)(i - 1) * U * U) + lane;
            const float* bi = a.bias + (size_t)i * U + 4 * h;
            const bool lastl = i == a.F - 1;
            ac_b8 hn[NQ];
#pragma unroll
            for (int t0 = 0; t0 < NU; t0 += TT) {
                ac_f16 acc[TT];
#pragma unroll
                for (int tt = 0; tt < TT; tt++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const float4 b4 = *(const float4*)(bi + 32 * (t0 + tt) + 8 * g);
                        acc[tt][4 * g + 0] = b4.x, acc[tt][4 * g + 1] = b4.y;
                        acc[tt][4 * g + 2] = b4.z, acc[tt][4 * g + 3] = b4.w;
                    }
#pragma unroll
                for (int q = 0; q < NQ; q++)
#pragma unroll
                    for (int tt = 0; tt < TT; tt++)
                        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[((t0 + tt) * NQ + q) * 64], hb[q], acc[tt], 0, 0, 0);
#pragma unroll
                for (int tt = 0; tt < TT; tt++) {
                    float v[16];
#pragma unroll
                    for (int r = 0; r < 16; r++) v[r] = acc[tt][r] > 0.0f ? acc[tt][r] : 0.0f;
                    if (lastl) {
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const float4 w = *(const float4*)(a.wl + 32 * (t0 + tt) + 8 * g + 4 * h);
                            z = __builtin_fmaf(v[4 * g + 0], w.x, z);
                            z = __builtin_fmaf(v[4 * g + 1], w.y, z);
                            z = __builtin_fmaf(v[4 * g + 2], w.z, z);
                            z = __builtin_fmaf(v[4 * g + 3], w.w, z);
                        }
                    }
                    hn[2 * (t0 + tt)] = ac_pack_b8(v);
                    hn[2 * (t0 + tt) + 1] = ac_pack_b8(v + 8);
                }
            }
#pragma unroll
            for (int q = 0; q < NQ; q++) hb[q] = hn[q];
        }

        z = (z + __shfl_xor(z, 32)) + a.bl[0];
        if (h == 0 && inx)
            a.vol[((size_t)d * a.H + y) * a.W + x] = ok ? (a.raw ? -z : -ac_sigmoid(z)) : __builtin_nanf("");
    }
}
#endif  // __HIPCC__ && !SM_MCACC_NO_KERNELS

}  // namespace smk
