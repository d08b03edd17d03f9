// sm_api_mcacc.hip — C-ABI of the MC-CNN accurate matching cost (sm_mcacc.hpp).  The only unit with these kernels.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sm_ctx.hpp"
#include "sm_mcacc.hpp"

extern "C" {

// ---- MC-CNN accurate matching cost (sm_mcacc.hpp)
namespace {

int mcacc_check_images(sm_ctx* ctx, int n, int H, int W)
{
    if (n < 1 || n > 65535) return fail(ctx, SM_E_ARG, "mcacc: %d images (1 .. 65535)", n);
    if (H < 1 || W < 1) return fail(ctx, SM_E_ARG, "mcacc: empty image (%dx%d)", W, H);
    if ((size_t)H * (size_t)W > smk::MC_MAXPIX)
        return fail(ctx, SM_E_UNSUPPORTED, "mcacc: image %dx%d has 2^24 pixels or more", W, H);
    return SM_OK;
}

int mcacc_check_strides(sm_ctx* ctx, int n, size_t image_stride, int H, int W, size_t row_stride)
{
    if (row_stride < (size_t)W) return fail(ctx, SM_E_ARG, "mcacc: row_stride %zu smaller than a row (%d)", row_stride, W);
    if (n > 1 && image_stride < (size_t)(H - 1) * row_stride + (size_t)W)
        return fail(ctx, SM_E_ARG, "mcacc: image_stride %zu smaller than one image", image_stride);
    return SM_OK;
}

// the kernels read and write feature maps 16 bytes at a time
int mcacc_check_aligned(sm_ctx* ctx, const void* p, const char* what)
{
    if ((uintptr_t)p & 15) return fail(ctx, SM_E_ARG, "mcacc: %s is not 16-byte aligned", what);
    return SM_OK;
}

int mcacc_check_planes(sm_ctx* ctx, int D)
{
    if (D < 1 || D > smk::MC_MAXD) return fail(ctx, SM_E_ARG, "mcacc: %d disparity planes (1 .. %d)", D, smk::MC_MAXD);
    return SM_OK;
}

int mcacc_check_conv(sm_ctx* ctx, int L, const float* const* w, const float* const* b)
{
    if (L < 1 || L > smk::AC_MAXL) return fail(ctx, SM_E_ARG, "mcacc: %d convolutions (1 .. %d)", L, smk::AC_MAXL);
    if (!w || !b) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    for (int i = 0; i < L; i++)
        if (!w[i] || !b[i]) return fail(ctx, SM_E_ARG, "mcacc: weights or biases of convolution %d are NULL", i);
    return SM_OK;
}

int mcacc_check_fc(sm_ctx* ctx, int F, int U, const float* const* fw, const float* const* fb)
{
    if (F < 1 || F > smk::AC_MAXF) return fail(ctx, SM_E_ARG, "mcacc: %d hidden layers (1 .. %d)", F, smk::AC_MAXF);
    if (U < 32 || U > smk::AC_MAXU || U % 32)
        return fail(ctx, SM_E_ARG, "mcacc: %d units (a multiple of 32, 32 .. %d)", U, smk::AC_MAXU);
    if (!fw || !fb) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    for (int i = 0; i <= F; i++)
        if (!fw[i] || !fb[i]) return fail(ctx, SM_E_ARG, "mcacc: weights or biases of scorer layer %d are NULL", i);
    return SM_OK;
}

int mcacc_dense(sm_ctx* ctx, const float* in, const float* wt, const float* bias, float* out, unsigned M, int K, int N,
                bool relu)
{
    smk::AcDenseArgs da{in, wt, bias, out, M, K, N};
    const dim3 grid((M + smk::AC_DM - 1) / smk::AC_DM, (N + smk::AC_DN - 1) / smk::AC_DN);
    if (relu)
        hipLaunchKernelGGL(smk::k_ac_dense<true>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, da);
    else
        hipLaunchKernelGGL(smk::k_ac_dense<false>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, da);
    return SM_OK;
}

// precision "bf16": one launch per image, no scratch
void mcacc_launch_fused16(sm_ctx* ctx, const smk::AcFusedArgs& fa, int U)
{
    const unsigned xt = ((unsigned)fa.W + smk::AC_GX - 1) / smk::AC_GX, ndg = ((unsigned)fa.D + smk::AC_GD - 1) / smk::AC_GD;
    const dim3 grid(xt * ndg, (unsigned)std::min(fa.H, 65535));
    switch (U / 32) {
    case 1: hipLaunchKernelGGL(smk::k_ac_fused16<1>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 2: hipLaunchKernelGGL(smk::k_ac_fused16<2>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 3: hipLaunchKernelGGL(smk::k_ac_fused16<3>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 4: hipLaunchKernelGGL(smk::k_ac_fused16<4>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 5: hipLaunchKernelGGL(smk::k_ac_fused16<5>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 6: hipLaunchKernelGGL(smk::k_ac_fused16<6>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 7: hipLaunchKernelGGL(smk::k_ac_fused16<7>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 8: hipLaunchKernelGGL(smk::k_ac_fused16<8>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 9: hipLaunchKernelGGL(smk::k_ac_fused16<9>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 10: hipLaunchKernelGGL(smk::k_ac_fused16<10>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    case 11: hipLaunchKernelGGL(smk::k_ac_fused16<11>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    default: hipLaunchKernelGGL(smk::k_ac_fused16<12>, grid, dim3(smk::AC_BLOCK), 0, ctx->stream, fa); break;
    }
}

const char* const MCACC_BF16_BAD = "mcacc: a weight of hidden layer %d is not finite or overflows in bf16";

}  // namespace

int sm_mcacc_set_precision(sm_ctx* ctx, int precision)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (precision != SM_MCACC_F32 && precision != SM_MCACC_BF16)
        return fail(ctx, SM_E_ARG, "mcacc: precision %d (SM_MCACC_F32 or SM_MCACC_BF16)", precision);
    ctx->mcacc.precision = precision;
    return SM_OK;
}

int sm_mcacc_set_weights(sm_ctx* ctx, int L, const float* const* w, const float* const* b, int F, int U,
                         const float* const* fw, const float* const* fb)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = mcacc_check_conv(ctx, L, w, b)) != SM_OK) return rc;
    if ((rc = mcacc_check_fc(ctx, F, U, fw, fb)) != SM_OK) return rc;
    smk::AcFc fc;
    fc.F = F, fc.U = U;
    std::vector<float> wp(smk::ac_pack_conv_floats(L)), bp((size_t)L * smk::AC_CP), fp(fc.floats());
    smk::ac_pack_conv(L, w, b, wp.data(), bp.data());
    smk::ac_pack_fc(fc, fw, fb, fp.data());
    // the hidden matrices in bf16, rounded here once; a net bf16 cannot hold stays usable in f32
    const int bad = smk::ac_fc_bf16_bad(F, U, fw);
    if (bad && ctx->mcacc.precision == SM_MCACC_BF16) return fail(ctx, SM_E_ARG, MCACC_BF16_BAD, bad);
    std::vector<uint16_t> qp(std::max<size_t>(smk::ac_pack_fc_bf16_count(F, U), 8));
    if (!bad) smk::ac_pack_fc_bf16(F, U, fw, qp.data());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no queued layer still reads the old weights
    ctx->mcacc.L = 0;
    if ((rc = stage_in(ctx, {{ctx->mcacc.w, wp.data(), wp.size() * sizeof(float)},
                             {ctx->mcacc.b, bp.data(), bp.size() * sizeof(float)},
                             {ctx->mcacc.fc, fp.data(), fp.size() * sizeof(float)},
                             {ctx->mcacc.fc16, qp.data(), qp.size() * sizeof(uint16_t)}})) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the packed arrays live on this frame
    ctx->mcacc.L = L, ctx->mcacc.F = F, ctx->mcacc.U = U, ctx->mcacc.bf16_bad = bad;
    return SM_OK;
}

int sm_mcacc_features_device(sm_ctx* ctx, const uint8_t* d_gray, int n, size_t image_stride, int H, int W,
                             size_t row_stride, float* d_feat)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_gray || !d_feat) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    int rc;
    if ((rc = mcacc_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_strides(ctx, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mcacc_check_aligned(ctx, d_feat, "d_feat")) != SM_OK) return rc;
    if (H > 2 * 65535) return fail(ctx, SM_E_UNSUPPORTED, "mcacc: %d rows (at most 131070)", H);
    const int L = ctx->mcacc.L;
    if (L < 1) return fail(ctx, SM_E_ARG, "mcacc: no weights (sm_mcacc_set_weights comes first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned npix = (unsigned)H * (unsigned)W;
    const size_t fimg = (size_t)npix * smk::AC_C;
    auto& mc = ctx->mcacc;
    if ((rc = ensure(ctx, mc.sums, (size_t)n * 16)) != SM_OK) return rc;
    if ((rc = ensure(ctx, mc.tab, (size_t)n * 256 * sizeof(float))) != SM_OK) return rc;
    if (L > 1 && (rc = ensure(ctx, mc.ping, fimg * sizeof(float))) != SM_OK) return rc;
    if (L > 2 && (rc = ensure(ctx, mc.pong, fimg * sizeof(float))) != SM_OK) return rc;

    // the images' sums, the wait for them (a constant image is an error) and the host's tables, as
    // in sm_mccnn_features_device: the twin's table is this one by construction
    mc.sums_host.resize((size_t)n * 2);
    HIP_TRY(ctx, hipMemsetAsync(mc.sums.p, 0, (size_t)n * 16, ctx->stream));
    smk::AcSumArgs sa{d_gray, image_stride, row_stride, H, W, (unsigned long long*)mc.sums.p};
    const unsigned sblocks = std::min(256u, (npix + smk::AC_BLOCK * 16 - 1) / (smk::AC_BLOCK * 16));
    hipLaunchKernelGGL(smk::k_ac_sums, dim3(sblocks, n), dim3(smk::AC_BLOCK), 0, ctx->stream, sa);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(mc.sums_host.data(), mc.sums.p, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    mc.tab_host.resize((size_t)n * 256);
    for (int img = 0; img < n; img++)
        if (!smk::mc_table(mc.sums_host[2 * img], mc.sums_host[2 * img + 1], npix, mc.tab_host.data() + (size_t)img * 256))
            return fail(ctx, SM_E_ARG, "mcacc: image %d is constant (standard deviation 0)", img);
    HIP_TRY(ctx, hipMemcpyAsync(mc.tab.p, mc.tab_host.data(), (size_t)n * 256 * sizeof(float), hipMemcpyHostToDevice,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // tab_host is pageable and lives across calls

    const float* wp = (const float*)mc.w.p;
    const float* bp = (const float*)mc.b.p;
    const dim3 cgrid((W + smk::AC_TW - 1) / smk::AC_TW, (H + smk::AC_TH - 1) / smk::AC_TH);
    for (int img = 0; img < n; img++) {
        float* feat = d_feat + (size_t)img * fimg;
        auto dst = [&](int i) { return i == L - 1 ? feat : (i & 1) ? (float*)mc.pong.p : (float*)mc.ping.p; };
        smk::AcL0Args l0{d_gray + (size_t)img * image_stride, row_stride, H, W, (const float*)mc.tab.p + (size_t)img * 256,
                         wp, bp, dst(0)};
        hipLaunchKernelGGL(smk::k_ac_layer0, dim3((npix * smk::AC_Q + smk::AC_BLOCK - 1) / smk::AC_BLOCK),
                           dim3(smk::AC_BLOCK), 0, ctx->stream, l0);
        for (int i = 1; i < L; i++) {
            smk::AcConvArgs ca{dst(i - 1), dst(i), wp + smk::AC_W0 + (size_t)(i - 1) * smk::AC_WL,
                               bp + (size_t)i * smk::AC_CP, H, W};
            hipLaunchKernelGGL(smk::k_ac_conv, cgrid, dim3(smk::AC_BLOCK), 0, ctx->stream, ca);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mcacc_join_device(sm_ctx* ctx, const float* d_feat_a, const float* d_feat_b, int n, int H, int W, int D,
                         int min_disparity, int a_is_left, int raw, float* d_vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_feat_a || !d_feat_b || !d_vol) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    int rc;
    if ((rc = mcacc_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_planes(ctx, D)) != SM_OK) return rc;
    if ((rc = mcacc_check_aligned(ctx, d_feat_a, "d_feat_a")) != SM_OK) return rc;
    if ((rc = mcacc_check_aligned(ctx, d_feat_b, "d_feat_b")) != SM_OK) return rc;
    auto& mc = ctx->mcacc;
    if (mc.L < 1) return fail(ctx, SM_E_ARG, "mcacc: no weights (sm_mcacc_set_weights comes first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    smk::AcFc fc;
    fc.F = mc.F, fc.U = mc.U;
    const int F = fc.F, U = fc.U;
    const unsigned npix = (unsigned)H * (unsigned)W;
    const size_t cells = (size_t)D * npix, pbytes = (size_t)npix * U * sizeof(float);
    const bool bf16 = mc.precision == SM_MCACC_BF16;
    if (bf16 && mc.bf16_bad) return fail(ctx, SM_E_ARG, MCACC_BF16_BAD, mc.bf16_bad);
    if ((rc = ensure(ctx, mc.pa, pbytes)) != SM_OK) return rc;
    if ((rc = ensure(ctx, mc.pb, pbytes)) != SM_OK) return rc;

    // cells per pass: the scratch (one buffer, two with a U x U layer) takes at most a quarter of
    // what is free, counting what the context already holds for it; never sized from H W D
    // (precision "bf16" has no scratch and no chunks: one fused kernel per image)
    size_t chunk = (size_t)ctx->tune_mcacc_chunk;
    const int nscr = F > 1 ? 2 : 1;
    if (bf16) chunk = cells;
    if (!chunk) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        const size_t avail = (free_b + mc.scr[0].n + mc.scr[1].n) / 4;
        chunk = avail / ((size_t)nscr * U * sizeof(float));
        chunk = std::min(chunk, (size_t)1 << 20) & ~(size_t)(smk::AC_DM - 1);
        if (!chunk) return fail(ctx, SM_E_HIP, "mcacc: not enough free device memory for the scorer's scratch");
    }
    chunk = std::min(chunk, cells);
    for (int i = 0; i < nscr && !bf16; i++)
        if ((rc = ensure(ctx, mc.scr[i], chunk * U * sizeof(float))) != SM_OK) return rc;

    const float* fcp = (const float*)mc.fc.p;
    const int m = smk::mc_clamp_min_disparity(min_disparity, W, D);
    for (int img = 0; img < n; img++) {
        const float* fimg[2] = {d_feat_a + (size_t)img * npix * smk::AC_C, d_feat_b + (size_t)img * npix * smk::AC_C};
        float* proj[2] = {(float*)mc.pa.p, (float*)mc.pb.p};
        for (int side = 0; side < 2; side++) {
            const bool left = (side == 0) == (a_is_left != 0);
            mcacc_dense(ctx, fimg[side], fcp + (left ? fc.pl() : fc.pr()), left ? fcp + fc.bias(0) : nullptr, proj[side],
                        npix, smk::AC_C, U, false);
        }
        float* vol = d_vol + (size_t)img * cells;
        if (bf16) {
            smk::AcFusedArgs ua{proj[0], proj[1], (const uint16_t*)mc.fc16.p, fcp + fc.bias(0), fcp + fc.last(),
                                fcp + fc.bias(F), vol, H, W, D, F, m, raw != 0};
            mcacc_launch_fused16(ctx, ua, U);
            continue;
        }
        for (size_t c0 = 0; c0 < cells; c0 += chunk) {
            const unsigned nc = (unsigned)std::min(chunk, cells - c0);
            smk::AcCellArgs ha{proj[0], proj[1], (float*)mc.scr[0].p, c0, nc, H, W, U, m};
            const unsigned hthreads = nc * (unsigned)(U / 4);
            hipLaunchKernelGGL(smk::k_ac_h1, dim3((hthreads + smk::AC_BLOCK - 1) / smk::AC_BLOCK), dim3(smk::AC_BLOCK), 0,
                               ctx->stream, ha);
            for (int i = 1; i < F; i++)
                mcacc_dense(ctx, (const float*)mc.scr[(i - 1) & 1].p, fcp + fc.hid(i), fcp + fc.bias(i),
                            (float*)mc.scr[i & 1].p, nc, U, U, true);
            smk::AcFinalArgs fa{(const float*)mc.scr[(F - 1) & 1].p, fcp + fc.last(), fcp + fc.bias(F), vol, c0, nc, H, W, U,
                                m, raw != 0};
            hipLaunchKernelGGL(smk::k_ac_final, dim3((nc + smk::AC_BLOCK - 1) / smk::AC_BLOCK), dim3(smk::AC_BLOCK), 0,
                               ctx->stream, fa);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mcacc_volume_device(sm_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int n, size_t image_stride, int H,
                           int W, size_t row_stride, int D, int min_disparity, int a_is_left, int raw, float* d_vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_a || !d_b || !d_vol) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    int rc;
    if ((rc = mcacc_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_planes(ctx, D)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));  // ensure allocates
    const size_t fbytes = (size_t)n * H * W * smk::AC_C * sizeof(float);
    if ((rc = ensure(ctx, ctx->mcacc.fa, fbytes)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->mcacc.fb, fbytes)) != SM_OK) return rc;
    if ((rc = sm_mcacc_features_device(ctx, d_a, n, image_stride, H, W, row_stride, (float*)ctx->mcacc.fa.p)) != SM_OK) return rc;
    if ((rc = sm_mcacc_features_device(ctx, d_b, n, image_stride, H, W, row_stride, (float*)ctx->mcacc.fb.p)) != SM_OK) return rc;
    return sm_mcacc_join_device(ctx, (const float*)ctx->mcacc.fa.p, (const float*)ctx->mcacc.fb.p, n, H, W, D, min_disparity,
                                a_is_left, raw, d_vol);
}

int sm_mcacc_features(sm_ctx* ctx, const uint8_t* gray, int n, int H, int W, float* feat)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!gray || !feat) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    int rc;
    if ((rc = mcacc_check_images(ctx, n, H, W)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ibytes = (size_t)n * H * W, fbytes = ibytes * smk::AC_C * sizeof(float);
    if ((rc = stage_in(ctx, {{ctx->mcacc.in_a, gray, ibytes}, {ctx->mcacc.fa, nullptr, fbytes}})) != SM_OK) return rc;
    if ((rc = sm_mcacc_features_device(ctx, (const uint8_t*)ctx->mcacc.in_a.p, n, (size_t)H * W, H, W, W,
                                       (float*)ctx->mcacc.fa.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->mcacc.fa, feat, fbytes}});
}

int sm_mcacc_join(sm_ctx* ctx, const float* feat_a, const float* feat_b, int n, int H, int W, int D, int min_disparity,
                  int a_is_left, int raw, float* vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!feat_a || !feat_b || !vol) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    int rc;
    if ((rc = mcacc_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_planes(ctx, D)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t fbytes = (size_t)n * H * W * smk::AC_C * sizeof(float), vbytes = (size_t)n * D * H * W * sizeof(float);
    if ((rc = stage_in(ctx, {{ctx->mcacc.fa, feat_a, fbytes}, {ctx->mcacc.fb, feat_b, fbytes}, {ctx->mcacc.vol, nullptr, vbytes}})) !=
        SM_OK)
        return rc;
    if ((rc = sm_mcacc_join_device(ctx, (const float*)ctx->mcacc.fa.p, (const float*)ctx->mcacc.fb.p, n, H, W, D, min_disparity,
                                   a_is_left, raw, (float*)ctx->mcacc.vol.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->mcacc.vol, vol, vbytes}});
}

int sm_mcacc_volume(sm_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D, int min_disparity,
                    int a_is_left, int raw, float* vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!a || !b || !vol) return fail(ctx, SM_E_ARG, "mcacc: a required pointer is NULL");
    int rc;
    if ((rc = mcacc_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_planes(ctx, D)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ibytes = (size_t)n * H * W, vbytes = (size_t)n * D * H * W * sizeof(float);
    if ((rc = stage_in(ctx, {{ctx->mcacc.in_a, a, ibytes}, {ctx->mcacc.in_b, b, ibytes}, {ctx->mcacc.vol, nullptr, vbytes}})) != SM_OK)
        return rc;
    if ((rc = sm_mcacc_volume_device(ctx, (const uint8_t*)ctx->mcacc.in_a.p, (const uint8_t*)ctx->mcacc.in_b.p, n, (size_t)H * W,
                                     H, W, W, D, min_disparity, a_is_left, raw, (float*)ctx->mcacc.vol.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->mcacc.vol, vol, vbytes}});
}

int sm_mcacc_features_host(int L, const float* const* w, const float* const* b, const uint8_t* gray, int n,
                           size_t image_stride, int H, int W, size_t row_stride, float* feat)
{
    int rc;
    if ((rc = mcacc_check_conv(nullptr, L, w, b)) != SM_OK) return rc;
    if (!gray || !feat) return fail(nullptr, SM_E_ARG, "mcacc: a required pointer is NULL");
    if ((rc = mcacc_check_images(nullptr, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_strides(nullptr, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    std::vector<float> wp(smk::ac_pack_conv_floats(L)), bp((size_t)L * smk::AC_CP);
    smk::ac_pack_conv(L, w, b, wp.data(), bp.data());
    const int bad = smk::mcacc_features_host(L, wp.data(), bp.data(), gray, n, image_stride, H, W, row_stride, feat);
    if (bad >= 0) return fail(nullptr, SM_E_ARG, "mcacc: image %d is constant (standard deviation 0)", bad);
    return SM_OK;
}

int sm_mcacc_join_host(int F, int U, const float* const* fw, const float* const* fb, const float* feat_a,
                       const float* feat_b, int n, int H, int W, int D, int min_disparity, int a_is_left, int raw,
                       float* vol)
{
    int rc;
    if ((rc = mcacc_check_fc(nullptr, F, U, fw, fb)) != SM_OK) return rc;
    if (!feat_a || !feat_b || !vol) return fail(nullptr, SM_E_ARG, "mcacc: a required pointer is NULL");
    if ((rc = mcacc_check_images(nullptr, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_planes(nullptr, D)) != SM_OK) return rc;
    smk::AcFc fc;
    fc.F = F, fc.U = U;
    std::vector<float> fp(fc.floats());
    smk::ac_pack_fc(fc, fw, fb, fp.data());
    smk::mcacc_join_host(fc, fp.data(), feat_a, feat_b, n, H, W, D, min_disparity, a_is_left != 0, raw != 0, vol);
    return SM_OK;
}

int sm_mcacc_join_host_bf16(int F, int U, const float* const* fw, const float* const* fb, const float* feat_a,
                            const float* feat_b, int n, int H, int W, int D, int min_disparity, int a_is_left, int raw,
                            float* vol)
{
    int rc;
    if ((rc = mcacc_check_fc(nullptr, F, U, fw, fb)) != SM_OK) return rc;
    if (!feat_a || !feat_b || !vol) return fail(nullptr, SM_E_ARG, "mcacc: a required pointer is NULL");
    if ((rc = mcacc_check_images(nullptr, n, H, W)) != SM_OK) return rc;
    if ((rc = mcacc_check_planes(nullptr, D)) != SM_OK) return rc;
    const int bad = smk::ac_fc_bf16_bad(F, U, fw);
    if (bad) return fail(nullptr, SM_E_ARG, MCACC_BF16_BAD, bad);
    smk::AcFc fc;
    fc.F = F, fc.U = U;
    std::vector<float> fp(fc.floats());
    smk::ac_pack_fc(fc, fw, fb, fp.data());
    smk::ac_round_fc(fc, fp.data());
    smk::mcacc_join_host(fc, fp.data(), feat_a, feat_b, n, H, W, D, min_disparity, a_is_left != 0, raw != 0, vol, true);
    return SM_OK;
}

int sm_mcacc_bf16_host(const float* x, size_t n, uint16_t* out)
{
    if (!x || !out) return fail(nullptr, SM_E_ARG, "mcacc: a required pointer is NULL");
    for (size_t i = 0; i < n; i++) out[i] = smk::ac_bf16(x[i]);
    return SM_OK;
}

int sm_mcacc_sigmoid_host(const float* z, size_t n, float* s)
{
    if (!z || !s) return fail(nullptr, SM_E_ARG, "mcacc: a required pointer is NULL");
    for (size_t i = 0; i < n; i++) s[i] = smk::ac_sigmoid(z[i]);
    return SM_OK;
}

}  // extern "C"
