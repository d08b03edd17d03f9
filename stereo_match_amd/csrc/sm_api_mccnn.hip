// sm_api_mccnn.hip — C-ABI of the MC-CNN fast matching cost (sm_mccnn.hpp).  The only unit with these kernels.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sm_ctx.hpp"
#include "sm_mccnn.hpp"

extern "C" {

// ---- MC-CNN matching cost (sm_mccnn.hpp)
namespace {

int mccnn_check_images(sm_ctx* ctx, int n, int H, int W)
{
    if (n < 1 || n > 65535) return fail(ctx, SM_E_ARG, "mccnn: %d images (1 .. 65535)", n);
    if (H < 1 || W < 1) return fail(ctx, SM_E_ARG, "mccnn: empty image (%dx%d)", W, H);
    if ((size_t)H * (size_t)W > smk::MC_MAXPIX)
        return fail(ctx, SM_E_UNSUPPORTED, "mccnn: image %dx%d has 2^24 pixels or more", W, H);
    return SM_OK;
}

int mccnn_check_strides(sm_ctx* ctx, int n, size_t image_stride, int H, int W, size_t row_stride)
{
    if (row_stride < (size_t)W) return fail(ctx, SM_E_ARG, "mccnn: row_stride %zu smaller than a row (%d)", row_stride, W);
    if (n > 1 && image_stride < (size_t)(H - 1) * row_stride + (size_t)W)
        return fail(ctx, SM_E_ARG, "mccnn: image_stride %zu smaller than one image", image_stride);
    return SM_OK;
}

// the kernels read and write feature maps 16 bytes at a time
int mccnn_check_aligned(sm_ctx* ctx, const void* p, const char* what)
{
    if ((uintptr_t)p & 15) return fail(ctx, SM_E_ARG, "mccnn: %s is not 16-byte aligned", what);
    return SM_OK;
}

int mccnn_check_planes(sm_ctx* ctx, int D)
{
    if (D < 1 || D > smk::MC_MAXD) return fail(ctx, SM_E_ARG, "mccnn: %d disparity planes (1 .. %d)", D, smk::MC_MAXD);
    return SM_OK;
}

int mccnn_check_weights(sm_ctx* ctx, int L, const float* const* w, const float* const* b)
{
    if (L < 1 || L > smk::MC_MAXL) return fail(ctx, SM_E_ARG, "mccnn: %d layers (1 .. %d)", L, smk::MC_MAXL);
    if (!w || !b) return fail(ctx, SM_E_ARG, "mccnn: a required pointer is NULL");
    for (int i = 0; i < L; i++)
        if (!w[i] || !b[i]) return fail(ctx, SM_E_ARG, "mccnn: weights or biases of layer %d are NULL", i);
    return SM_OK;
}

}  // namespace

int sm_mccnn_set_weights(sm_ctx* ctx, int L, const float* const* w, const float* const* b)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = mccnn_check_weights(ctx, L, w, b)) != SM_OK) return rc;
    std::vector<float> wp(smk::mc_pack_floats(L)), bp((size_t)L * smk::MC_C);
    smk::mc_pack_weights(L, w, wp.data());
    for (int i = 0; i < L; i++) std::memcpy(bp.data() + (size_t)i * smk::MC_C, b[i], smk::MC_C * sizeof(float));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no queued layer still reads the old weights
    ctx->mccnn.L = 0;
    if ((rc = stage_in(ctx, {{ctx->mccnn.w, wp.data(), wp.size() * sizeof(float)},
                             {ctx->mccnn.b, bp.data(), bp.size() * sizeof(float)}})) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // wp and bp live on this frame
    ctx->mccnn.L = L;
    return SM_OK;
}

int sm_mccnn_features_device(sm_ctx* ctx, const uint8_t* d_gray, int n, size_t image_stride, int H, int W,
                             size_t row_stride, float* d_feat)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_gray || !d_feat) return fail(ctx, SM_E_ARG, "mccnn: a required pointer is NULL");
    int rc;
    if ((rc = mccnn_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mccnn_check_strides(ctx, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mccnn_check_aligned(ctx, d_feat, "d_feat")) != SM_OK) return rc;
    // the convolutions' grid has a workgroup row per MC_TH image rows, at most 65535 of them
    if (H > smk::MC_TH * 65535) return fail(ctx, SM_E_UNSUPPORTED, "mccnn: %d rows (at most 524280)", H);
    const int L = ctx->mccnn.L;
    if (L < 1) return fail(ctx, SM_E_ARG, "mccnn: no weights (sm_mccnn_set_weights comes first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned npix = (unsigned)H * (unsigned)W;
    const size_t fimg = (size_t)npix * smk::MC_C;
    auto& mc = ctx->mccnn;
    if ((rc = ensure(ctx, mc.sums, (size_t)n * 16)) != SM_OK) return rc;
    if ((rc = ensure(ctx, mc.tab, (size_t)n * 256 * sizeof(float))) != SM_OK) return rc;
    if (L > 1 && (rc = ensure(ctx, mc.ping, fimg * sizeof(float))) != SM_OK) return rc;
    if (L > 2 && (rc = ensure(ctx, mc.pong, fimg * sizeof(float))) != SM_OK) return rc;

    // the images' sums, the first wait of this entry point (a constant image is an error), and the
    // tables: the host's float64 expression, so the twin's table is this one by construction
    mc.sums_host.resize((size_t)n * 2);
    HIP_TRY(ctx, hipMemsetAsync(mc.sums.p, 0, (size_t)n * 16, ctx->stream));
    smk::McSumArgs sa{d_gray, image_stride, row_stride, H, W, (unsigned long long*)mc.sums.p};
    const unsigned sblocks = std::min(256u, (npix + smk::MC_BLOCK * 16 - 1) / (smk::MC_BLOCK * 16));
    hipLaunchKernelGGL(smk::k_mc_sums, dim3(sblocks, n), dim3(smk::MC_BLOCK), 0, ctx->stream, sa);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(mc.sums_host.data(), mc.sums.p, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    mc.tab_host.resize((size_t)n * 256);
    for (int img = 0; img < n; img++)
        if (!smk::mc_table(mc.sums_host[2 * img], mc.sums_host[2 * img + 1], npix, mc.tab_host.data() + (size_t)img * 256))
            return fail(ctx, SM_E_ARG, "mccnn: image %d is constant (standard deviation 0)", img);
    HIP_TRY(ctx, hipMemcpyAsync(mc.tab.p, mc.tab_host.data(), (size_t)n * 256 * sizeof(float), hipMemcpyHostToDevice,
                                ctx->stream));
    // tab_host is pageable and lives across calls: the copy has left it before this call goes on, whatever
    // stream the next call runs on.  sums and tab are then only touched by work queued on this stream;
    // a caller that moves the context to another stream orders the two streams itself, as for every buffer
    // of the context.
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    const float* wp = (const float*)mc.w.p;
    const float* bp = (const float*)mc.b.p;
    const dim3 cgrid((W + smk::MC_TW - 1) / smk::MC_TW, (H + smk::MC_TH - 1) / smk::MC_TH);
    for (int img = 0; img < n; img++) {
        float* feat = d_feat + (size_t)img * fimg;
        auto dst = [&](int i) { return i == L - 1 ? feat : (i & 1) ? (float*)mc.pong.p : (float*)mc.ping.p; };
        smk::McL0Args l0{d_gray + (size_t)img * image_stride, row_stride, H, W, (const float*)mc.tab.p + (size_t)img * 256,
                         wp, bp, dst(0), L > 1};
        hipLaunchKernelGGL(smk::k_mc_layer0, dim3((npix * 16 + smk::MC_BLOCK - 1) / smk::MC_BLOCK), dim3(smk::MC_BLOCK), 0,
                           ctx->stream, l0);
        if (L == 1) {
            smk::McUnitArgs ua{feat, npix};
            hipLaunchKernelGGL(smk::k_mc_unit, dim3((npix + smk::MC_BLOCK - 1) / smk::MC_BLOCK), dim3(smk::MC_BLOCK), 0,
                               ctx->stream, ua);
        }
        for (int i = 1; i < L; i++) {
            smk::McConvArgs ca{dst(i - 1), dst(i), wp + smk::MC_W0 + (size_t)(i - 1) * smk::MC_WL, bp + (size_t)i * smk::MC_C,
                               H, W};
            if (i == L - 1)
                hipLaunchKernelGGL(smk::k_mc_conv<true>, cgrid, dim3(smk::MC_BLOCK), 0, ctx->stream, ca);
            else
                hipLaunchKernelGGL(smk::k_mc_conv<false>, cgrid, dim3(smk::MC_BLOCK), 0, ctx->stream, ca);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mccnn_join_device(sm_ctx* ctx, const float* d_feat_a, const float* d_feat_b, int n, int H, int W, int D,
                         int min_disparity, float* d_vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_feat_a || !d_feat_b || !d_vol) return fail(ctx, SM_E_ARG, "mccnn: a required pointer is NULL");
    int rc;
    if ((rc = mccnn_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mccnn_check_planes(ctx, D)) != SM_OK) return rc;
    if (H > 65535) return fail(ctx, SM_E_UNSUPPORTED, "mccnn: %d rows (at most 65535)", H);
    if ((rc = mccnn_check_aligned(ctx, d_feat_a, "d_feat_a")) != SM_OK) return rc;
    if ((rc = mccnn_check_aligned(ctx, d_feat_b, "d_feat_b")) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    smk::McJoinArgs ja{d_feat_a, d_feat_b, d_vol, H, W, D, smk::mc_clamp_min_disparity(min_disparity, W, D)};
    hipLaunchKernelGGL(smk::k_mc_join, dim3((W + smk::MC_JX - 1) / smk::MC_JX, H, n), dim3(smk::MC_JX), 0, ctx->stream, ja);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mccnn_volume_device(sm_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int n, size_t image_stride, int H,
                           int W, size_t row_stride, int D, int min_disparity, float* d_vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_a || !d_b || !d_vol) return fail(ctx, SM_E_ARG, "mccnn: a required pointer is NULL");
    int rc;
    if ((rc = mccnn_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mccnn_check_planes(ctx, D)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));  // ensure allocates
    const size_t fbytes = (size_t)n * H * W * smk::MC_C * sizeof(float);
    if ((rc = ensure(ctx, ctx->mccnn.fa, fbytes)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->mccnn.fb, fbytes)) != SM_OK) return rc;
    if ((rc = sm_mccnn_features_device(ctx, d_a, n, image_stride, H, W, row_stride, (float*)ctx->mccnn.fa.p)) != SM_OK) return rc;
    if ((rc = sm_mccnn_features_device(ctx, d_b, n, image_stride, H, W, row_stride, (float*)ctx->mccnn.fb.p)) != SM_OK) return rc;
    return sm_mccnn_join_device(ctx, (const float*)ctx->mccnn.fa.p, (const float*)ctx->mccnn.fb.p, n, H, W, D, min_disparity,
                                d_vol);
}

int sm_mccnn_features(sm_ctx* ctx, const uint8_t* gray, int n, int H, int W, float* feat)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!gray || !feat) return fail(ctx, SM_E_ARG, "mccnn: a required pointer is NULL");
    int rc;
    if ((rc = mccnn_check_images(ctx, n, H, W)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ibytes = (size_t)n * H * W, fbytes = ibytes * smk::MC_C * sizeof(float);
    if ((rc = stage_in(ctx, {{ctx->mccnn.in_a, gray, ibytes}, {ctx->mccnn.fa, nullptr, fbytes}})) != SM_OK) return rc;
    if ((rc = sm_mccnn_features_device(ctx, (const uint8_t*)ctx->mccnn.in_a.p, n, (size_t)H * W, H, W, W,
                                       (float*)ctx->mccnn.fa.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->mccnn.fa, feat, fbytes}});
}

int sm_mccnn_join(sm_ctx* ctx, const float* feat_a, const float* feat_b, int n, int H, int W, int D, int min_disparity,
                  float* vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!feat_a || !feat_b || !vol) return fail(ctx, SM_E_ARG, "mccnn: a required pointer is NULL");
    int rc;
    if ((rc = mccnn_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mccnn_check_planes(ctx, D)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t fbytes = (size_t)n * H * W * smk::MC_C * sizeof(float), vbytes = (size_t)n * D * H * W * sizeof(float);
    if ((rc = stage_in(ctx, {{ctx->mccnn.fa, feat_a, fbytes}, {ctx->mccnn.fb, feat_b, fbytes}, {ctx->mccnn.vol, nullptr, vbytes}})) !=
        SM_OK)
        return rc;
    if ((rc = sm_mccnn_join_device(ctx, (const float*)ctx->mccnn.fa.p, (const float*)ctx->mccnn.fb.p, n, H, W, D, min_disparity,
                                   (float*)ctx->mccnn.vol.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->mccnn.vol, vol, vbytes}});
}

int sm_mccnn_volume(sm_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D, int min_disparity,
                    float* vol)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!a || !b || !vol) return fail(ctx, SM_E_ARG, "mccnn: a required pointer is NULL");
    int rc;
    if ((rc = mccnn_check_images(ctx, n, H, W)) != SM_OK) return rc;
    if ((rc = mccnn_check_planes(ctx, D)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ibytes = (size_t)n * H * W, vbytes = (size_t)n * D * H * W * sizeof(float);
    if ((rc = stage_in(ctx, {{ctx->mccnn.in_a, a, ibytes}, {ctx->mccnn.in_b, b, ibytes}, {ctx->mccnn.vol, nullptr, vbytes}})) != SM_OK)
        return rc;
    if ((rc = sm_mccnn_volume_device(ctx, (const uint8_t*)ctx->mccnn.in_a.p, (const uint8_t*)ctx->mccnn.in_b.p, n, (size_t)H * W,
                                     H, W, W, D, min_disparity, (float*)ctx->mccnn.vol.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->mccnn.vol, vol, vbytes}});
}

int sm_mccnn_features_host(int L, const float* const* w, const float* const* b, const uint8_t* gray, int n,
                           size_t image_stride, int H, int W, size_t row_stride, float* feat)
{
    int rc;
    if ((rc = mccnn_check_weights(nullptr, L, w, b)) != SM_OK) return rc;
    if (!gray || !feat) return fail(nullptr, SM_E_ARG, "mccnn: a required pointer is NULL");
    if ((rc = mccnn_check_images(nullptr, n, H, W)) != SM_OK) return rc;
    if ((rc = mccnn_check_strides(nullptr, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    std::vector<float> wp(smk::mc_pack_floats(L)), bp((size_t)L * smk::MC_C);
    smk::mc_pack_weights(L, w, wp.data());
    for (int i = 0; i < L; i++) std::memcpy(bp.data() + (size_t)i * smk::MC_C, b[i], smk::MC_C * sizeof(float));
    const int bad = smk::mccnn_features_host(L, wp.data(), bp.data(), gray, n, image_stride, H, W, row_stride, feat);
    if (bad >= 0) return fail(nullptr, SM_E_ARG, "mccnn: image %d is constant (standard deviation 0)", bad);
    return SM_OK;
}

int sm_mccnn_join_host(const float* feat_a, const float* feat_b, int n, int H, int W, int D, int min_disparity, float* vol)
{
    if (!feat_a || !feat_b || !vol) return fail(nullptr, SM_E_ARG, "mccnn: a required pointer is NULL");
    int rc;
    if ((rc = mccnn_check_images(nullptr, n, H, W)) != SM_OK) return rc;
    if ((rc = mccnn_check_planes(nullptr, D)) != SM_OK) return rc;
    smk::mccnn_join_host(feat_a, feat_b, n, H, W, D, min_disparity, vol);
    return SM_OK;
}

}  // extern "C"
