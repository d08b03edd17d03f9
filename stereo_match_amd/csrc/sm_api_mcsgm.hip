// sm_api_mcsgm.hip — C-ABI of MC-CNN's stereo method (sm_mcsgm.hpp).  The only unit with these kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#define SM_MCCNN_NO_KERNELS 1  // sm_mccnn.hpp: its host functions only (its kernels live in sm_api_mccnn.hip)
#include "sm_ctx.hpp"
#include "sm_mcsgm.hpp"

// ---- MC-CNN's stereo method (sm_mcsgm.hpp)
namespace {

int mcsgm_check_shape(sm_ctx* ctx, int n, int H, int W, int D)
{
    if (n < 1 || n > 65535) return fail(ctx, SM_E_ARG, "mcsgm: %d images (1 .. 65535)", n);
    if (H < 1 || W < 1) return fail(ctx, SM_E_ARG, "mcsgm: empty image (%dx%d)", W, H);
    if ((size_t)H * (size_t)W > smk::MC_MAXPIX)
        return fail(ctx, SM_E_UNSUPPORTED, "mcsgm: image %dx%d has 2^24 pixels or more", W, H);
    if (D < 1 || D > smk::MC_MAXD) return fail(ctx, SM_E_ARG, "mcsgm: %d disparity planes (1 .. %d)", D, smk::MC_MAXD);
    return SM_OK;
}

int mcsgm_check_strides(sm_ctx* ctx, int n, size_t image_stride, int H, int W, size_t row_stride)
{
    if (row_stride < (size_t)W) return fail(ctx, SM_E_ARG, "mcsgm: row_stride %zu smaller than a row (%d)", row_stride, W);
    if (n > 1 && image_stride < (size_t)(H - 1) * row_stride + (size_t)W)
        return fail(ctx, SM_E_ARG, "mcsgm: image_stride %zu smaller than one image", image_stride);
    return SM_OK;
}

bool positive(float v) { return std::isfinite(v) && v > 0.0f; }

int mcsgm_check_sgm(sm_ctx* ctx, const sm_mcsgm_params* p, int W)
{
    if (!p) return fail(ctx, SM_E_ARG, "mcsgm: params is NULL");
    if (!std::isfinite(p->pi1) || p->pi1 < 0.0f || !std::isfinite(p->pi2) || p->pi2 < 0.0f)
        return fail(ctx, SM_E_ARG, "mcsgm: pi1 and pi2 must be finite and not negative");
    if (!positive(p->sgm_q1) || !positive(p->sgm_q2) || !positive(p->sgm_v) || !positive(p->sgm_d))
        return fail(ctx, SM_E_ARG, "mcsgm: sgm_q1, sgm_q2, sgm_v and sgm_d must be finite and positive");
    if (p->sgm_i < 1 || p->sgm_i > 16) return fail(ctx, SM_E_ARG, "mcsgm: sgm_i %d (1 .. 16)", p->sgm_i);
    if (W > smk::MCS_MAXW) return fail(ctx, SM_E_UNSUPPORTED, "mcsgm: %d columns (at most %d)", W, smk::MCS_MAXW);
    return SM_OK;
}

int mcsgm_check_disparity(sm_ctx* ctx, const sm_mcsgm_params* p, int D, int m)
{
    if (!p) return fail(ctx, SM_E_ARG, "mcsgm: params is NULL");
    if (!positive(p->blur_sigma) || !positive(p->blur_t))
        return fail(ctx, SM_E_ARG, "mcsgm: blur_sigma and blur_t must be finite and positive");
    if (p->blur_sigma > (float)smk::MCS_MAXR || smk::mcs_blur_radius(p->blur_sigma) > smk::MCS_MAXR)
        return fail(ctx, SM_E_UNSUPPORTED, "mcsgm: blur_sigma %g gives a window radius above %d", (double)p->blur_sigma, smk::MCS_MAXR);
    if (m < -smk::MCS_MAXOFF || m > smk::MCS_MAXOFF - D)
        return fail(ctx, SM_E_ARG, "mcsgm: min_disparity %d with %d planes leaves [-2^23, 2^23]", m, D);
    return SM_OK;
}

smk::McsPen penalties(const sm_mcsgm_params* p) { return smk::mcs_penalties(p->pi1, p->pi2, p->sgm_q1, p->sgm_q2, p->sgm_v, p->sgm_d); }

}  // namespace

// (declared in sm_ctx.hpp: sm_api_mccbca.hip calls it too)
// normalised float32 images of `sets` groups of n images each into dst[s] ([n][H][W]): the images'
// sums, one wait for them, the tables from the host's float64 expression (the twin's by
// construction), one upload
int mcsgm_normalise(sm_ctx* ctx, int sets, const uint8_t* const* d_gray, int n, size_t image_stride, int H, int W,
                    size_t row_stride, DevBuf* const* dst)
{
    auto& mc = ctx->mcsgm;
    const int total = sets * n;
    const unsigned npix = (unsigned)H * (unsigned)W;
    int rc;
    if ((rc = ensure(ctx, mc.sums, (size_t)total * 16)) != SM_OK) return rc;
    if ((rc = ensure(ctx, mc.tab, (size_t)total * 256 * sizeof(float))) != SM_OK) return rc;
    for (int s = 0; s < sets; s++)
        if ((rc = ensure(ctx, *dst[s], (size_t)n * npix * sizeof(float))) != SM_OK) return rc;
    mc.sums_host.resize((size_t)total * 2);
    HIP_TRY(ctx, hipMemsetAsync(mc.sums.p, 0, (size_t)total * 16, ctx->stream));
    const unsigned sblocks = std::min(256u, (npix + smk::MCS_BLOCK * 16 - 1) / (smk::MCS_BLOCK * 16));
    for (int s = 0; s < sets; s++) {
        smk::McsSumArgs sa{d_gray[s], image_stride, row_stride, H, W, (unsigned long long*)mc.sums.p + (size_t)s * n * 2};
        hipLaunchKernelGGL(smk::k_mcs_sums, dim3(sblocks, n), dim3(smk::MCS_BLOCK), 0, ctx->stream, sa);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(mc.sums_host.data(), mc.sums.p, (size_t)total * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    mc.tab_host.resize((size_t)total * 256);
    for (int i = 0; i < total; i++) smk::mcs_table(mc.sums_host[2 * i], mc.sums_host[2 * i + 1], npix, mc.tab_host.data() + (size_t)i * 256);
    HIP_TRY(ctx, hipMemcpyAsync(mc.tab.p, mc.tab_host.data(), (size_t)total * 256 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // tab_host is pageable and lives across calls
    for (int s = 0; s < sets; s++)
        for (int img = 0; img < n; img++) {
            smk::McsNormArgs na{d_gray[s] + (size_t)img * image_stride, row_stride, H, W,
                                (const float*)mc.tab.p + ((size_t)s * n + img) * 256, (float*)dst[s]->p + (size_t)img * npix};
            hipLaunchKernelGGL(smk::k_mcs_norm, dim3((npix + smk::MCS_BLOCK - 1) / smk::MCS_BLOCK), dim3(smk::MCS_BLOCK), 0, ctx->stream, na);
        }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

namespace {

void launch_horz(sm_ctx* ctx, const smk::McsAggArgs& a)
{
    const int nj = a.D <= 64 ? 1 : a.D <= 128 ? 2 : 4;
    const size_t lds = ((size_t)64 * nj * smk::MCS_HS + 2 * ((size_t)a.W + 1)) * sizeof(float);
    if (nj == 1)
        hipLaunchKernelGGL(smk::k_mcs_horz<1>, dim3(a.H), dim3(64), lds, ctx->stream, a);
    else if (nj == 2)
        hipLaunchKernelGGL(smk::k_mcs_horz<2>, dim3(a.H), dim3(64), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL(smk::k_mcs_horz<4>, dim3(a.H), dim3(64), lds, ctx->stream, a);
}

}  // namespace

extern "C" {

int sm_mcsgm_default_params(sm_mcsgm_params* out)
{
    if (!out) return fail(nullptr, SM_E_ARG, "mcsgm: out is NULL");
    *out = sm_mcsgm_params{4.0f, 55.72f, 3.0f, 2.5f, 1.5f, 0.02f, 1, 7.74f, 5.0f};
    return SM_OK;
}

int sm_mcsgm_aggregate_device(sm_ctx* ctx, const float* d_vol, const uint8_t* d_a, const uint8_t* d_b, int n,
                              size_t image_stride, int H, int W, size_t row_stride, int D, int min_disparity,
                              const sm_mcsgm_params* params, float* d_agg)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_vol || !d_a || !d_b || !d_agg) return fail(ctx, SM_E_ARG, "mcsgm: a required pointer is NULL");
    int rc;
    if ((rc = mcsgm_check_shape(ctx, n, H, W, D)) != SM_OK) return rc;
    if ((rc = mcsgm_check_strides(ctx, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mcsgm_check_sgm(ctx, params, W)) != SM_OK) return rc;
    const size_t npix = (size_t)H * W, cells = npix * D;
    if (d_agg < d_vol + (size_t)n * cells && d_vol < d_agg + (size_t)n * cells)
        return fail(ctx, SM_E_ARG, "mcsgm: the aggregated volume overlaps the input volume");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& mc = ctx->mcsgm;
    const int iters = params->sgm_i;
    if ((rc = ensure(ctx, mc.l2, cells * sizeof(float))) != SM_OK) return rc;
    if ((rc = ensure(ctx, mc.l3, cells * sizeof(float))) != SM_OK) return rc;
    if (iters > 1 && (rc = ensure(ctx, mc.iter, cells * sizeof(float))) != SM_OK) return rc;
    const uint8_t* gray[2] = {d_a, d_b};
    DevBuf* norm[2] = {&mc.ta, &mc.tb};
    if ((rc = mcsgm_normalise(ctx, 2, gray, n, image_stride, H, W, row_stride, norm)) != SM_OK) return rc;

    const smk::McsPen pen = penalties(params);
    const int m = smk::mc_clamp_min_disparity(min_disparity, W, D);
    for (int img = 0; img < n; img++) {
        const float* src = d_vol + (size_t)img * cells;
        float* out = d_agg + (size_t)img * cells;
        for (int it = 0; it < iters; it++) {
            float* dst = (iters - 1 - it) % 2 == 0 ? out : (float*)mc.iter.p;
            smk::McsAggArgs a{src, (const float*)mc.ta.p + (size_t)img * npix, (const float*)mc.tb.p + (size_t)img * npix,
                              dst, (float*)mc.l2.p, (float*)mc.l3.p, H, W, D, m, pen};
            hipLaunchKernelGGL(smk::k_mcs_vert, dim3((W + smk::MCS_VX - 1) / smk::MCS_VX, 2), dim3(smk::MCS_BLOCK), 0, ctx->stream, a);
            launch_horz(ctx, a);
            src = dst;
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mcsgm_disparity_device(sm_ctx* ctx, const float* d_agg_l, const float* d_agg_r, const uint8_t* d_a, int n,
                              size_t image_stride, int H, int W, size_t row_stride, int D, int min_disparity,
                              const sm_mcsgm_params* params, float* d_disp, const sm_mcsgm_stages* d_stages)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_agg_l || !d_agg_r || !d_a || !d_disp) return fail(ctx, SM_E_ARG, "mcsgm: a required pointer is NULL");
    int rc;
    if ((rc = mcsgm_check_shape(ctx, n, H, W, D)) != SM_OK) return rc;
    if ((rc = mcsgm_check_strides(ctx, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mcsgm_check_disparity(ctx, params, D, min_disparity)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& mc = ctx->mcsgm;
    const size_t npix = (size_t)H * W, cells = npix * D;
    const sm_mcsgm_stages none{};
    const sm_mcsgm_stages& st = d_stages ? *d_stages : none;
    struct { DevBuf& buf; const void* given; } maps[6] = {{mc.wta_l, st.wta_left}, {mc.wta_r, st.wta_right}, {mc.status, st.status},
                                                          {mc.filled, st.filled}, {mc.sub, st.subpixel}, {mc.med, st.median}};
    void* mp[6];
    for (int i = 0; i < 6; i++) {
        if (!maps[i].given && (rc = ensure(ctx, maps[i].buf, (size_t)n * npix * 4)) != SM_OK) return rc;
        mp[i] = maps[i].given ? const_cast<void*>(maps[i].given) : maps[i].buf.p;
    }
    const uint8_t* gray[1] = {d_a};
    DevBuf* norm[1] = {&mc.ta};
    if ((rc = mcsgm_normalise(ctx, 1, gray, n, image_stride, H, W, row_stride, norm)) != SM_OK) return rc;

    uint32_t sigma_bits;
    std::memcpy(&sigma_bits, &params->blur_sigma, 4);
    if (mc.R < 0 || sigma_bits != mc.sigma_bits) {
        const int R = smk::mcs_blur_radius(params->blur_sigma);
        const size_t nw = (size_t)(2 * R + 1) * (2 * R + 1);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no queued filter still reads the old weights
        mc.R = -1;
        mc.w_host.resize(nw);
        smk::mcs_blur_weights(params->blur_sigma, R, mc.w_host.data());
        if ((rc = ensure(ctx, mc.w, nw * sizeof(float))) != SM_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(mc.w.p, mc.w_host.data(), nw * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        mc.R = R, mc.sigma_bits = sigma_bits;
    }

    const dim3 grid((unsigned)((npix + smk::MCS_BLOCK - 1) / smk::MCS_BLOCK)), block(smk::MCS_BLOCK);
    const size_t wbytes = (size_t)(2 * mc.R + 1) * (2 * mc.R + 1) * sizeof(float);
    for (int img = 0; img < n; img++) {
        const size_t o = (size_t)img * npix;
        smk::McsDispArgs a{d_agg_l + (size_t)img * cells, d_agg_r + (size_t)img * cells, (const float*)mc.ta.p + o,
                           (const float*)mc.w.p, H, W, D, min_disparity, mc.R, params->blur_t,
                           smk::McsMaps{(int*)mp[0] + o, (int*)mp[1] + o, (int*)mp[2] + o, (int*)mp[3] + o, (float*)mp[4] + o,
                                        (float*)mp[5] + o, d_disp + o}};
        hipLaunchKernelGGL(smk::k_mcs_wta, grid, block, 0, ctx->stream, a);
        hipLaunchKernelGGL(smk::k_mcs_status, grid, block, 0, ctx->stream, a);
        hipLaunchKernelGGL(smk::k_mcs_fill, grid, block, 0, ctx->stream, a);
        hipLaunchKernelGGL(smk::k_mcs_subpixel, grid, block, 0, ctx->stream, a);
        hipLaunchKernelGGL(smk::k_mcs_median, grid, block, 0, ctx->stream, a);
        hipLaunchKernelGGL(smk::k_mcs_bilateral, dim3((W + 31) / 32, (H + 7) / 8), block, wbytes, ctx->stream, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mcsgm_aggregate(sm_ctx* ctx, const float* vol, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D,
                       int min_disparity, const sm_mcsgm_params* params, float* agg)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!vol || !a || !b || !agg) return fail(ctx, SM_E_ARG, "mcsgm: a required pointer is NULL");
    int rc;
    if ((rc = mcsgm_check_shape(ctx, n, H, W, D)) != SM_OK) return rc;
    if ((rc = mcsgm_check_sgm(ctx, params, W)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& mc = ctx->mcsgm;
    const size_t ibytes = (size_t)n * H * W, vbytes = ibytes * D * sizeof(float);
    if ((rc = stage_in(ctx, {{mc.in_vol, vol, vbytes}, {mc.in_a, a, ibytes}, {mc.in_b, b, ibytes}, {mc.out, nullptr, vbytes}})) != SM_OK)
        return rc;
    if ((rc = sm_mcsgm_aggregate_device(ctx, (const float*)mc.in_vol.p, (const uint8_t*)mc.in_a.p, (const uint8_t*)mc.in_b.p, n,
                                        (size_t)H * W, H, W, W, D, min_disparity, params, (float*)mc.out.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{mc.out, agg, vbytes}});
}

int sm_mcsgm_disparity(sm_ctx* ctx, const float* agg_l, const float* agg_r, const uint8_t* a, int n, int H, int W, int D,
                       int min_disparity, const sm_mcsgm_params* params, float* disp, const sm_mcsgm_stages* stages)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!agg_l || !agg_r || !a || !disp) return fail(ctx, SM_E_ARG, "mcsgm: a required pointer is NULL");
    int rc;
    if ((rc = mcsgm_check_shape(ctx, n, H, W, D)) != SM_OK) return rc;
    if ((rc = mcsgm_check_disparity(ctx, params, D, min_disparity)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& mc = ctx->mcsgm;
    const size_t ibytes = (size_t)n * H * W, mbytes = ibytes * 4, vbytes = mbytes * D;
    if ((rc = stage_in(ctx, {{mc.in_vol, agg_l, vbytes}, {mc.in_vol_r, agg_r, vbytes}, {mc.in_a, a, ibytes}, {mc.out, nullptr, mbytes}})) != SM_OK)
        return rc;
    // the stage maps land in the context's own buffers (no device pointers given)
    if ((rc = sm_mcsgm_disparity_device(ctx, (const float*)mc.in_vol.p, (const float*)mc.in_vol_r.p, (const uint8_t*)mc.in_a.p, n,
                                        (size_t)H * W, H, W, W, D, min_disparity, params, (float*)mc.out.p, nullptr)) != SM_OK)
        return rc;
    const sm_mcsgm_stages none{};
    const sm_mcsgm_stages& st = stages ? *stages : none;
    return stage_out(ctx, {{mc.out, disp, mbytes}, {mc.wta_l, st.wta_left, mbytes}, {mc.wta_r, st.wta_right, mbytes},
                           {mc.status, st.status, mbytes}, {mc.filled, st.filled, mbytes}, {mc.sub, st.subpixel, mbytes},
                           {mc.med, st.median, mbytes}});
}

int sm_mcsgm_aggregate_host(const float* vol, const uint8_t* a, const uint8_t* b, int n, size_t image_stride, int H,
                            int W, size_t row_stride, int D, int min_disparity, const sm_mcsgm_params* params, float* agg)
{
    if (!vol || !a || !b || !agg) return fail(nullptr, SM_E_ARG, "mcsgm: a required pointer is NULL");
    int rc;
    if ((rc = mcsgm_check_shape(nullptr, n, H, W, D)) != SM_OK) return rc;
    if ((rc = mcsgm_check_strides(nullptr, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mcsgm_check_sgm(nullptr, params, W)) != SM_OK) return rc;
    const size_t cells = (size_t)n * D * H * W;
    if (agg < vol + cells && vol < agg + cells) return fail(nullptr, SM_E_ARG, "mcsgm: the aggregated volume overlaps the input volume");
    smk::mcsgm_aggregate_host(vol, a, b, n, image_stride, H, W, row_stride, D, min_disparity, penalties(params), params->sgm_i, agg);
    return SM_OK;
}

int sm_mcsgm_disparity_host(const float* agg_l, const float* agg_r, const uint8_t* a, int n, size_t image_stride, int H,
                            int W, size_t row_stride, int D, int min_disparity, const sm_mcsgm_params* params, float* disp,
                            const sm_mcsgm_stages* stages)
{
    if (!agg_l || !agg_r || !a || !disp) return fail(nullptr, SM_E_ARG, "mcsgm: a required pointer is NULL");
    int rc;
    if ((rc = mcsgm_check_shape(nullptr, n, H, W, D)) != SM_OK) return rc;
    if ((rc = mcsgm_check_strides(nullptr, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mcsgm_check_disparity(nullptr, params, D, min_disparity)) != SM_OK) return rc;
    const sm_mcsgm_stages none{};
    const sm_mcsgm_stages& st = stages ? *stages : none;
    smk::mcsgm_disparity_host(agg_l, agg_r, a, n, image_stride, H, W, row_stride, D, min_disparity, params->blur_sigma,
                              params->blur_t,
                              smk::McsMaps{st.wta_left, st.wta_right, st.status, st.filled, st.subpixel, st.median, disp});
    return SM_OK;
}

}  // extern "C"
