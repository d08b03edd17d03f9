// sm_api_mccbca.hip — C-ABI of the cross-based cost aggregation (sm_mccbca.hpp).  The only unit with these kernels.
#include <cmath>
#include <vector>

#define SM_MCCNN_NO_KERNELS 1  // sm_mccnn.hpp and sm_mcsgm.hpp: their host functions only
#define SM_MCSGM_NO_KERNELS 1
#include "sm_ctx.hpp"
#include "sm_mccbca.hpp"

// ---- cross-based cost aggregation (sm_mccbca.hpp)
namespace {

int mccbca_check_image(sm_ctx* ctx, int n, size_t image_stride, int H, int W, size_t row_stride)
{
    if (n < 1 || n > 65535) return fail(ctx, SM_E_ARG, "mccbca: %d images (1 .. 65535)", n);
    if (H < 1 || W < 1) return fail(ctx, SM_E_ARG, "mccbca: empty image (%dx%d)", W, H);
    if ((size_t)H * (size_t)W > smk::MC_MAXPIX)
        return fail(ctx, SM_E_UNSUPPORTED, "mccbca: image %dx%d has 2^24 pixels or more", W, H);
    if (row_stride < (size_t)W) return fail(ctx, SM_E_ARG, "mccbca: row_stride %zu smaller than a row (%d)", row_stride, W);
    if (n > 1 && image_stride < (size_t)(H - 1) * row_stride + (size_t)W)
        return fail(ctx, SM_E_ARG, "mccbca: image_stride %zu smaller than one image", image_stride);
    return SM_OK;
}

int mccbca_check_params(sm_ctx* ctx, const sm_mccbca_params* p)
{
    if (!p) return fail(ctx, SM_E_ARG, "mccbca: params is NULL");
    if (p->l1 < 1 || p->l1 > smk::MCB_MAXL) return fail(ctx, SM_E_ARG, "mccbca: l1 %d (1 .. %d)", p->l1, smk::MCB_MAXL);
    if (!std::isfinite(p->tau1) || !(p->tau1 > 0.0f)) return fail(ctx, SM_E_ARG, "mccbca: tau1 must be finite and positive");
    if (p->i1 < 0 || p->i1 > smk::MCB_MAXI || p->i2 < 0 || p->i2 > smk::MCB_MAXI)
        return fail(ctx, SM_E_ARG, "mccbca: i1 %d, i2 %d (0 .. %d)", p->i1, p->i2, smk::MCB_MAXI);
    return SM_OK;
}

int mccbca_check_volume(sm_ctx* ctx, int W, int D, int iterations)
{
    if (D < 1 || D > smk::MC_MAXD) return fail(ctx, SM_E_ARG, "mccbca: %d disparity planes (1 .. %d)", D, smk::MC_MAXD);
    if (W > smk::MCS_MAXW) return fail(ctx, SM_E_UNSUPPORTED, "mccbca: %d columns (at most %d)", W, smk::MCS_MAXW);
    if (iterations < 1 || iterations > smk::MCB_MAXI)
        return fail(ctx, SM_E_ARG, "mccbca: %d iterations (1 .. %d)", iterations, smk::MCB_MAXI);
    return SM_OK;
}

// the arms of n normalised images t ([n][H][W]): packed words into `packed` ([n][H][W]) or bytes into
// `planar` ([n][4][H][W])
void launch_arms(sm_ctx* ctx, const float* t, int n, int H, int W, const sm_mccbca_params* p, uint32_t* packed, uint8_t* planar)
{
    const size_t npix = (size_t)H * W;
    for (int img = 0; img < n; img++) {
        smk::McbArmsArgs a{t + (size_t)img * npix, H, W, p->l1, p->tau1, packed ? packed + (size_t)img * npix : nullptr,
                           planar ? planar + (size_t)img * 4 * npix : nullptr};
        hipLaunchKernelGGL(smk::k_mcb_arms, dim3((unsigned)((npix + smk::MCB_BLOCK - 1) / smk::MCB_BLOCK)), dim3(smk::MCB_BLOCK), 0,
                           ctx->stream, a);
    }
}

}  // namespace

extern "C" {

int sm_mccbca_default_params(sm_mccbca_params* out)
{
    if (!out) return fail(nullptr, SM_E_ARG, "mccbca: out is NULL");
    *out = sm_mccbca_params{5, 0.13f, 2, 0};
    return SM_OK;
}

int sm_mccbca_arms_device(sm_ctx* ctx, const uint8_t* d_gray, int n, size_t image_stride, int H, int W, size_t row_stride,
                          const sm_mccbca_params* params, uint8_t* d_arms)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_gray || !d_arms) return fail(ctx, SM_E_ARG, "mccbca: a required pointer is NULL");
    int rc;
    if ((rc = mccbca_check_image(ctx, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mccbca_check_params(ctx, params)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& cb = ctx->mccbca;
    const uint8_t* gray[1] = {d_gray};
    DevBuf* norm[1] = {&cb.ta};
    if ((rc = mcsgm_normalise(ctx, 1, gray, n, image_stride, H, W, row_stride, norm)) != SM_OK) return rc;
    launch_arms(ctx, (const float*)cb.ta.p, n, H, W, params, nullptr, d_arms);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mccbca_aggregate_device(sm_ctx* ctx, const float* d_vol, const uint8_t* d_a, const uint8_t* d_b, int n,
                               size_t image_stride, int H, int W, size_t row_stride, int D, int min_disparity,
                               const sm_mccbca_params* params, int iterations, float* d_agg)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_vol || !d_a || !d_b || !d_agg) return fail(ctx, SM_E_ARG, "mccbca: a required pointer is NULL");
    int rc;
    if ((rc = mccbca_check_image(ctx, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mccbca_check_params(ctx, params)) != SM_OK) return rc;
    if ((rc = mccbca_check_volume(ctx, W, D, iterations)) != SM_OK) return rc;
    const size_t npix = (size_t)H * W, cells = npix * D;
    if (d_agg < d_vol + (size_t)n * cells && d_vol < d_agg + (size_t)n * cells)
        return fail(ctx, SM_E_ARG, "mccbca: the aggregated volume overlaps the input volume");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& cb = ctx->mccbca;
    if ((rc = ensure(ctx, cb.arms_a, (size_t)n * npix * 4)) != SM_OK) return rc;
    if ((rc = ensure(ctx, cb.arms_b, (size_t)n * npix * 4)) != SM_OK) return rc;
    if (iterations > 1 && (rc = ensure(ctx, cb.iter, cells * sizeof(float))) != SM_OK) return rc;
    const uint8_t* gray[2] = {d_a, d_b};
    DevBuf* norm[2] = {&cb.ta, &cb.tb};
    if ((rc = mcsgm_normalise(ctx, 2, gray, n, image_stride, H, W, row_stride, norm)) != SM_OK) return rc;
    launch_arms(ctx, (const float*)cb.ta.p, n, H, W, params, (uint32_t*)cb.arms_a.p, nullptr);
    launch_arms(ctx, (const float*)cb.tb.p, n, H, W, params, (uint32_t*)cb.arms_b.p, nullptr);

    const int h = params->l1 - 1, ty = smk::mcb_tile_rows(h);
    const size_t lds = smk::mcb_lds_bytes(ty, h);
    const dim3 grid((unsigned)((H + ty - 1) / ty), (unsigned)((W + smk::MCB_TX - 1) / smk::MCB_TX), (unsigned)D);
    const int m = smk::mc_clamp_min_disparity(min_disparity, W, D);
    for (int img = 0; img < n; img++) {
        const float* src = d_vol + (size_t)img * cells;
        float* out = d_agg + (size_t)img * cells;
        for (int it = 0; it < iterations; it++) {
            float* dst = (iterations - 1 - it) % 2 == 0 ? out : (float*)cb.iter.p;
            smk::McbAggArgs a{src, dst, (const uint32_t*)cb.arms_a.p + (size_t)img * npix,
                              (const uint32_t*)cb.arms_b.p + (size_t)img * npix, H, W, D, m, h, ty};
            hipLaunchKernelGGL(smk::k_mcb_agg, grid, dim3(smk::MCB_BLOCK), lds, ctx->stream, a);
            src = dst;
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_mccbca_arms(sm_ctx* ctx, const uint8_t* gray, int n, int H, int W, const sm_mccbca_params* params, uint8_t* arms)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!gray || !arms) return fail(ctx, SM_E_ARG, "mccbca: a required pointer is NULL");
    int rc;
    if ((rc = mccbca_check_image(ctx, n, (size_t)H * W, H, W, W)) != SM_OK) return rc;
    if ((rc = mccbca_check_params(ctx, params)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& cb = ctx->mccbca;
    const size_t ibytes = (size_t)n * H * W;
    if ((rc = stage_in(ctx, {{cb.in_a, gray, ibytes}, {cb.out, nullptr, 4 * ibytes}})) != SM_OK) return rc;
    if ((rc = sm_mccbca_arms_device(ctx, (const uint8_t*)cb.in_a.p, n, (size_t)H * W, H, W, W, params, (uint8_t*)cb.out.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{cb.out, arms, 4 * ibytes}});
}

int sm_mccbca_aggregate(sm_ctx* ctx, const float* vol, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D,
                        int min_disparity, const sm_mccbca_params* params, int iterations, float* agg)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!vol || !a || !b || !agg) return fail(ctx, SM_E_ARG, "mccbca: a required pointer is NULL");
    int rc;
    if ((rc = mccbca_check_image(ctx, n, (size_t)H * W, H, W, W)) != SM_OK) return rc;
    if ((rc = mccbca_check_params(ctx, params)) != SM_OK) return rc;
    if ((rc = mccbca_check_volume(ctx, W, D, iterations)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& cb = ctx->mccbca;
    const size_t ibytes = (size_t)n * H * W, vbytes = ibytes * D * sizeof(float);
    if ((rc = stage_in(ctx, {{cb.in_vol, vol, vbytes}, {cb.in_a, a, ibytes}, {cb.in_b, b, ibytes}, {cb.out, nullptr, vbytes}})) != SM_OK)
        return rc;
    if ((rc = sm_mccbca_aggregate_device(ctx, (const float*)cb.in_vol.p, (const uint8_t*)cb.in_a.p, (const uint8_t*)cb.in_b.p, n,
                                         (size_t)H * W, H, W, W, D, min_disparity, params, iterations, (float*)cb.out.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{cb.out, agg, vbytes}});
}

int sm_mccbca_arms_host(const uint8_t* gray, int n, size_t image_stride, int H, int W, size_t row_stride,
                        const sm_mccbca_params* params, uint8_t* arms)
{
    if (!gray || !arms) return fail(nullptr, SM_E_ARG, "mccbca: a required pointer is NULL");
    int rc;
    if ((rc = mccbca_check_image(nullptr, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mccbca_check_params(nullptr, params)) != SM_OK) return rc;
    smk::mccbca_arms_host(gray, n, image_stride, H, W, row_stride, params->l1, params->tau1, arms);
    return SM_OK;
}

int sm_mccbca_aggregate_host(const float* vol, const uint8_t* a, const uint8_t* b, int n, size_t image_stride, int H,
                             int W, size_t row_stride, int D, int min_disparity, const sm_mccbca_params* params,
                             int iterations, float* agg)
{
    if (!vol || !a || !b || !agg) return fail(nullptr, SM_E_ARG, "mccbca: a required pointer is NULL");
    int rc;
    if ((rc = mccbca_check_image(nullptr, n, image_stride, H, W, row_stride)) != SM_OK) return rc;
    if ((rc = mccbca_check_params(nullptr, params)) != SM_OK) return rc;
    if ((rc = mccbca_check_volume(nullptr, W, D, iterations)) != SM_OK) return rc;
    const size_t cells = (size_t)n * D * H * W;
    if (agg < vol + cells && vol < agg + cells) return fail(nullptr, SM_E_ARG, "mccbca: the aggregated volume overlaps the input volume");
    smk::mccbca_aggregate_host(vol, a, b, n, image_stride, H, W, row_stride, D, min_disparity, params->l1, params->tau1, iterations,
                               agg);
    return SM_OK;
}

}  // extern "C"
