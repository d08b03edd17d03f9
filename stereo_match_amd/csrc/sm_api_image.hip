// sm_api_image.hip — C-ABI of the image front end: rectification maps, remap and BGR->gray
// (sm_rectify.hpp), fastNlMeansDenoising (sm_nlm.hpp), the float64 Gaussian filters, image_measure
// and pyrDown (sm_filter.hpp, which includes sm_rectify.hpp).  The only unit with these kernels.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sm_ctx.hpp"
#include "sm_rectify.hpp"
#include "sm_nlm.hpp"
#include "sm_filter.hpp"

extern "C" {

// ---- rectification front end (sm_rectify.hpp)
namespace {
bool aligned_to(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
}  // namespace

int sm_rectify_map_device(sm_ctx* ctx, const sm_rectify_cam* cam, int H, int W, float* d_mapx, float* d_mapy)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!cam || !d_mapx || !d_mapy) return fail(ctx, SM_E_ARG, "rectify map: NULL argument");
    if (H <= 0 || W <= 0 || H > kRectMaxDim || W > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "rectify map: size %d x %d outside 1..%d", W, H, kRectMaxDim);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    smk::RectMapArgs a{};
    std::memcpy(a.iR, cam->iR, sizeof a.iR);
    a.k1 = cam->dist[0], a.k2 = cam->dist[1], a.p1 = cam->dist[2], a.p2 = cam->dist[3], a.k3 = cam->dist[4];
    a.fx = cam->K[0], a.fy = cam->K[4], a.cx = cam->K[2], a.cy = cam->K[5];
    a.mapx = d_mapx, a.mapy = d_mapy, a.H = H, a.W = W;
    hipLaunchKernelGGL(smk::k_rectify_map, dim3((W + 255) / 256, H), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_rectify_map(sm_ctx* ctx, const sm_rectify_cam* cam, int H, int W, float* mapx, float* mapy)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!cam || !mapx || !mapy) return fail(ctx, SM_E_ARG, "rectify map: NULL argument");
    if (H <= 0 || W <= 0 || H > kRectMaxDim || W > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "rectify map: size %d x %d outside 1..%d", W, H, kRectMaxDim);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t mb = (size_t)H * W * 4;
    int rc;
    if ((rc = ensure(ctx, ctx->rm.mapx, mb)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->rm.mapy, mb)) != SM_OK) return rc;
    if ((rc = sm_rectify_map_device(ctx, cam, H, W, (float*)ctx->rm.mapx.p, (float*)ctx->rm.mapy.p)) != SM_OK) return rc;
    return stage_out(ctx, {{ctx->rm.mapx, mapx, mb}, {ctx->rm.mapy, mapy, mb}});
}

namespace {
int remap_check(sm_ctx* ctx, const void* src, int srcH, int srcW, int src_stride, int channels, const void* mapx,
                const void* mapy, int H, int W, const void* dst, const void* gray)
{
    if (!src || !mapx || !mapy) return fail(ctx, SM_E_ARG, "remap: NULL source or map");
    if (!dst && !gray) return fail(ctx, SM_E_ARG, "remap: both outputs are NULL");
    if (channels != 1 && channels != 3) return fail(ctx, SM_E_ARG, "remap: channels %d (1 or 3)", channels);
    if (gray && channels != 3) return fail(ctx, SM_E_ARG, "remap: the gray output needs a 3-channel (BGR) source");
    if (srcH <= 0 || srcW <= 0 || srcH > kRectMaxDim || srcW > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "remap: source size %d x %d outside 1..%d", srcW, srcH, kRectMaxDim);
    if (H <= 0 || W <= 0 || H > kRectMaxDim || W > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "remap: destination size %d x %d outside 1..%d", W, H, kRectMaxDim);
    if (src_stride < srcW * channels) return fail(ctx, SM_E_ARG, "remap: src_stride %d < %d", src_stride, srcW * channels);
    return SM_OK;
}
}  // namespace

int sm_remap_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t img_stride_bytes, int srcH, int srcW,
                             int src_stride, int channels, const float* d_mapx, const float* d_mapy, int H, int W,
                             uint8_t* d_dst, uint8_t* d_gray)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = remap_check(ctx, d_src, srcH, srcW, src_stride, channels, d_mapx, d_mapy, H, W, d_dst, d_gray)) != SM_OK)
        return rc;
    if (nimg < 0 || nimg > 65535 * smk::REMAP_IPT) return fail(ctx, SM_E_ARG, "remap: nimg %d", nimg);
    if (nimg > 1 && img_stride_bytes < (size_t)(srcH - 1) * src_stride + (size_t)srcW * channels)
        return fail(ctx, SM_E_ARG, "remap: img_stride_bytes %zu smaller than one image", img_stride_bytes);
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    smk::RemapArgs a{};
    a.src = d_src, a.mapx = d_mapx, a.mapy = d_mapy, a.dst = d_dst, a.gray = d_gray;
    a.img_stride = img_stride_bytes;
    a.nimg = nimg, a.srcH = srcH, a.srcW = srcW, a.src_stride = src_stride, a.H = H, a.W = W;
    a.Wq = (W + 3) / 4;
    a.vec = W % 4 == 0 && aligned_to(d_mapx, 16) && aligned_to(d_mapy, 16) && aligned_to(d_dst, 4) &&
            aligned_to(d_gray, 4);
    const dim3 grid(((unsigned)H * a.Wq + 255) / 256, (nimg + smk::REMAP_IPT - 1) / smk::REMAP_IPT);
    if (channels == 1)
        hipLaunchKernelGGL((smk::k_remap_u8<1, false>), grid, dim3(256), 0, ctx->stream, a);
    else if (d_gray)
        hipLaunchKernelGGL((smk::k_remap_u8<3, true>), grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((smk::k_remap_u8<3, false>), grid, dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_remap_u8(sm_ctx* ctx, const uint8_t* src, int srcH, int srcW, int src_stride, int channels, const float* mapx,
                const float* mapy, int H, int W, uint8_t* dst, uint8_t* gray)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = remap_check(ctx, src, srcH, srcW, src_stride, channels, mapx, mapy, H, W, dst, gray)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = (size_t)(srcH - 1) * src_stride + (size_t)srcW * channels, npx = (size_t)H * W;
    if (dst && (rc = ensure(ctx, ctx->rm.dst, npx * channels)) != SM_OK) return rc;
    if (gray && (rc = ensure(ctx, ctx->rm.gray, npx)) != SM_OK) return rc;
    if ((rc = stage_in(ctx, {{ctx->rm.src, src, sb}, {ctx->rm.mapx, mapx, npx * 4}, {ctx->rm.mapy, mapy, npx * 4}})) != SM_OK)
        return rc;
    if ((rc = sm_remap_u8_batch_device(ctx, (const uint8_t*)ctx->rm.src.p, 1, 0, srcH, srcW, src_stride, channels,
                                       (const float*)ctx->rm.mapx.p, (const float*)ctx->rm.mapy.p, H, W,
                                       dst ? (uint8_t*)ctx->rm.dst.p : nullptr,
                                       gray ? (uint8_t*)ctx->rm.gray.p : nullptr)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->rm.dst, dst, npx * channels}, {ctx->rm.gray, gray, npx}});  // a NULL output is skipped
}

int sm_bgr2gray_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t img_stride_bytes, int H, int W,
                                int src_stride, uint8_t* d_gray)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_src || !d_gray) return fail(ctx, SM_E_ARG, "bgr2gray: NULL argument");
    if (H <= 0 || W <= 0 || H > kRectMaxDim || W > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "bgr2gray: size %d x %d outside 1..%d", W, H, kRectMaxDim);
    if (src_stride < W * 3) return fail(ctx, SM_E_ARG, "bgr2gray: src_stride %d < %d", src_stride, W * 3);
    if (nimg < 0 || nimg > 65535) return fail(ctx, SM_E_ARG, "bgr2gray: nimg %d", nimg);
    if (nimg > 1 && img_stride_bytes < (size_t)(H - 1) * src_stride + (size_t)W * 3)
        return fail(ctx, SM_E_ARG, "bgr2gray: img_stride_bytes %zu smaller than one image", img_stride_bytes);
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    smk::GrayArgs a{};
    a.src = d_src, a.gray = d_gray, a.img_stride = img_stride_bytes, a.H = H, a.W = W, a.src_stride = src_stride;
    hipLaunchKernelGGL(smk::k_bgr2gray, dim3((W + 255) / 256, H, nimg), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_bgr2gray_u8(sm_ctx* ctx, const uint8_t* src, int H, int W, int src_stride, uint8_t* gray)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!src || !gray) return fail(ctx, SM_E_ARG, "bgr2gray: NULL argument");
    if (H <= 0 || W <= 0 || H > kRectMaxDim || W > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "bgr2gray: size %d x %d outside 1..%d", W, H, kRectMaxDim);
    if (src_stride < W * 3) return fail(ctx, SM_E_ARG, "bgr2gray: src_stride %d < %d", src_stride, W * 3);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = (size_t)(H - 1) * src_stride + (size_t)W * 3, npx = (size_t)H * W;
    int rc;
    if ((rc = stage_in(ctx, {{ctx->rm.src, src, sb}, {ctx->rm.gray, nullptr, npx}})) != SM_OK) return rc;
    if ((rc = sm_bgr2gray_u8_batch_device(ctx, (const uint8_t*)ctx->rm.src.p, 1, 0, H, W, src_stride,
                                          (uint8_t*)ctx->rm.gray.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->rm.gray, gray, npx}});
}

// ---- fastNlMeansDenoising (sm_nlm.hpp)
namespace {
struct NlmGeo {
    int th, sh, t, s, fpm, shift, n;
    double mult;
};

// window sizes and h checked, and the table's constants (the only floating-point part)
int nlm_geo(sm_ctx* ctx, float h, int template_window, int search_window, NlmGeo& g)
{
    if (template_window < 1) return fail(ctx, SM_E_ARG, "nlm: templateWindowSize %d < 1", template_window);
    if (search_window < 1) return fail(ctx, SM_E_ARG, "nlm: searchWindowSize %d < 1", search_window);
    if (!(h >= 0.f) || std::isinf(h)) return fail(ctx, SM_E_ARG, "nlm: h = %g (a finite h >= 0 is needed)", (double)h);
    g.th = template_window / 2, g.sh = search_window / 2;
    g.t = 2 * g.th + 1, g.s = 2 * g.sh + 1;
    if (g.th > smk::NLM_MAX_TH)
        return fail(ctx, SM_E_UNSUPPORTED, "nlm: templateWindowSize %d (template %d x %d) not built: 1..%d",
                    template_window, g.t, g.t, 2 * smk::NLM_MAX_TH + 1);
    if (g.sh > smk::NLM_MAX_SH)
        return fail(ctx, SM_E_UNSUPPORTED, "nlm: searchWindowSize %d (search %d x %d) not built: 1..%d", search_window,
                    g.s, g.s, 2 * smk::NLM_MAX_SH + 1);
    g.fpm = INT32_MAX / (g.s * g.s * 255);
    g.shift = 0;
    while ((1 << g.shift) < g.t * g.t) g.shift++;
    g.mult = double(1 << g.shift) / double(g.t * g.t);
    g.n = int(65025.0 / g.mult + 1);
    return SM_OK;
}

// tab[a] = rint(fpm * exp(-(a * mult) / (h * h))) (h * h in float32; a NaN weight, h = 0 at
// a = 0, counts as 1), entries below fpm / 1000 zeroed; returns the non-zero prefix's length
int nlm_table(const NlmGeo& g, float h, int32_t* tab)
{
    const float hhf = h * h;
    const double hh = (double)hhf, floor_w = 0.001 * g.fpm;
    int last = 0;
    for (int a = 0; a < g.n; a++) {
        double w = std::exp(-(a * g.mult) / hh);
        if (w != w) w = 1.0;
        int v = (int)std::nearbyint(g.fpm * w);  // the default rounding mode: half to even
        if (v < floor_w) v = 0;
        tab[a] = v;
        if (v) last = a + 1;
    }
    return last;
}

// the device copy of the table's non-zero prefix for (h, t, s), cached in the context
int ensure_nlm_table(sm_ctx* ctx, const NlmGeo& g, float h)
{
    uint32_t hb;
    std::memcpy(&hb, &h, 4);
    if (ctx->nlm.ntab > 0 && ctx->nlm.key_h == hb && ctx->nlm.key_t == g.t && ctx->nlm.key_s == g.s) return SM_OK;
    // launches that read the old table (on whichever stream they were queued) finish first
    HIP_TRY(ctx, hipDeviceSynchronize());
    ctx->nlm.ntab = 0;
    ctx->nlm.tab_host.resize(g.n);
    const int ntab = nlm_table(g, h, ctx->nlm.tab_host.data());
    int rc;
    if ((rc = ensure(ctx, ctx->nlm.tab, (size_t)ntab * 4)) != SM_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->nlm.tab.p, ctx->nlm.tab_host.data(), (size_t)ntab * 4, hipMemcpyHostToDevice,
                                ctx->stream));
    // once per (h, t, s): the table is complete before a launch on any other stream uses it,
    // and nlm.tab_host (kept anyway) is not touched while the copy runs
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->nlm.key_h = hb, ctx->nlm.key_t = g.t, ctx->nlm.key_s = g.s, ctx->nlm.shift = g.shift;
    ctx->nlm.ntab = ntab;
    return SM_OK;
}

int nlm_image_check(sm_ctx* ctx, const void* src, const void* dst, int H, int W, int src_stride)
{
    if (H <= 0 || W <= 0 || H > kRectMaxDim || W > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "nlm: size %d x %d outside 1..%d", W, H, kRectMaxDim);
    if (!src || !dst) return fail(ctx, SM_E_ARG, "nlm: NULL argument");
    if (src_stride < W) return fail(ctx, SM_E_ARG, "nlm: src_stride %d < %d", src_stride, W);
    return SM_OK;
}
}  // namespace

int sm_nlm_weight_table(float h, int template_window, int search_window, int32_t* tab, int* n, int* fpm, int* shift)
{
    NlmGeo g;
    int rc;
    if ((rc = nlm_geo(nullptr, h, template_window, search_window, g)) != SM_OK) return rc;
    if (n) *n = g.n;
    if (fpm) *fpm = g.fpm;
    if (shift) *shift = g.shift;
    if (tab) nlm_table(g, h, tab);
    return SM_OK;
}

int sm_nlm_denoise_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t img_stride_bytes, int H, int W,
                                   int src_stride, float h, int template_window, int search_window, uint8_t* d_dst)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    NlmGeo g;
    if ((rc = nlm_image_check(ctx, d_src, d_dst, H, W, src_stride)) != SM_OK) return rc;
    if ((rc = nlm_geo(ctx, h, template_window, search_window, g)) != SM_OK) return rc;
    if (nimg < 0 || nimg > 65535) return fail(ctx, SM_E_ARG, "nlm: nimg %d", nimg);
    if (nimg > 1 && img_stride_bytes < (size_t)(H - 1) * src_stride + (size_t)W)
        return fail(ctx, SM_E_ARG, "nlm: img_stride_bytes %zu smaller than one image", img_stride_bytes);
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_nlm_table(ctx, g, h)) != SM_OK) return rc;
    smk::NlmArgs a{};
    a.src = d_src, a.dst = d_dst, a.tab = (const int32_t*)ctx->nlm.tab.p;
    a.img_stride = img_stride_bytes;
    a.H = H, a.W = W, a.src_stride = src_stride;
    a.sh = g.sh, a.shift = ctx->nlm.shift, a.ntab = ctx->nlm.ntab;
    a.pitch = smk::nlm_pitch(g.th, g.sh);
    const bool lds_tab = a.ntab <= smk::NLM_LDS_TAB_MAX;
    const size_t lds = smk::nlm_lds_bytes(g.th, g.sh, lds_tab ? a.ntab : 0);
    const dim3 grid((W + smk::NLM_TILE - 1) / smk::NLM_TILE, (H + smk::NLM_TILE - 1) / smk::NLM_TILE, nimg);
    if (lds_tab)
        smk::nlm_launch<true>(g.th, grid, lds, ctx->stream, a);
    else
        smk::nlm_launch<false>(g.th, grid, lds, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_nlm_denoise_u8(sm_ctx* ctx, const uint8_t* src, int H, int W, int src_stride, float h, int template_window,
                      int search_window, uint8_t* dst)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    NlmGeo g;
    if ((rc = nlm_image_check(ctx, src, dst, H, W, src_stride)) != SM_OK) return rc;
    if ((rc = nlm_geo(ctx, h, template_window, search_window, g)) != SM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = (size_t)(H - 1) * src_stride + (size_t)W, npx = (size_t)H * W;
    if ((rc = stage_in(ctx, {{ctx->rm.src, src, sb}, {ctx->rm.gray, nullptr, npx}})) != SM_OK) return rc;
    if ((rc = sm_nlm_denoise_u8_batch_device(ctx, (const uint8_t*)ctx->rm.src.p, 1, 0, H, W, src_stride, h,
                                             template_window, search_window, (uint8_t*)ctx->rm.gray.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->rm.gray, dst, npx}});
}

// ---- gaussian_filter, image_measure and pyrDown (sm_filter.hpp)
namespace {

// the half kernel of one axis into the kernel arguments; NULL or r = 0: the identity
int gauss_axis(sm_ctx* ctx, const char* who, const char* axis, const double* w, int r, double* out, int& r_out)
{
    if (r < 0) return fail(ctx, SM_E_ARG, "%s: radius %d of axis %s < 0", who, r, axis);
    if (r > smk::GF_MAX_R)
        return fail(ctx, SM_E_UNSUPPORTED, "%s: radius %d of axis %s not built: 0..%d", who, r, axis, smk::GF_MAX_R);
    if (!w || r == 0) {
        out[0] = 1.0;
        r_out = 0;
        return SM_OK;
    }
    std::copy(w, w + r + 1, out);
    r_out = r;
    return SM_OK;
}

int filter_image_check(sm_ctx* ctx, const char* who, const void* src, const void* dst, int nimg, int H, int W)
{
    if (H <= 0 || W <= 0 || H > kRectMaxDim || W > kRectMaxDim)
        return fail(ctx, SM_E_ARG, "%s: size %d x %d outside 1..%d", who, W, H, kRectMaxDim);
    if (!src || !dst) return fail(ctx, SM_E_ARG, "%s: NULL argument", who);
    if (nimg < 0 || nimg > 65535) return fail(ctx, SM_E_ARG, "%s: nimg %d", who, nimg);
    return SM_OK;
}

// elements from the first image's first to the last image's last
size_t filter_span(int nimg, size_t img_stride, int H, int W, int stride)
{
    return (size_t)(nimg - 1) * img_stride + (size_t)(H - 1) * stride + (size_t)W;
}

extern "C++" template <bool BGR, bool UNSHARP>
int gauss_launch(sm_ctx* ctx, const smk::GaussArgs& a, int nimg)
{
    const size_t lds = smk::gauss_lds_bytes(a.ry, a.rx);
    const auto kernel = smk::k_gauss2d_f64<BGR, UNSHARP>;
    if (lds > 48 * 1024)  // above the default limit of dynamic LDS
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((a.W + smk::GF_TW - 1) / smk::GF_TW, (a.H + smk::GF_TH - 1) / smk::GF_TH, nimg);
    hipLaunchKernelGGL(kernel, grid, dim3(smk::GF_THREADS), lds, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

}  // namespace

int sm_gauss2d_f64_batch_device(sm_ctx* ctx, const double* d_src, int nimg, size_t src_img_stride, int H, int W,
                                int src_stride, const double* wy, int ry, const double* wx, int rx, double* d_dst,
                                size_t dst_img_stride, int dst_stride)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = filter_image_check(ctx, "gauss2d", d_src, d_dst, nimg, H, W)) != SM_OK) return rc;
    if (src_stride < W || dst_stride < W)
        return fail(ctx, SM_E_ARG, "gauss2d: row stride %d / %d < %d", src_stride, dst_stride, W);
    if (nimg > 1 && (src_img_stride < filter_span(1, 0, H, W, src_stride) ||
                     dst_img_stride < filter_span(1, 0, H, W, dst_stride)))
        return fail(ctx, SM_E_ARG, "gauss2d: image stride %zu / %zu smaller than one image", src_img_stride,
                    dst_img_stride);
    smk::GaussArgs a{};
    if ((rc = gauss_axis(ctx, "gauss2d", "0", wy, ry, a.wy, a.ry)) != SM_OK) return rc;
    if ((rc = gauss_axis(ctx, "gauss2d", "1", wx, rx, a.wx, a.rx)) != SM_OK) return rc;
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    a.src = d_src, a.dst = d_dst, a.src_img_stride = src_img_stride, a.dst_img_stride = dst_img_stride;
    a.H = H, a.W = W, a.src_stride = src_stride, a.dst_stride = dst_stride;
    return gauss_launch<false, false>(ctx, a, nimg);
}

int sm_gauss2d_f64(sm_ctx* ctx, const double* src, int nimg, size_t src_img_stride, int H, int W, int src_stride,
                   const double* wy, int ry, const double* wx, int rx, double* dst)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = filter_image_check(ctx, "gauss2d", src, dst, nimg, H, W)) != SM_OK) return rc;
    if (src_stride < W) return fail(ctx, SM_E_ARG, "gauss2d: row stride %d < %d", src_stride, W);
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = filter_span(nimg, src_img_stride, H, W, src_stride) * 8, db = (size_t)nimg * H * W * 8;
    if ((rc = stage_in(ctx, {{ctx->rm.src, src, sb}, {ctx->rm.dst, nullptr, db}})) != SM_OK) return rc;
    if ((rc = sm_gauss2d_f64_batch_device(ctx, (const double*)ctx->rm.src.p, nimg, src_img_stride, H, W, src_stride,
                                          wy, ry, wx, rx, (double*)ctx->rm.dst.p, (size_t)H * W, W)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->rm.dst, dst, db}});
}

int sm_image_measure_u8_batch_device(sm_ctx* ctx, const uint8_t* d_bgr, int nimg, size_t img_stride_bytes, int H, int W,
                                     int src_stride, const double* w1, int r1, const double* w2, int r2, double alpha,
                                     double* d_dst)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = filter_image_check(ctx, "image_measure", d_bgr, d_dst, nimg, H, W)) != SM_OK) return rc;
    if (src_stride < W * 3) return fail(ctx, SM_E_ARG, "image_measure: src_stride %d < %d", src_stride, W * 3);
    if (nimg > 1 && img_stride_bytes < (size_t)(H - 1) * src_stride + (size_t)W * 3)
        return fail(ctx, SM_E_ARG, "image_measure: img_stride_bytes %zu smaller than one image", img_stride_bytes);
    smk::GaussArgs a{}, b{};
    if ((rc = gauss_axis(ctx, "image_measure", "0 and 1 of the first filter", w1, r1, a.wy, a.ry)) != SM_OK) return rc;
    if ((rc = gauss_axis(ctx, "image_measure", "0 and 1 of the second filter", w2, r2, b.wy, b.ry)) != SM_OK) return rc;
    std::copy(a.wy, a.wy + a.ry + 1, a.wx), a.rx = a.ry;
    std::copy(b.wy, b.wy + b.ry + 1, b.wx), b.rx = b.ry;
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)H * W;
    // a reallocation waits for the whole device (ensure), so no earlier launch still uses filter.a
    if ((rc = ensure(ctx, ctx->filter.a, (size_t)nimg * npx * 8)) != SM_OK) return rc;
    a.src = d_bgr, a.dst = (double*)ctx->filter.a.p, a.src_img_stride = img_stride_bytes, a.dst_img_stride = npx;
    a.H = H, a.W = W, a.src_stride = src_stride, a.dst_stride = W;
    if ((rc = gauss_launch<true, false>(ctx, a, nimg)) != SM_OK) return rc;
    b.src = ctx->filter.a.p, b.dst = d_dst, b.src_img_stride = npx, b.dst_img_stride = npx;
    b.H = H, b.W = W, b.src_stride = W, b.dst_stride = W, b.alpha = alpha;
    return gauss_launch<false, true>(ctx, b, nimg);
}

int sm_image_measure_u8(sm_ctx* ctx, const uint8_t* bgr, int H, int W, int src_stride, const double* w1, int r1,
                        const double* w2, int r2, double alpha, double* dst)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = filter_image_check(ctx, "image_measure", bgr, dst, 1, H, W)) != SM_OK) return rc;
    if (src_stride < W * 3) return fail(ctx, SM_E_ARG, "image_measure: src_stride %d < %d", src_stride, W * 3);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = (size_t)(H - 1) * src_stride + (size_t)W * 3, db = (size_t)H * W * 8;
    if ((rc = stage_in(ctx, {{ctx->rm.src, bgr, sb}, {ctx->rm.dst, nullptr, db}})) != SM_OK) return rc;
    if ((rc = sm_image_measure_u8_batch_device(ctx, (const uint8_t*)ctx->rm.src.p, 1, 0, H, W, src_stride, w1, r1, w2,
                                               r2, alpha, (double*)ctx->rm.dst.p)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->rm.dst, dst, db}});
}

int sm_pyr_down_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t src_img_stride_bytes, int H, int W,
                                int src_stride, int channels, uint8_t* d_dst, size_t dst_img_stride_bytes,
                                int dst_stride)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = filter_image_check(ctx, "pyrDown", d_src, d_dst, nimg, H, W)) != SM_OK) return rc;
    if (channels != 1 && channels != 3) return fail(ctx, SM_E_ARG, "pyrDown: channels %d (1 or 3)", channels);
    const int dH = (H + 1) / 2, dW = (W + 1) / 2;
    if (src_stride < W * channels || dst_stride < dW * channels)
        return fail(ctx, SM_E_ARG, "pyrDown: row stride %d / %d < %d / %d", src_stride, dst_stride, W * channels,
                    dW * channels);
    if (nimg > 1 && (src_img_stride_bytes < filter_span(1, 0, H, W * channels, src_stride) ||
                     dst_img_stride_bytes < filter_span(1, 0, dH, dW * channels, dst_stride)))
        return fail(ctx, SM_E_ARG, "pyrDown: image stride %zu / %zu smaller than one image", src_img_stride_bytes,
                    dst_img_stride_bytes);
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    smk::PyrArgs a{};
    a.src = d_src, a.dst = d_dst, a.src_img_stride = src_img_stride_bytes, a.dst_img_stride = dst_img_stride_bytes;
    a.H = H, a.W = W, a.dH = dH, a.dW = dW, a.src_stride = src_stride, a.dst_stride = dst_stride;
    a.vec = ((uintptr_t)d_dst | (uintptr_t)dst_stride | (nimg > 1 ? dst_img_stride_bytes : 0)) % 4 == 0;
    const dim3 grid(((dW * channels + 3) / 4 + 255) / 256, dH, nimg);
    if (channels == 1)
        hipLaunchKernelGGL(smk::k_pyr_down_u8<1>, grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(smk::k_pyr_down_u8<3>, grid, dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_pyr_down_u8(sm_ctx* ctx, const uint8_t* src, int H, int W, int src_stride, int channels, uint8_t* dst)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    int rc;
    if ((rc = filter_image_check(ctx, "pyrDown", src, dst, 1, H, W)) != SM_OK) return rc;
    if (channels != 1 && channels != 3) return fail(ctx, SM_E_ARG, "pyrDown: channels %d (1 or 3)", channels);
    if (src_stride < W * channels) return fail(ctx, SM_E_ARG, "pyrDown: src_stride %d < %d", src_stride, W * channels);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int dH = (H + 1) / 2, dW = (W + 1) / 2;
    const size_t sb = (size_t)(H - 1) * src_stride + (size_t)W * channels, db = (size_t)dH * dW * channels;
    if ((rc = stage_in(ctx, {{ctx->rm.src, src, sb}, {ctx->rm.dst, nullptr, db}})) != SM_OK) return rc;
    if ((rc = sm_pyr_down_u8_batch_device(ctx, (const uint8_t*)ctx->rm.src.p, 1, 0, H, W, src_stride, channels,
                                          (uint8_t*)ctx->rm.dst.p, 0, dW * channels)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->rm.dst, dst, db}});
}

}  // extern "C"
