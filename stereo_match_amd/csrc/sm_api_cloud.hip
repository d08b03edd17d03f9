// sm_api_cloud.hip — C-ABI of reprojectImageTo3D (sm_reproject.hpp) and of the point clouds:
// masked extraction and the ASCII PLY body (sm_cloud.hpp, which includes sm_reproject.hpp).
// The only unit with these kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "sm_ctx.hpp"
#include "sm_reproject.hpp"
#include "sm_cloud.hpp"

namespace {

// the maps' minima on the ctx stream (k_disp_min, k_keys_to_float): mn[img] is the minimum of
// the non-NaN pixels (handleMissingValues), lo[img] numpy's `d.min()` (lo = "min"; may be NULL).
// ctx->rp.min: int keys [2][nimg], then float [2][nimg].
int disp_minima_enqueue(sm_ctx* ctx, const void* d_disp, int disp_type, int nimg, size_t npx, const float** mn,
                        const float** lo)
{
    int rc;
    if ((rc = ensure(ctx, ctx->rp.min, (size_t)nimg * 16)) != SM_OK) return rc;
    int* keys = (int*)ctx->rp.min.p;
    float* out = (float*)(keys + 2 * (size_t)nimg);
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)keys, smk::KEY_NONE, 2 * (size_t)nimg, ctx->stream));
    const dim3 g((unsigned)std::min<size_t>((npx + 255) / 256, 1024), nimg);
    if (disp_type == SM_DISP_S16)
        hipLaunchKernelGGL(smk::k_disp_min<int16_t>, g, dim3(256), 0, ctx->stream, (const int16_t*)d_disp, keys, npx);
    else
        hipLaunchKernelGGL(smk::k_disp_min<float>, g, dim3(256), 0, ctx->stream, (const float*)d_disp, keys, npx);
    hipLaunchKernelGGL(smk::k_keys_to_float, dim3((nimg + 63) / 64), dim3(64), 0, ctx->stream, keys, out, nimg);
    *mn = out;
    if (lo) *lo = out + nimg;
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_reproject_image_to_3d_device(sm_ctx* ctx, const void* d_disp, int disp_type, int nimg, int H, int W,
                                    const double* Q, int handle_missing, float* d_xyz)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_disp || !d_xyz || !Q || nimg < 0 || H <= 0 || W <= 0) return fail(ctx, SM_E_ARG, "bad arguments");
    if (disp_type != SM_DISP_S16 && disp_type != SM_DISP_F32)
        return fail(ctx, SM_E_UNSUPPORTED, "disparity type %d not supported (int16 or float32)", disp_type);
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    smk::ReprojArgs ra{};
    ra.disp = d_disp;
    ra.xyz = d_xyz;
    std::memcpy(ra.Q, Q, sizeof ra.Q);
    ra.H = H;
    ra.W = W;
    ra.handle_missing = handle_missing != 0;
    const size_t npx = (size_t)H * W;
    if (ra.handle_missing) {
        int rc;
        if ((rc = disp_minima_enqueue(ctx, d_disp, disp_type, nimg, npx, &ra.min_disp, nullptr)) != SM_OK) return rc;
    }
    const dim3 grid((W + 255) / 256, H, nimg);
    if (disp_type == SM_DISP_S16)
        hipLaunchKernelGGL(smk::k_reproject<int16_t>, grid, dim3(256), 0, ctx->stream, ra);
    else
        hipLaunchKernelGGL(smk::k_reproject<float>, grid, dim3(256), 0, ctx->stream, ra);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_reproject_image_to_3d(sm_ctx* ctx, const void* disp, int disp_type, int H, int W, const double* Q,
                             int handle_missing, float* xyz)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!disp || !xyz || !Q || H <= 0 || W <= 0) return fail(ctx, SM_E_ARG, "bad arguments");
    if (disp_type != SM_DISP_S16 && disp_type != SM_DISP_F32)
        return fail(ctx, SM_E_UNSUPPORTED, "disparity type %d not supported (int16 or float32)", disp_type);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)H * W, ib = npx * (disp_type == SM_DISP_S16 ? 2 : 4);
    int rc;
    if ((rc = stage_in(ctx, {{ctx->rp.in, disp, ib}, {ctx->rp.out, nullptr, npx * 12}})) != SM_OK) return rc;
    if ((rc = sm_reproject_image_to_3d_device(ctx, ctx->rp.in.p, disp_type, 1, H, W, Q, handle_missing,
                                              (float*)ctx->rp.out.p)) != SM_OK)
        return rc;
    if ((rc = stage_out(ctx, {{ctx->rp.out, xyz, npx * 12}})) != SM_OK) return rc;
    return check_sweep_errors(ctx);
}

// ---- point clouds: masked extraction and the ASCII PLY body (sm_cloud.hpp)
namespace {

struct CloudGeo {
    size_t npx, nblk, rows_max;
    int bpi;
    double lo, hi;
};

int cloud_check(sm_ctx* ctx, const void* disp, int disp_type, const uint8_t* bgr, size_t img_stride, int bgr_stride,
                int nimg, int H, int W, const double* Q, const sm_cloud_params* p, CloudGeo& g)
{
    if (!disp || !bgr || !Q || !p) return fail(ctx, SM_E_ARG, "cloud: a required pointer is NULL");
    if (H <= 0 || W <= 0) return fail(ctx, SM_E_ARG, "cloud: empty map (%dx%d)", W, H);
    if (disp_type != SM_DISP_S16 && disp_type != SM_DISP_F32)
        return fail(ctx, SM_E_UNSUPPORTED, "cloud: disparity type %d not supported (int16 or float32)", disp_type);
    if (nimg < 0 || nimg > 65535) return fail(ctx, SM_E_ARG, "cloud: nimg %d", nimg);
    if ((size_t)H * (size_t)W > ((size_t)1 << 30))
        return fail(ctx, SM_E_UNSUPPORTED, "cloud: %dx%d is more than 2^30 pixels", W, H);
    if ((size_t)bgr_stride < 3 * (size_t)W || bgr_stride < 0)
        return fail(ctx, SM_E_ARG, "cloud: bgr_stride %d smaller than a row of %d BGR pixels", bgr_stride, W);
    if (nimg > 1 && img_stride < (size_t)(H - 1) * bgr_stride + 3 * (size_t)W)
        return fail(ctx, SM_E_ARG, "cloud: bgr_img_stride_bytes %zu smaller than one image", img_stride);
    if (p->lo_mode != SM_CLOUD_LO_NONE && p->lo_mode != SM_CLOUD_LO_VALUE && p->lo_mode != SM_CLOUD_LO_MIN)
        return fail(ctx, SM_E_ARG, "cloud: lo_mode %d unknown", p->lo_mode);
    if ((p->lo_mode == SM_CLOUD_LO_VALUE && std::isnan(p->lo)) || (p->has_hi && std::isnan(p->hi)))
        return fail(ctx, SM_E_ARG, "cloud: a bound is NaN");
    g.npx = (size_t)H * W;
    g.bpi = (int)((g.npx + smk::CLOUD_BLOCK - 1) / smk::CLOUD_BLOCK);
    g.nblk = (size_t)g.bpi * (size_t)nimg;
    g.rows_max = g.npx * (size_t)nimg;
    if (g.nblk > 0x7FFFFFFFull) return fail(ctx, SM_E_UNSUPPORTED, "cloud: %zu blocks of pixels in one call", g.nblk);
    // numpy >= 2 compares a float32 map with the Python scalar rounded to float32; an int16 map
    // compares as the numbers they are
    g.lo = disp_type == SM_DISP_F32 ? (double)(float)p->lo : p->lo;
    g.hi = disp_type == SM_DISP_F32 ? (double)(float)p->hi : p->hi;
    return SM_OK;
}

// the three launches of the extraction (+ the maps' minima when asked for) on the ctx stream.
// d_verts NULL: counts only.  The total is left in ctx->cloud.off[g.nblk].
int cloud_extract_enqueue(sm_ctx* ctx, const void* d_disp, int disp_type, const uint8_t* d_bgr, size_t img_stride,
                          int bgr_stride, int nimg, int H, int W, const double* Q, const sm_cloud_params* p,
                          const CloudGeo& g, size_t cap_rows, float* d_verts, uint8_t* d_colors, int64_t* d_counts)
{
    int rc;
    if ((rc = ensure(ctx, ctx->cloud.tot, g.nblk * 4)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->cloud.off, (g.nblk + 1) * 8)) != SM_OK) return rc;
    smk::CloudArgs a{};
    a.disp = d_disp, a.bgr = d_bgr, a.bgr_img_stride = img_stride;
    std::memcpy(a.Q, Q, sizeof a.Q);
    a.lo = g.lo, a.hi = g.hi;
    a.tot = (uint32_t*)ctx->cloud.tot.p, a.offs = (const uint64_t*)ctx->cloud.off.p;
    a.verts = d_verts, a.colors = d_colors, a.cap_rows = cap_rows;
    a.H = H, a.W = W, a.bgr_stride = bgr_stride, a.bpi = g.bpi;
    a.has_lo = p->lo_mode == SM_CLOUD_LO_VALUE, a.has_hi = p->has_hi != 0;
    a.handle_missing = p->handle_missing != 0, a.zero_nonfinite = p->zero_nonfinite != 0;
    const bool s16 = disp_type == SM_DISP_S16;
    if (a.handle_missing || p->lo_mode == SM_CLOUD_LO_MIN) {
        const float *mn, *lo;
        if ((rc = disp_minima_enqueue(ctx, d_disp, disp_type, nimg, g.npx, &mn, &lo)) != SM_OK) return rc;
        if (a.handle_missing) a.min_disp = mn;
        if (p->lo_mode == SM_CLOUD_LO_MIN) a.lo_dev = lo;
    }
    const dim3 grid(g.bpi, nimg), blk(smk::CLOUD_BLOCK);
    if (s16)
        hipLaunchKernelGGL(smk::k_cloud_count<int16_t>, grid, blk, 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(smk::k_cloud_count<float>, grid, blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_scan_totals, dim3(1), dim3(smk::SCAN_BLOCK), 0, ctx->stream, (const uint32_t*)ctx->cloud.tot.p,
                       (uint64_t*)ctx->cloud.off.p, g.nblk, (uint64_t*)nullptr);
    if (d_counts)
        hipLaunchKernelGGL(smk::k_seg_counts, dim3((nimg + 63) / 64), dim3(64), 0, ctx->stream,
                           (const uint64_t*)ctx->cloud.off.p, d_counts, nimg, (size_t)g.bpi);
    if (d_verts) {
        if (s16)
            hipLaunchKernelGGL(smk::k_cloud_scatter<int16_t>, grid, blk, 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(smk::k_cloud_scatter<float>, grid, blk, 0, ctx->stream, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

// blocks of CLOUD_BLOCK rows that n rows make (at least one, so that a total is always written)
int ply_blocks(sm_ctx* ctx, size_t n, size_t& nb)
{
    nb = std::max<size_t>((n + smk::CLOUD_BLOCK - 1) / smk::CLOUD_BLOCK, 1);
    if (nb > 0x7FFFFFFFull) return fail(ctx, SM_E_UNSUPPORTED, "ply: %zu rows in one call", n);
    return SM_OK;
}

// the byte lengths and their scan (the total lands in ctx->cloud.ply_off[nb] and, when given, *d_nbytes),
// then the rows themselves when d_out is given.  n_dev: the row count in device memory (n is its cap).
int ply_enqueue(sm_ctx* ctx, const float* d_verts, const uint8_t* d_colors, size_t n, const uint64_t* n_dev,
                bool measure, size_t cap_bytes, char* d_out, uint64_t* d_nbytes)
{
    size_t nb;
    int rc;
    if ((rc = ply_blocks(ctx, n, nb)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->cloud.ply_tot, nb * 4)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->cloud.ply_off, (nb + 1) * 8)) != SM_OK) return rc;
    smk::PlyArgs a{};
    a.verts = d_verts, a.colors = d_colors, a.n_dev = n_dev, a.n = n;
    a.tot = (uint32_t*)ctx->cloud.ply_tot.p, a.offs = (const uint64_t*)ctx->cloud.ply_off.p;
    a.out = d_out, a.cap_bytes = cap_bytes;
    if (measure) {
        hipLaunchKernelGGL(smk::k_ply_len, dim3((unsigned)nb), dim3(smk::CLOUD_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(smk::k_scan_totals, dim3(1), dim3(smk::SCAN_BLOCK), 0, ctx->stream,
                           (const uint32_t*)ctx->cloud.ply_tot.p, (uint64_t*)ctx->cloud.ply_off.p, nb, d_nbytes);
    }
    if (d_out) {
        if (ctx->tune_ply_stage >= 0)
            hipLaunchKernelGGL(smk::k_ply_write_lds, dim3((unsigned)nb), dim3(smk::CLOUD_BLOCK), smk::PLY_LDS_BYTES,
                               ctx->stream, a);
        else
            hipLaunchKernelGGL(smk::k_ply_write, dim3((unsigned)nb), dim3(smk::CLOUD_BLOCK), 0, ctx->stream, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

// host form: the map and its BGR image into the context's buffers
int cloud_upload(sm_ctx* ctx, const void* disp, int disp_type, const uint8_t* bgr, int bgr_stride, int H, int W)
{
    const size_t npx = (size_t)H * W, ib = npx * (disp_type == SM_DISP_S16 ? 2 : 4);
    const size_t cb = (size_t)(H - 1) * bgr_stride + 3 * (size_t)W;
    return stage_in(ctx, {{ctx->rp.in, disp, ib},
                          {ctx->rm.src, bgr, cb},
                          {ctx->cloud.verts, nullptr, npx * 12},
                          {ctx->cloud.colors, nullptr, npx * 3}});
}

}  // namespace

int sm_cloud_extract_batch_device(sm_ctx* ctx, const void* d_disp, int disp_type, const uint8_t* d_bgr,
                                  size_t bgr_img_stride_bytes, int bgr_stride, int nimg, int H, int W, const double* Q,
                                  const sm_cloud_params* p, size_t capacity_rows, float* d_verts, uint8_t* d_colors,
                                  int64_t* d_counts)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    CloudGeo g;
    int rc;
    if ((rc = cloud_check(ctx, d_disp, disp_type, d_bgr, bgr_img_stride_bytes, bgr_stride, nimg, H, W, Q, p, g)) != SM_OK)
        return rc;
    if ((d_verts == nullptr) != (d_colors == nullptr) || (!d_verts && capacity_rows))
        return fail(ctx, SM_E_ARG, "cloud: d_verts and d_colors go together (both NULL with capacity 0: counts only)");
    if (!d_verts && !d_counts) return fail(ctx, SM_E_ARG, "cloud: nothing to compute (no outputs and no counts)");
    if (nimg == 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return cloud_extract_enqueue(ctx, d_disp, disp_type, d_bgr, bgr_img_stride_bytes, bgr_stride, nimg, H, W, Q, p, g,
                                 capacity_rows, d_verts, d_colors, d_counts);
}

int sm_cloud_extract(sm_ctx* ctx, const void* disp, int disp_type, const uint8_t* bgr, int bgr_stride, int H, int W,
                     const double* Q, const sm_cloud_params* p, size_t capacity_rows, float* verts, uint8_t* colors,
                     int64_t* count)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    CloudGeo g;
    int rc;
    if ((rc = cloud_check(ctx, disp, disp_type, bgr, 0, bgr_stride, 1, H, W, Q, p, g)) != SM_OK) return rc;
    if (!count || (capacity_rows && (!verts || !colors))) return fail(ctx, SM_E_ARG, "cloud: an output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = cloud_upload(ctx, disp, disp_type, bgr, bgr_stride, H, W)) != SM_OK) return rc;
    if ((rc = cloud_extract_enqueue(ctx, ctx->rp.in.p, disp_type, (const uint8_t*)ctx->rm.src.p, 0, bgr_stride, 1, H, W, Q,
                                    p, g, g.npx, (float*)ctx->cloud.verts.p, (uint8_t*)ctx->cloud.colors.p, nullptr)) != SM_OK)
        return rc;
    uint64_t n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, (const uint64_t*)ctx->cloud.off.p + g.nblk, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *count = (int64_t)n;
    if (n > capacity_rows)
        return fail(ctx, SM_E_ARG, "cloud: %llu rows pass the mask, the capacity is %zu", (unsigned long long)n,
                    capacity_rows);
    if (!n) return SM_OK;  // nothing is queued behind the wait above
    return stage_out(ctx, {{ctx->cloud.verts, verts, n * 12}, {ctx->cloud.colors, colors, n * 3}});
}

int sm_ply_format_device(sm_ctx* ctx, const float* d_verts, const uint8_t* d_colors, size_t n, size_t capacity_bytes,
                         char* d_out, uint64_t* d_nbytes)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (n && (!d_verts || !d_colors)) return fail(ctx, SM_E_ARG, "ply: d_verts / d_colors is NULL");
    if (!d_out && (capacity_bytes || !d_nbytes))
        return fail(ctx, SM_E_ARG, "ply: d_out NULL needs capacity 0 and d_nbytes (the size query)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ply_enqueue(ctx, d_verts, d_colors, n, nullptr, true, capacity_bytes, d_out, d_nbytes);
}

int sm_cloud_ply_batch_device(sm_ctx* ctx, const void* d_disp, int disp_type, const uint8_t* d_bgr,
                              size_t bgr_img_stride_bytes, int bgr_stride, int nimg, int H, int W, const double* Q,
                              const sm_cloud_params* p, size_t capacity_bytes, char* d_out, int64_t* d_counts,
                              uint64_t* d_nbytes)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    CloudGeo g;
    int rc;
    if ((rc = cloud_check(ctx, d_disp, disp_type, d_bgr, bgr_img_stride_bytes, bgr_stride, nimg, H, W, Q, p, g)) != SM_OK)
        return rc;
    if (nimg == 0) return fail(ctx, SM_E_ARG, "cloud: nimg 0");
    if (!d_out && (capacity_bytes || !d_nbytes))
        return fail(ctx, SM_E_ARG, "ply: d_out NULL needs capacity 0 and d_nbytes (the size query)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->cloud.verts, g.rows_max * 12)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->cloud.colors, g.rows_max * 3)) != SM_OK) return rc;
    if ((rc = cloud_extract_enqueue(ctx, d_disp, disp_type, d_bgr, bgr_img_stride_bytes, bgr_stride, nimg, H, W, Q, p, g,
                                    g.rows_max, (float*)ctx->cloud.verts.p, (uint8_t*)ctx->cloud.colors.p, d_counts)) != SM_OK)
        return rc;
    return ply_enqueue(ctx, (const float*)ctx->cloud.verts.p, (const uint8_t*)ctx->cloud.colors.p, g.rows_max,
                       (const uint64_t*)ctx->cloud.off.p + g.nblk, true, capacity_bytes, d_out, d_nbytes);
}

int sm_cloud_ply(sm_ctx* ctx, const void* disp, int disp_type, const uint8_t* bgr, int bgr_stride, int H, int W,
                 const double* Q, const sm_cloud_params* p, size_t capacity_bytes, char* out, int64_t* count,
                 uint64_t* nbytes)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    CloudGeo g;
    int rc;
    if ((rc = cloud_check(ctx, disp, disp_type, bgr, 0, bgr_stride, 1, H, W, Q, p, g)) != SM_OK) return rc;
    if (!count || !nbytes || (capacity_bytes && !out)) return fail(ctx, SM_E_ARG, "cloud: an output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = cloud_upload(ctx, disp, disp_type, bgr, bgr_stride, H, W)) != SM_OK) return rc;
    if ((rc = cloud_extract_enqueue(ctx, ctx->rp.in.p, disp_type, (const uint8_t*)ctx->rm.src.p, 0, bgr_stride, 1, H, W, Q,
                                    p, g, g.npx, (float*)ctx->cloud.verts.p, (uint8_t*)ctx->cloud.colors.p, nullptr)) != SM_OK)
        return rc;
    size_t nb;
    if ((rc = ply_blocks(ctx, g.npx, nb)) != SM_OK) return rc;
    const uint64_t* n_dev = (const uint64_t*)ctx->cloud.off.p + g.nblk;
    if ((rc = ply_enqueue(ctx, (const float*)ctx->cloud.verts.p, (const uint8_t*)ctx->cloud.colors.p, g.npx, n_dev, true, 0,
                          nullptr, nullptr)) != SM_OK)
        return rc;
    uint64_t n = 0, nby = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, n_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nby, (const uint64_t*)ctx->cloud.ply_off.p + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *count = (int64_t)n;
    *nbytes = nby;
    if (nby > capacity_bytes)
        return fail(ctx, SM_E_ARG, "ply: the body is %llu bytes, the capacity is %zu", (unsigned long long)nby,
                    capacity_bytes);
    if (!nby) return SM_OK;  // nothing is queued behind the wait above
    // the rows only: the lengths and their scan are still in place (ensure of a new buffer
    // leaves the others alone)
    if ((rc = ensure(ctx, ctx->cloud.out, nby)) != SM_OK) return rc;
    if ((rc = ply_enqueue(ctx, (const float*)ctx->cloud.verts.p, (const uint8_t*)ctx->cloud.colors.p, g.npx, n_dev, false,
                          nby, (char*)ctx->cloud.out.p, nullptr)) != SM_OK)
        return rc;
    return stage_out(ctx, {{ctx->cloud.out, out, nby}});
}

int sm_ply_format_host(const float* verts, const uint8_t* colors, size_t n, size_t capacity_bytes, char* out,
                       uint64_t* nbytes)
{
    if (!nbytes || (n && (!verts || !colors)) || (capacity_bytes && !out))
        return fail(nullptr, SM_E_ARG, "ply: a required pointer is NULL");
    // rows in chunks, one thread a chunk: the lengths first, then every chunk writes at its offset
    const size_t nt = std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), 16, n / 32768}));
    const size_t per = (n + nt - 1) / nt;
    std::vector<uint64_t> len(nt, 0), at(nt + 1, 0);
    auto span = [&](size_t t, bool write) {
        const size_t r0 = std::min(n, t * per), r1 = std::min(n, r0 + per);
        if (write) {
            char* o = out + at[t];
            for (size_t r = r0; r < r1; ++r) o += smk::ply_row<true>(verts + 3 * r, colors + 3 * r, o);
        } else {
            uint64_t s = 0;
            for (size_t r = r0; r < r1; ++r) s += (uint64_t)smk::ply_row<false>(verts + 3 * r, colors + 3 * r, nullptr);
            len[t] = s;
        }
    };
    auto run = [&](bool write) {
        std::vector<std::thread> th;
        for (size_t t = 1; t < nt; ++t) th.emplace_back(span, t, write);
        span(0, write);
        for (auto& x : th) x.join();
    };
    run(false);
    for (size_t t = 0; t < nt; ++t) at[t + 1] = at[t] + len[t];
    *nbytes = at[nt];
    if (at[nt] > capacity_bytes)
        return fail(nullptr, SM_E_ARG, "ply: the body is %llu bytes, the capacity is %zu", (unsigned long long)at[nt],
                    capacity_bytes);
    run(true);
    return SM_OK;
}

}  // extern "C"
