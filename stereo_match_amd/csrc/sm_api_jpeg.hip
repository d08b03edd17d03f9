// sm_api_jpeg.hip — C-ABI of baseline JPEG input (sm_jpegdec.hpp).  The only unit with these kernels.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sm_ctx.hpp"
#include "sm_jpegdec.hpp"

extern "C" {

// ---- JPEG input (sm_jpegdec.hpp)
namespace {

thread_local int g_jd_host_nsub = 0;  // lanes the last sm_jpeg_decode_host would have used

int jpegdec_code(int status)
{
    if (status == smk::JD_OK) return SM_OK;
    return smk::jpegdec_unsupported(status) ? SM_E_UNSUPPORTED : SM_E_DATA;
}

int jpegdec_fail(sm_ctx* ctx, int status)
{
    return fail(ctx, jpegdec_code(status), "jpeg decode: %s", smk::jpegdec_message(status));
}

// the checks and the geometry of all entry points (ctx NULL: the CPU twin)
int jpegdec_setup(sm_ctx* ctx, int nimg, int H, int W, const sm_jpegdec_params* p, int fch, int sub, const void* out,
                  size_t img_stride, size_t row_stride, smk::JdArgs& a)
{
    if (!p || !out) return fail(ctx, SM_E_ARG, "jpeg decode: a required pointer is NULL");
    if (nimg < 1 || nimg > 65535) return fail(ctx, SM_E_ARG, "jpeg decode: nimg %d", nimg);
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return fail(ctx, SM_E_ARG, "jpeg decode: image size %dx%d", W, H);
    if ((size_t)H * (size_t)W >= (1u << 28))
        return fail(ctx, SM_E_UNSUPPORTED, "jpeg decode: %s", smk::jpegdec_message(smk::JD_E_SIZE));
    if (!((fch == 1) || (fch == 3 && (sub == 444 || sub == 422 || sub == 420))))
        return fail(ctx, SM_E_ARG, "jpeg decode: file_channels %d with subsampling %d (1, or 3 with 444, 422 or 420)", fch, sub);
    if (p->flags < -1 || p->flags > 1) return fail(ctx, SM_E_ARG, "jpeg decode: flags %d (1, 0 or -1)", p->flags);
    a = smk::JdArgs{};
    a.nimg = nimg, a.H = H, a.W = W, a.ncomp = fch;
    a.hs = fch == 3 && sub != 444 ? 2 : 1, a.vs = fch == 3 && sub == 420 ? 2 : 1;
    a.out_ch = p->flags == 1 ? 3 : p->flags == 0 ? 1 : fch;
    a.y_only = a.out_ch == 1 || fch == 1, a.keep = p->keep_channel_order != 0;
    const size_t opb = (size_t)a.out_ch;
    if (row_stride < (size_t)W * opb)
        return fail(ctx, SM_E_ARG, "jpeg decode: row_stride_bytes %zu smaller than a row (%zu)", row_stride, (size_t)W * opb);
    if (nimg > 1 && img_stride < (size_t)(H - 1) * row_stride + (size_t)W * opb)
        return fail(ctx, SM_E_ARG, "jpeg decode: img_stride_bytes %zu smaller than one image", img_stride);
    smk::jd_geometry(a);
    a.out = static_cast<uint8_t*>(const_cast<void*>(out)), a.img_stride = img_stride, a.row_stride = row_stride;
    return SM_OK;
}

}  // namespace

const char* sm_jpegdec_status_message(int status) { return smk::jpegdec_message(status); }

int sm_jpegdec_status_code(int status) { return jpegdec_code(status); }

size_t sm_jpeg_desc_bytes(void) { return sizeof(smk::JdDesc); }

int sm_jpeg_parse(const uint8_t* file, size_t nbytes, void* desc, int* status)
{
    if (!file || !desc) return fail(nullptr, SM_E_ARG, "jpeg parse: a required pointer is NULL");
    smk::JdDesc d;
    const int st = smk::jd_parse(file, nbytes, d);
    std::memcpy(desc, &d, sizeof d);
    if (status) *status = st;
    return st ? jpegdec_fail(nullptr, st) : SM_OK;
}

int sm_jpeg_info(const uint8_t* file, size_t nbytes, int* H, int* W, int* channels, int* subsampling)
{
    if (!file || !H || !W || !channels || !subsampling) return fail(nullptr, SM_E_ARG, "jpeg info: a required pointer is NULL");
    smk::JdDesc d;
    const int st = smk::jd_parse(file, nbytes, d);
    if (st) return jpegdec_fail(nullptr, st);
    *H = (int)d.H, *W = (int)d.W, *channels = d.ncomp, *subsampling = smk::jd_subsampling(d);
    return SM_OK;
}

int sm_jpeg_decode_batch_device(sm_ctx* ctx, const uint8_t* d_files, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                int nimg, int H, int W, const sm_jpegdec_params* p, void* d_out, size_t img_stride_bytes,
                                size_t row_stride_bytes, int* d_status)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_files || !d_offsets || !d_sizes || !d_status || !p || !p->d_desc)
        return fail(ctx, SM_E_ARG, "jpeg decode: a required pointer is NULL");
    smk::JdArgs a;
    int rc;
    if ((rc = jpegdec_setup(ctx, nimg, H, W, p, p->file_channels, p->subsampling, d_out, img_stride_bytes, row_stride_bytes,
                            a)) != SM_OK)
        return rc;
    if (p->max_file_bytes < 1 || p->max_file_bytes > smk::JD_MAX_FILE)
        return fail(ctx, SM_E_ARG, "jpeg decode: max_file_bytes %llu (1 .. 2^28 - 1)", (unsigned long long)p->max_file_bytes);
    a.files = d_files, a.offsets = d_offsets, a.sizes = d_sizes, a.desc = static_cast<const smk::JdDesc*>(p->d_desc);
    a.max_file = (uint32_t)p->max_file_bytes;
    a.iv_cap = a.nmcu;
    a.lane_cap = (a.max_file + smk::JD_SUBSEQ - 1) / smk::JD_SUBSEQ + a.nmcu + 1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)nimg, ivn = n * (a.iv_cap + 1), ln = n * a.lane_cap;
    const size_t coef_bytes = n * a.nmcu * a.bpm * 64 * sizeof(int16_t);
    if ((rc = ensure(ctx, ctx->jpegdec.img, n * sizeof(smk::JdImg))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->jpegdec.iv, 3 * ivn * sizeof(uint32_t))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->jpegdec.state, 3 * ln * sizeof(smk::JdState))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->jpegdec.lane, ln * (3 * sizeof(uint32_t) + 1))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->jpegdec.coef, coef_bytes)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->jpegdec.planes, n * a.plane_stride)) != SM_OK) return rc;
    a.img = (smk::JdImg*)ctx->jpegdec.img.p;
    a.ibeg = (uint32_t*)ctx->jpegdec.iv.p, a.iend = a.ibeg + ivn, a.ilane = a.iend + ivn;
    a.start = (smk::JdState*)ctx->jpegdec.state.p, a.exit_a = a.start + ln, a.exit_b = a.exit_a + ln;
    a.nblk = (uint32_t*)ctx->jpegdec.lane.p, a.lane_iv = a.nblk + ln, a.gpre = a.lane_iv + ln, a.flag = (uint8_t*)(a.gpre + ln);
    a.coef = (int16_t*)ctx->jpegdec.coef.p, a.planes = (uint8_t*)ctx->jpegdec.planes.p;
    HIP_TRY(ctx, hipMemsetAsync(ctx->jpegdec.coef.p, 0, coef_bytes, ctx->stream));
    const dim3 blk(smk::JD_BLOCK);
    const uint32_t lgrid = (a.lane_cap + smk::JD_BLOCK - 1) / smk::JD_BLOCK;
    const uint32_t nblocks = a.nmcu * a.bpm;
    hipLaunchKernelGGL(smk::k_jpeg_split, dim3(nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_sync_a, dim3(lgrid, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_sync_b, dim3(lgrid, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_sync_loop, dim3(nimg), dim3(smk::JD_LOOP_BLOCK), 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_write, dim3(lgrid, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_dc, dim3(a.y_only ? 1 : a.ncomp, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_idct, dim3((nblocks + 31) / 32, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_color, dim3((W + smk::JD_BLOCK - 1) / smk::JD_BLOCK, (H + 1) / 2, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_jpeg_status, dim3((nimg + smk::JD_BLOCK - 1) / smk::JD_BLOCK), blk, 0, ctx->stream, a, d_status);
    HIP_TRY(ctx, hipGetLastError());
    ctx->jpegdec.last_nimg = nimg;
    return SM_OK;
}

int sm_jpeg_decode(sm_ctx* ctx, const uint8_t* file, size_t nbytes, const sm_jpegdec_params* p, void* out,
                   size_t row_stride_bytes, int* status)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!file || !p || !out) return fail(ctx, SM_E_ARG, "jpeg decode: a required pointer is NULL");
    if (status) *status = 0;
    smk::JdDesc d;
    int st = smk::jd_parse(file, nbytes, d);
    if (st) {
        if (status) *status = st;
        return jpegdec_fail(ctx, st);
    }
    sm_jpegdec_params q = *p;
    if (!q.file_channels) q.file_channels = d.ncomp, q.subsampling = smk::jd_subsampling(d);
    q.max_file_bytes = nbytes;
    smk::JdArgs a;
    int rc;
    if ((rc = jpegdec_setup(ctx, 1, (int)d.H, (int)d.W, &q, q.file_channels, q.subsampling, out, 0, row_stride_bytes, a)) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t drow = (size_t)d.W * a.out_ch;
    const uint64_t tab[2] = {0, (uint64_t)nbytes};
    if ((rc = stage_in(ctx, {{ctx->jpegdec.in, file, nbytes},
                             {ctx->jpegdec.desc, &d, sizeof d},
                             {ctx->jpegdec.tab, tab, 16},
                             {ctx->jpegdec.out, nullptr, drow, d.H},
                             {ctx->jpegdec.status, nullptr, 4}})) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // d and tab live on this frame
    q.d_desc = ctx->jpegdec.desc.p;
    const uint64_t* dtab = (const uint64_t*)ctx->jpegdec.tab.p;
    if ((rc = sm_jpeg_decode_batch_device(ctx, (const uint8_t*)ctx->jpegdec.in.p, dtab, dtab + 1, 1, (int)d.H, (int)d.W, &q,
                                          ctx->jpegdec.out.p, 0, drow, (int*)ctx->jpegdec.status.p)) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(&st, ctx->jpegdec.status.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (status) *status = st;
    if (st) return jpegdec_fail(ctx, st);
    return stage_out(ctx, {{ctx->jpegdec.out, out, drow, d.H, row_stride_bytes}});
}

int sm_jpeg_decode_host(const uint8_t* file, size_t nbytes, const sm_jpegdec_params* p, void* out, size_t row_stride_bytes,
                        int* status)
{
    if (!file || !p || !out) return fail(nullptr, SM_E_ARG, "jpeg decode: a required pointer is NULL");
    if (status) *status = 0;
    g_jd_host_nsub = 0;
    smk::JdDesc d;
    int st = smk::jd_parse(file, nbytes, d);
    if (!st) {
        const int fch = p->file_channels ? p->file_channels : d.ncomp;
        const int sub = p->file_channels ? p->subsampling : smk::jd_subsampling(d);
        smk::JdArgs a;
        int rc;
        if ((rc = jpegdec_setup(nullptr, 1, (int)d.H, (int)d.W, p, fch, sub, out, 0, row_stride_bytes, a)) != SM_OK) return rc;
        const uint64_t off = 0, size = nbytes;
        a.files = file, a.offsets = &off, a.sizes = &size, a.desc = &d, a.max_file = (uint32_t)nbytes;
        uint32_t nsub = 0;
        st = smk::jpegdec_host(a, nsub);
        g_jd_host_nsub = (int)nsub;
    }
    if (status) *status = st;
    return st ? jpegdec_fail(nullptr, st) : SM_OK;
}

int sm_jpeg_decode_stats(sm_ctx* ctx, int* n_subsequences, int* n_sync_rounds)
{
    if (!n_subsequences || !n_sync_rounds) return fail(ctx, SM_E_ARG, "jpeg decode: a required pointer is NULL");
    *n_subsequences = *n_sync_rounds = 0;
    if (!ctx) {
        *n_subsequences = g_jd_host_nsub;
        return SM_OK;
    }
    if (ctx->jpegdec.last_nimg <= 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<smk::JdImg> v((size_t)ctx->jpegdec.last_nimg);
    HIP_TRY(ctx, hipMemcpyAsync(v.data(), ctx->jpegdec.img.p, v.size() * sizeof(smk::JdImg), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const smk::JdImg& im : v) {
        *n_subsequences += (int)im.nsub;
        *n_sync_rounds = std::max(*n_sync_rounds, (int)im.rounds);
    }
    return SM_OK;
}

}  // extern "C"
