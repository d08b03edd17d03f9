// sm_api_png.hip — C-ABI of PNG output (sm_png.hpp) and PNG input (sm_pngdec.hpp, which includes
// sm_png.hpp; png_bound_of serves both).  The only unit with these kernels.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sm_ctx.hpp"
#include "sm_png.hpp"
#include "sm_pngdec.hpp"

extern "C" {

// ---- PNG output (sm_png.hpp)
namespace {

// the checks and the geometry of all three entry points (ctx NULL: the CPU twin)
int png_setup(sm_ctx* ctx, const void* img, size_t img_stride, size_t row_stride, int nimg, int H, int W,
              const sm_png_params* p, smk::PngArgs& a)
{
    if (!img || !p) return fail(ctx, SM_E_ARG, "png: a required pointer is NULL");
    if (H <= 0 || W <= 0) return fail(ctx, SM_E_ARG, "png: empty image (%dx%d)", W, H);
    if (nimg < 1 || nimg > 65535) return fail(ctx, SM_E_ARG, "png: nimg %d", nimg);
    if (p->src_kind < SM_PNG_SRC_U8 || p->src_kind > SM_PNG_SRC_DISP_F32)
        return fail(ctx, SM_E_ARG, "png: src_kind %d unknown", p->src_kind);
    const bool disp = p->src_kind >= SM_PNG_SRC_DISP_I16;
    if (p->src_kind == SM_PNG_SRC_U8 ? (p->channels != 1 && p->channels != 3) : p->channels != 1)
        return fail(ctx, SM_E_ARG, "png: %d channels (uint8: 1 or 3; uint16 and disparity maps: 1)", p->channels);
    if (p->filter < -1 || p->filter > 4) return fail(ctx, SM_E_ARG, "png: filter %d (-1 adaptive, 0..4)", p->filter);
    if (disp && p->disp_mode != SM_PNG_DISP_KITTI && p->disp_mode != SM_PNG_DISP_LINEAR_U8)
        return fail(ctx, SM_E_ARG, "png: disp_mode %d unknown", p->disp_mode);
    const bool linear = disp && p->disp_mode == SM_PNG_DISP_LINEAR_U8;
    if (linear && p->src_kind == SM_PNG_SRC_DISP_F32)
        return fail(ctx, SM_E_UNSUPPORTED, "png: SM_PNG_DISP_LINEAR_U8 takes an int16 map");
    if (linear && p->has_bounds && p->hi < p->lo) return fail(ctx, SM_E_ARG, "png: hi %d < lo %d", p->hi, p->lo);
    const size_t esz = p->src_kind == SM_PNG_SRC_U8 ? 1 : p->src_kind == SM_PNG_SRC_DISP_F32 ? 4 : 2;
    const size_t src_row = (size_t)W * esz * (size_t)p->channels;
    if (row_stride < src_row) return fail(ctx, SM_E_ARG, "png: row_stride_bytes %zu smaller than a row (%zu)", row_stride, src_row);
    if (nimg > 1 && img_stride < (size_t)(H - 1) * row_stride + src_row)
        return fail(ctx, SM_E_ARG, "png: img_stride_bytes %zu smaller than one image", img_stride);
    if (row_stride % esz || (nimg > 1 && img_stride % esz) || reinterpret_cast<uintptr_t>(img) % esz)
        return fail(ctx, SM_E_ARG, "png: the image is not aligned to its %zu-byte samples", esz);
    a = smk::PngArgs{};
    a.img = static_cast<const uint8_t*>(img), a.img_stride = img_stride, a.row_stride = row_stride;
    a.H = H, a.W = W;
    a.kind = p->src_kind, a.channels = p->channels, a.keep = p->keep_channel_order != 0, a.filter = p->filter;
    a.mode = disp ? p->disp_mode : 0;
    a.lo = p->lo, a.hi = p->hi;
    a.depth = (p->src_kind == SM_PNG_SRC_U16 || (disp && !linear)) ? 16 : 8;
    a.out_channels = p->channels;
    a.bpp = a.out_channels * a.depth / 8;
    const uint64_t rowbytes = (uint64_t)W * a.bpp, stream = (rowbytes + 1) * (uint64_t)H;
    if (stream >= (1ull << 31)) return fail(ctx, SM_E_UNSUPPORTED, "png: a filtered stream of %llu bytes (2^31 and more)", (unsigned long long)stream);
    a.rowbytes = (uint32_t)rowbytes, a.stream_len = stream, a.stream_stride = (stream + 15) & ~15ull;
    a.nseg = (uint32_t)((stream + smk::PNG_SEG - 1) / smk::PNG_SEG);
    return SM_OK;
}

size_t png_bound_of(uint64_t stream, uint32_t nseg) { return (size_t)(57 + 6 + 17ull * nseg + stream); }

}  // namespace

size_t sm_png_bound(int H, int W, int channels, int depth)
{
    if (H <= 0 || W <= 0 || (channels != 1 && channels != 3) || (depth != 8 && depth != 16) || (channels == 3 && depth == 16))
        return 0;
    const uint64_t stream = ((uint64_t)W * channels * (depth / 8) + 1) * (uint64_t)H;
    if (stream >= (1ull << 31)) return 0;
    return png_bound_of(stream, (uint32_t)((stream + smk::PNG_SEG - 1) / smk::PNG_SEG));
}

int sm_png_encode_batch_device(sm_ctx* ctx, const void* d_img, size_t img_stride_bytes, size_t row_stride_bytes,
                               int nimg, int H, int W, const sm_png_params* p, size_t capacity_bytes, uint8_t* d_out,
                               uint64_t* d_nbytes)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    smk::PngArgs a;
    int rc;
    if ((rc = png_setup(ctx, d_img, img_stride_bytes, row_stride_bytes, nimg, H, W, p, a)) != SM_OK) return rc;
    if (!d_out && (capacity_bytes || !d_nbytes))
        return fail(ctx, SM_E_ARG, "png: d_out NULL needs capacity 0 and d_nbytes (the size query)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nchunk = (size_t)nimg * a.nseg;
    if ((rc = ensure(ctx, ctx->png.stream, (size_t)nimg * a.stream_stride)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->png.slots, nchunk * smk::PNG_SLOT)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->png.seg, nchunk * sizeof(smk::PngSegInfo))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->png.off, nchunk * 8)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->png.img, (size_t)nimg * sizeof(smk::PngImgInfo))) != SM_OK) return rc;
    if (!d_nbytes) {
        if ((rc = ensure(ctx, ctx->png.nb, (size_t)nimg * 8)) != SM_OK) return rc;
        d_nbytes = (uint64_t*)ctx->png.nb.p;
    }
    a.stream = (uint8_t*)ctx->png.stream.p, a.slots = (uint8_t*)ctx->png.slots.p;
    a.seginfo = (smk::PngSegInfo*)ctx->png.seg.p, a.offs = (uint64_t*)ctx->png.off.p;
    a.imginfo = (smk::PngImgInfo*)ctx->png.img.p;
    a.out = d_out, a.capacity = capacity_bytes, a.nbytes = d_nbytes;
    const dim3 blk(smk::PNG_BLOCK);
    if (a.kind == SM_PNG_SRC_DISP_I16 && a.mode == SM_PNG_DISP_LINEAR_U8 && !p->has_bounds) {
        if ((rc = ensure(ctx, ctx->png.range, (size_t)nimg * 8)) != SM_OK) return rc;
        int* keys = (int*)ctx->png.range.p;
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)keys, 0x7FFFFFFF, 2 * (size_t)nimg, ctx->stream));
        hipLaunchKernelGGL(smk::k_png_minmax, dim3(std::min(H, 64), nimg), blk, 0, ctx->stream, a, keys);
        a.range = keys;
    }
    const dim3 fgrid((H + smk::PNG_FILTER_ROWS - 1) / smk::PNG_FILTER_ROWS, nimg);
    if (a.rowbytes <= smk::PNG_MAX_ROW) {
        const size_t flds = (size_t)(smk::PNG_FILTER_ROWS + 1) * ((a.rowbytes + 3u) & ~3u);
        if (flds > 48 * 1024)  // above the default limit of dynamic LDS
            HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(smk::k_png_filter<true>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)flds));
        hipLaunchKernelGGL(smk::k_png_filter<true>, fgrid, blk, flds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(smk::k_png_filter<false>, fgrid, blk, 0, ctx->stream, a);
    }
    const size_t dlds = sizeof(smk::PngDeflateLds);
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(smk::k_png_deflate),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)dlds));
    hipLaunchKernelGGL(smk::k_png_deflate, dim3(a.nseg, nimg), dim3(smk::PNG_DBLOCK), dlds, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_png_assemble, dim3(nimg), blk, 0, ctx->stream, a);
    if (d_out) hipLaunchKernelGGL(smk::k_png_scatter, dim3(a.nseg, nimg), blk, 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SM_OK;
}

int sm_png_encode(sm_ctx* ctx, const void* img, size_t row_stride_bytes, int H, int W, const sm_png_params* p,
                  size_t capacity_bytes, uint8_t* out, uint64_t* nbytes)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    smk::PngArgs a;
    int rc;
    if ((rc = png_setup(ctx, img, 0, row_stride_bytes, 1, H, W, p, a)) != SM_OK) return rc;
    if (!nbytes || (capacity_bytes && !out)) return fail(ctx, SM_E_ARG, "png: an output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t esz = a.kind == SM_PNG_SRC_U8 ? 1 : a.kind == SM_PNG_SRC_DISP_F32 ? 4 : 2;
    const size_t ib = (size_t)(H - 1) * row_stride_bytes + (size_t)W * esz * a.channels;
    const size_t bound = png_bound_of(a.stream_len, a.nseg);
    if ((rc = stage_in(ctx, {{ctx->png.in, img, ib}, {ctx->png.out, nullptr, bound}, {ctx->png.nb, nullptr, 8}})) != SM_OK)
        return rc;
    if ((rc = sm_png_encode_batch_device(ctx, ctx->png.in.p, 0, row_stride_bytes, 1, H, W, p, bound,
                                         (uint8_t*)ctx->png.out.p, (uint64_t*)ctx->png.nb.p)) != SM_OK)
        return rc;
    uint64_t n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, ctx->png.nb.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *nbytes = n;
    if (n > capacity_bytes)
        return fail(ctx, SM_E_ARG, "png: the file is %llu bytes, the capacity is %zu", (unsigned long long)n, capacity_bytes);
    return stage_out(ctx, {{ctx->png.out, out, n}});
}

int sm_png_encode_host(const void* img, size_t row_stride_bytes, int H, int W, const sm_png_params* p,
                       size_t capacity_bytes, uint8_t* out, uint64_t* nbytes)
{
    smk::PngArgs a;
    int rc;
    if ((rc = png_setup(nullptr, img, 0, row_stride_bytes, 1, H, W, p, a)) != SM_OK) return rc;
    if (!nbytes || (capacity_bytes && !out)) return fail(nullptr, SM_E_ARG, "png: an output pointer is NULL");
    if (a.kind == SM_PNG_SRC_DISP_I16 && a.mode == SM_PNG_DISP_LINEAR_U8 && !p->has_bounds) {
        int lo = 0x7FFFFFFF, hi = -0x7FFFFFFF;
        for (int y = 0; y < H; ++y) {
            const int16_t* row = reinterpret_cast<const int16_t*>(a.img + (size_t)y * row_stride_bytes);
            for (int x = 0; x < W; ++x) lo = std::min(lo, (int)row[x]), hi = std::max(hi, (int)row[x]);
        }
        a.lo = lo, a.hi = hi;
    }
    std::vector<uint8_t> file;
    smk::png_encode_host(a, file);
    *nbytes = file.size();
    if (file.size() > capacity_bytes)
        return fail(nullptr, SM_E_ARG, "png: the file is %zu bytes, the capacity is %zu", file.size(), capacity_bytes);
    std::memcpy(out, file.data(), file.size());
    return SM_OK;
}

// ---- PNG input (sm_pngdec.hpp)
namespace {

thread_local int g_pd_host_path[2] = {0, 0};  // the last sm_png_decode_host: parallel, serial

int pngdec_code(int status)
{
    if (status == smk::PD_OK) return SM_OK;
    return (status >= smk::PD_E_INTERLACE && status <= smk::PD_E_SIZE) ? SM_E_UNSUPPORTED : SM_E_DATA;
}

int pngdec_fail(sm_ctx* ctx, int status, int index)
{
    const int code = pngdec_code(status);
    if (index >= 0) return fail(ctx, code, "png decode: image %d: %s", index, smk::pngdec_message(status));
    return fail(ctx, code, "png decode: %s", smk::pngdec_message(status));
}

// IHDR of a file in host memory: a status of the decoder
int pngdec_info(const uint8_t* f, size_t n, smk::PdHdr& h)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8 || std::memcmp(f, sig, 8) != 0) return smk::PD_E_SIG;
    if (n < 33) return smk::PD_E_TRUNC;
    if (smk::pd_be32(f + 8) != 13u || std::memcmp(f + 12, "IHDR", 4) != 0) return smk::PD_E_IHDR;
    return smk::pd_ihdr(f + 16, h);
}

// the checks and the geometry of all entry points (ctx NULL: the CPU twin)
int pngdec_setup(sm_ctx* ctx, int nimg, int H, int W, const sm_pngdec_params* p, int fch, int fdepth, const void* out,
                 size_t img_stride, size_t row_stride, smk::PdArgs& a)
{
    if (!p || !out) return fail(ctx, SM_E_ARG, "png decode: a required pointer is NULL");
    if (nimg < 1 || nimg > 65535) return fail(ctx, SM_E_ARG, "png decode: nimg %d", nimg);
    if (H < 1 || W < 1) return fail(ctx, SM_E_ARG, "png decode: empty image (%dx%d)", W, H);
    if ((fch != 1 && fch != 3 && fch != 4) || (fdepth != 8 && fdepth != 16) || (fdepth == 16 && fch != 1))
        return fail(ctx, SM_E_ARG, "png decode: file_channels %d at file_depth %d (1 at 8 or 16; 3 or 4 at 8)", fch, fdepth);
    if (p->out_kind < SM_PNGDEC_U8 || p->out_kind > SM_PNGDEC_DISP_F32)
        return fail(ctx, SM_E_ARG, "png decode: out_kind %d unknown", p->out_kind);
    if (p->flags < -1 || p->flags > 1) return fail(ctx, SM_E_ARG, "png decode: flags %d (1, 0 or -1)", p->flags);
    a = smk::PdArgs{};
    a.kind = p->out_kind, a.keep = p->keep_channel_order != 0, a.inv_i16 = p->invalid_i16, a.inv_f32 = p->invalid_f32;
    size_t opb;
    if (p->out_kind == SM_PNGDEC_U8) {
        if (p->flags == -1 && fdepth == 16)
            return fail(ctx, SM_E_ARG, "png decode: flags -1 on a 16-bit file needs out_kind SM_PNGDEC_U16");
        a.out_ch = p->flags == 1 ? 3 : p->flags == 0 ? 1 : (fch == 1 ? 1 : 3);
        opb = (size_t)a.out_ch;
    } else {
        if (fdepth != 16 || fch != 1)
            return fail(ctx, SM_E_UNSUPPORTED, "png decode: out_kind %d takes a 16-bit gray file, not %d channel(s) at depth %d",
                        p->out_kind, fch, fdepth);
        if (p->flags != -1) return fail(ctx, SM_E_ARG, "png decode: out_kind %d takes flags -1", p->out_kind);
        if (p->out_kind != SM_PNGDEC_U16 && p->disp_mode != SM_PNG_DISP_KITTI)
            return fail(ctx, SM_E_UNSUPPORTED, "png decode: only SM_PNG_DISP_KITTI maps are read back");
        a.out_ch = 1;
        opb = p->out_kind == SM_PNGDEC_DISP_F32 ? 4 : 2;
    }
    const size_t esz = p->out_kind == SM_PNGDEC_U8 ? 1 : opb;
    if (row_stride < (size_t)W * opb)
        return fail(ctx, SM_E_ARG, "png decode: row_stride_bytes %zu smaller than a row (%zu)", row_stride, (size_t)W * opb);
    if (nimg > 1 && img_stride < (size_t)(H - 1) * row_stride + (size_t)W * opb)
        return fail(ctx, SM_E_ARG, "png decode: img_stride_bytes %zu smaller than one image", img_stride);
    if (row_stride % esz || (nimg > 1 && img_stride % esz) || reinterpret_cast<uintptr_t>(out) % esz)
        return fail(ctx, SM_E_ARG, "png decode: the output is not aligned to its %zu-byte samples", esz);
    a.nimg = nimg, a.H = H, a.W = W, a.file_ch = fch, a.depth = fdepth, a.bpp = fch * fdepth / 8;
    const uint64_t rowbytes = (uint64_t)W * a.bpp, stream = (rowbytes + 1) * (uint64_t)H;
    if (stream >= (1ull << 31))
        return fail(ctx, SM_E_UNSUPPORTED, "png decode: a filtered stream of %llu bytes (2^31 and more)", (unsigned long long)stream);
    a.rowbytes = (uint32_t)rowbytes, a.stream_len = stream, a.stream_stride = (stream + 15) & ~15ull;
    a.nseg = (uint32_t)((stream + smk::PNG_SEG - 1) / smk::PNG_SEG);
    a.maxpar = 2u * (uint32_t)((stream + smk::PNGDEC_CAP - 1) / smk::PNGDEC_CAP) + 4u;
    a.out = static_cast<uint8_t*>(const_cast<void*>(out)), a.img_stride = img_stride, a.row_stride = row_stride;
    return SM_OK;
}

}  // namespace

const char* sm_pngdec_status_message(int status) { return smk::pngdec_message(status); }

int sm_pngdec_status_code(int status) { return pngdec_code(status); }

int sm_png_info(const uint8_t* file, size_t nbytes, int* H, int* W, int* channels, int* depth)
{
    if (!file || !H || !W || !channels || !depth) return fail(nullptr, SM_E_ARG, "png info: a required pointer is NULL");
    smk::PdHdr h{};
    const int st = pngdec_info(file, nbytes, h);
    if (st) return pngdec_fail(nullptr, st, -1);
    *H = (int)h.H, *W = (int)h.W, *channels = h.channels, *depth = h.depth;
    return SM_OK;
}

int sm_png_decode_batch_device(sm_ctx* ctx, const uint8_t* d_files, const uint64_t* d_offsets, const uint64_t* d_sizes,
                               int nimg, int H, int W, const sm_pngdec_params* p, void* d_out, size_t img_stride_bytes,
                               size_t row_stride_bytes, int* d_status)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!d_files || !d_offsets || !d_sizes || !d_status) return fail(ctx, SM_E_ARG, "png decode: a required pointer is NULL");
    smk::PdArgs a;
    int rc;
    if ((rc = pngdec_setup(ctx, nimg, H, W, p, p ? p->file_channels : 0, p ? p->file_depth : 0, d_out, img_stride_bytes,
                           row_stride_bytes, a)) != SM_OK)
        return rc;
    if (p->max_chunks < 0) return fail(ctx, SM_E_ARG, "png decode: max_chunks %d", p->max_chunks);
    a.files = d_files, a.offsets = d_offsets, a.sizes = d_sizes;
    a.max_chunks = p->max_chunks ? (uint32_t)p->max_chunks : 2u * a.nseg + 64u;
    a.max_file = p->max_file_bytes ? p->max_file_bytes : 2ull * png_bound_of(a.stream_len, a.nseg);
    if (a.max_file > 0xFFFFFFFFull) a.max_file = 0xFFFFFFFFull;
    a.zstride = (a.max_file + 15) & ~15ull;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)nimg;
    if ((rc = ensure(ctx, ctx->pngdec.img, n * sizeof(smk::PdImg))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->pngdec.chunks, n * a.max_chunks * sizeof(smk::PdChunk))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->pngdec.idat, n * a.max_chunks * sizeof(smk::PdIdat))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->pngdec.cinfo, n * a.maxpar * sizeof(smk::PdChunkInfo))) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->pngdec.slots, n * a.maxpar * smk::PNGDEC_CAP)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->pngdec.zbuf, n * a.zstride)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->pngdec.stream, n * a.stream_stride)) != SM_OK) return rc;
    if ((rc = ensure(ctx, ctx->pngdec.seg, n * a.nseg * sizeof(smk::PdChunkInfo))) != SM_OK) return rc;
    const uint32_t ngrp = (uint32_t)((H + 63) / 64);  // row groups of the unfilter pass
    if ((rc = ensure(ctx, ctx->pngdec.carry, n * ngrp * (size_t)W * 4)) != SM_OK) return rc;
    a.img = (smk::PdImg*)ctx->pngdec.img.p, a.chunks = (smk::PdChunk*)ctx->pngdec.chunks.p, a.idat = (smk::PdIdat*)ctx->pngdec.idat.p;
    a.cinfo = (smk::PdChunkInfo*)ctx->pngdec.cinfo.p, a.slots = (uint8_t*)ctx->pngdec.slots.p, a.zbuf = (uint8_t*)ctx->pngdec.zbuf.p;
    a.stream = (uint8_t*)ctx->pngdec.stream.p, a.seg = (smk::PdChunkInfo*)ctx->pngdec.seg.p, a.carry = (uint32_t*)ctx->pngdec.carry.p;
    const dim3 blk(smk::PNGDEC_BLOCK), wave(64);
    const uint32_t cgrid = std::min<uint32_t>(a.max_chunks, 256u);
    hipLaunchKernelGGL(smk::k_pngdec_parse, dim3(nimg), wave, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_crc, dim3(cgrid, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_inflate, dim3(a.maxpar, nimg), wave, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_place, dim3(nimg), wave, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_compact, dim3(a.maxpar, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_gather, dim3(cgrid, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_inflate_serial, dim3(nimg), wave, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_adler, dim3(a.nseg, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_verify, dim3(nimg), wave, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_unfilter, dim3(ngrp, nimg), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(smk::k_pngdec_status, dim3((nimg + 255) / 256), blk, 0, ctx->stream, a, d_status);
    HIP_TRY(ctx, hipGetLastError());
    ctx->pngdec.last_nimg = nimg;
    return SM_OK;
}

int sm_png_decode(sm_ctx* ctx, const uint8_t* file, size_t nbytes, const sm_pngdec_params* p, void* out,
                  size_t row_stride_bytes, int* status)
{
    if (!ctx) return fail(nullptr, SM_E_ARG, "ctx is NULL");
    if (!file || !p || !out) return fail(ctx, SM_E_ARG, "png decode: a required pointer is NULL");
    if (status) *status = 0;
    smk::PdHdr h{};
    int st = pngdec_info(file, nbytes, h);
    if (st) {
        if (status) *status = st;
        return pngdec_fail(ctx, st, -1);
    }
    sm_pngdec_params q = *p;
    if (!q.file_channels) q.file_channels = h.channels;
    if (!q.file_depth) q.file_depth = h.depth;
    {  // the chunks the walk on the device can meet: counted here, every length checked first
        size_t pos = 8, nc = 0;
        while (nbytes - pos >= 12) {
            const uint32_t len = smk::pd_be32(file + pos);
            ++nc;
            if ((uint64_t)len > nbytes - pos - 12) break;
            pos += 12 + (size_t)len;
        }
        q.max_chunks = (int)std::min<size_t>(nc + 1, 0x7FFFFFFF);
    }
    q.max_file_bytes = nbytes;
    smk::PdArgs a;
    int rc;
    if ((rc = pngdec_setup(ctx, 1, (int)h.H, (int)h.W, &q, q.file_channels, q.file_depth, out, 0, row_stride_bytes, a)) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t opb = a.kind == SM_PNGDEC_U8 ? (size_t)a.out_ch : a.kind == SM_PNGDEC_DISP_F32 ? 4 : 2;
    const size_t drow = (size_t)h.W * opb;
    const uint64_t tab[2] = {0, (uint64_t)nbytes};
    if ((rc = stage_in(ctx, {{ctx->pngdec.in, file, nbytes},
                             {ctx->pngdec.tab, tab, 16},
                             {ctx->pngdec.out, nullptr, drow, h.H},
                             {ctx->pngdec.status, nullptr, 4}})) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // tab lives on this frame
    const uint64_t* dtab = (const uint64_t*)ctx->pngdec.tab.p;
    if ((rc = sm_png_decode_batch_device(ctx, (const uint8_t*)ctx->pngdec.in.p, dtab, dtab + 1, 1, (int)h.H, (int)h.W, &q,
                                         ctx->pngdec.out.p, 0, drow, (int*)ctx->pngdec.status.p)) != SM_OK)
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(&st, ctx->pngdec.status.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (status) *status = st;
    if (st) return pngdec_fail(ctx, st, -1);
    return stage_out(ctx, {{ctx->pngdec.out, out, drow, h.H, row_stride_bytes}});
}

int sm_png_decode_host(const uint8_t* file, size_t nbytes, const sm_pngdec_params* p, void* out, size_t row_stride_bytes,
                       int* status)
{
    if (!file || !p || !out) return fail(nullptr, SM_E_ARG, "png decode: a required pointer is NULL");
    if (status) *status = 0;
    g_pd_host_path[0] = g_pd_host_path[1] = 0;
    smk::PdHdr h{};
    int st = pngdec_info(file, nbytes, h);
    if (!st) {
        const int fch = p->file_channels ? p->file_channels : h.channels, fdepth = p->file_depth ? p->file_depth : h.depth;
        smk::PdArgs a;
        int rc;
        if ((rc = pngdec_setup(nullptr, 1, (int)h.H, (int)h.W, p, fch, fdepth, out, 0, row_stride_bytes, a)) != SM_OK) return rc;
        const uint64_t off = 0, size = nbytes;
        a.files = file, a.offsets = &off, a.sizes = &size;
        uint32_t path = 0;
        st = smk::pngdec_host(a, path);
        if (path == smk::PD_PATH_PARALLEL) g_pd_host_path[0] = 1;
        if (path == smk::PD_PATH_SERIAL) g_pd_host_path[1] = 1;
    }
    if (status) *status = st;
    return st ? pngdec_fail(nullptr, st, -1) : SM_OK;
}

int sm_png_decode_stats(sm_ctx* ctx, int* n_parallel, int* n_serial)
{
    if (!n_parallel || !n_serial) return fail(ctx, SM_E_ARG, "png decode: a required pointer is NULL");
    *n_parallel = *n_serial = 0;
    if (!ctx) {
        *n_parallel = g_pd_host_path[0], *n_serial = g_pd_host_path[1];
        return SM_OK;
    }
    if (ctx->pngdec.last_nimg <= 0) return SM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<smk::PdImg> v((size_t)ctx->pngdec.last_nimg);
    HIP_TRY(ctx, hipMemcpyAsync(v.data(), ctx->pngdec.img.p, v.size() * sizeof(smk::PdImg), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const smk::PdImg& im : v) {
        if (im.path == smk::PD_PATH_PARALLEL) ++*n_parallel;
        if (im.path == smk::PD_PATH_SERIAL) ++*n_serial;
    }
    return SM_OK;
}

}  // extern "C"
