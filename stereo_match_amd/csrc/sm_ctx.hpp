// sm_ctx.hpp — the host-side context of the C-ABI, shared by its translation units
// (sm_api.hip: the matcher core; sm_api_image.hip, sm_api_cloud.hip, sm_api_png.hip,
// sm_api_jpeg.hip, sm_api_mccnn.hip, sm_api_mcacc.hip, sm_api_mcsgm.hip, sm_api_mccbca.hip: the leaf subsystems).  Host code only: every kernel header is compiled
// in exactly one unit (sm_paths.hpp, all templates, also in sm_deep.hip's), so none is included here.  fail, ensure, get_event, stage_in,
// stage_out and check_sweep_errors are defined once, in sm_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/stereo_match_amd.h"

// internal to the library: nothing below is an exported symbol
#pragma GCC visibility push(hidden)

// a device allocation the context owns, freed with it (sm_destroy has selected and
// synchronised the device by then)
struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct TimedEvent {
    int stage, pairs;
    hipEvent_t a, b;
};

// per-group device buffers (double-buffered across launch groups)
struct BufSet {
    DevBuf census[2], cost, L, raw;
    DevBuf part, key2, pre;  // sweep engine: u16 partial sums, WTA winner records, sub-pixel inputs
    DevBuf st;               // in-sweep E/W lines (MODE 3): the strip segments' boundary states
    DevBuf vst;              // MODE 3 row bands: the vertical paths' boundary states
    hipEvent_t paths_done = nullptr, wta_done = nullptr;
    bool pending = false;  // wta_done recorded and not yet waited for by stream A
};

struct sm_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // stream A
    hipStream_t side = nullptr;    // stream B
    DevBuf img[2], planes, out, dbg, volbuf, sp_parent, sp_count, bm_pre[2], bm_cost;
    // host-pointer reprojection and point clouds: the staged map, the points, the maps' minima
    struct { DevBuf in, out, min; } rp;
    // host-pointer rectify-map / remap / gray entry points (the filters and clouds stage in src too)
    struct { DevBuf src, mapx, mapy, dst, gray; } rm;
    // fastNlMeansDenoising: the non-zero prefix of the weight table on the device, cached for the
    // (h, t, s) it was built for; its host copy lives here too, so it outlives the upload
    struct {
        DevBuf tab;
        std::vector<int32_t> tab_host;
        uint32_t key_h = 0;
        int key_t = 0, key_s = 0, ntab = 0, shift = 0;
    } nlm;
    // point clouds (sm_cloud.hpp): block totals and their scans of the extraction and the PLY
    // formatter (ply_); vertices, colours and the PLY body of the host and fused entry points
    struct { DevBuf tot, off, ply_tot, ply_off, verts, colors, out; } cloud;
    // PNG output (sm_png.hpp): the filtered streams, the segments' data and records, the chunk
    // offsets, per-image records, min / max keys; image, files and sizes of the host entry point
    struct { DevBuf stream, slots, seg, off, img, range, in, out, nb; } png;
    // PNG input (sm_pngdec.hpp): per-image records, chunk tables, the chunks' slots and records, the
    // concatenated IDAT data, the filtered streams, Adler pieces, the carried rows; the staged
    // file, its offset / size pair, the pixels and the status of the host-pointer call
    struct {
        DevBuf img, chunks, idat, cinfo, slots, zbuf, stream, seg, carry, in, tab, out, status;
        int last_nimg = 0;
    } pngdec;
    // JPEG input (sm_jpegdec.hpp): per-image records, the restart intervals, the lanes' states and
    // counts, coefficients, component planes; the staged file, descriptor, offset / size pair,
    // pixels and status of the host-pointer call
    struct {
        DevBuf img, iv, state, lane, coef, planes, in, desc, tab, out, status;
        int last_nimg = 0;
    } jpegdec;
    // MC-CNN matching cost (sm_mccnn.hpp): the packed weights and biases of the L layers, the
    // images' sums and grey-level tables (and their host copies, which outlive the transfers),
    // the two ping-pong feature maps of one image, the feature maps of the volume entry points;
    // images, features and volume of the host-pointer calls
    struct {
        DevBuf w, b, sums, tab, ping, pong, fa, fb, in_a, in_b, vol;
        std::vector<unsigned long long> sums_host;
        std::vector<float> tab_host;
        int L = 0;
    } mccnn;
    // MC-CNN accurate matching cost (sm_mcacc.hpp): the packed convolutions, their biases and the
    // packed scorer; sums, tables and ping-pong maps as above; the two projection maps of one image
    // pair and the scorer's two scratch buffers of one chunk of cells; feature maps of the volume
    // entry points; images, features and volume of the host-pointer calls; the hidden matrices in
    // bf16 (fc16), the scorer's precision (SM_MCACC_*) and the first hidden layer whose weights
    // bf16 cannot hold (0: none)
    struct {
        DevBuf w, b, fc, fc16, sums, tab, ping, pong, fa, fb, pa, pb, scr[2], in_a, in_b, vol;
        std::vector<unsigned long long> sums_host;
        std::vector<float> tab_host;
        int L = 0, F = 0, U = 0;
        int precision = 0, bf16_bad = 0;
    } mcacc;
    // MC-CNN's stereo method (sm_mcsgm.hpp): the images' sums and grey-level tables (and their host
    // copies, which outlive the transfers), the normalised images, the vertical paths, the volume
    // between two iterations, the bilateral weights (cached for sigma_bits); the stage maps a
    // caller did not ask for; volumes, images and results of the host-pointer calls
    struct {
        DevBuf sums, tab, ta, tb, l2, l3, iter, w;
        DevBuf wta_l, wta_r, status, filled, sub, med;
        DevBuf in_vol, in_vol_r, in_a, in_b, out;
        std::vector<unsigned long long> sums_host;
        std::vector<float> tab_host, w_host;
        uint32_t sigma_bits = 0;
        int R = -1;
    } mcsgm;
    // cross-based cost aggregation (sm_mccbca.hpp): the normalised images, their packed arms, the
    // volume between two iterations; image, volumes and results of the host-pointer calls
    struct {
        DevBuf ta, tb, arms_a, arms_b, iter;
        DevBuf in_vol, in_a, in_b, out;
    } mccbca;
    struct { DevBuf a; } filter;  // image_measure: the first Gaussian's result, [img][H][W] float64
    DevBuf wls_num, wls_den, wls_inter, wls_w, wls_disp[2], wls_out;  // WLS scratch
    DevBuf wls_R, wls_IT;         // WLS: Thomas pivots / elimination factors of every pass
    hipStream_t wls_stream = nullptr;  // compute_disparity: WLS weights + pivots beside the matchers
    hipStream_t lr_stream = nullptr;   // compute_disparity: the left matcher, staggered behind the right one
    hipEvent_t ev_stagger = nullptr;
    // (set by the caller for one call) recorded on the stream right after a MODE 3 down sweep;
    // sweep_done_hit tells the caller it was
    hipEvent_t sweep_done_ev = nullptr;
    bool sweep_done_hit = false;
    int tune_lr_stagger = 0;  // SM_TUNE_LR_STAGGER: 0 automatic (on), -1 off
    hipEvent_t ev_wls_fork = nullptr, ev_wls_ready = nullptr;
    DevBuf hop, sweep_err;  // sweep engine: strip-boundary granules, device error word
    DevBuf volwin;          // external cost volumes, automatic window: [pair] min/max keys + offset/scale

    void* pin = nullptr;    // page-locked host staging of the host-pointer entry points (HostStage)
    size_t pin_n = 0;
    // compute_disparity: the right matcher runs on a twin context (own streams and
    // buffers); created on first use, destroyed with this one
    sm_ctx* twin = nullptr;
    hipEvent_t ev_lr_fork = nullptr, ev_lr_join = nullptr;
    std::vector<uint32_t> cu_mask;  // sm_set_cu_mask words (applied to the twin too)
    uint32_t hop_epoch = 0;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;  // sweep engine: E/W kernel on the side stream
    hipEvent_t ev_fb_fork = nullptr, ev_fb_join = nullptr;  // sweep engine: fallback beside the LR pass
    hipEvent_t ev_ew_done = nullptr;  // banded lines: the E/W patch on the side stream (before the WTA)
    const uint32_t* fb_guard = nullptr;  // set while enqueuing a group's guarded per-direction fallback
    hipStream_t wta_override = nullptr;  // stream of the WTA launch when it is not stream_b()
    const uint32_t* wta_skip = nullptr;  // the WTA row kernel exits when this flag is set (WtaArgs::skip)
    int16_t* wta_dst = nullptr;  // integer WTA index of the current launch group (sm_compute_wta_*), or null
    BufSet set[2];
    int next_set = 0;
    // geometry of the last computation (for sm_debug_fetch): its last pair
    int lastH = 0, lastW = 0, last_width1 = 0, lastD = 0, last_ndirs = 0, last_cost = 0, last_minD = 0;
    int last_minX1 = 0, last_index = 0, last_set = 0;
    size_t last_L_pair = 0;
    uint32_t timing = 0;  // stages timed (bit = SM_STAGE_*), sm_set_timing
    int dbg_flags = 0;
    // sm_set_tuning knobs (0 = automatic)
    int tune_ew_lanes = 0, tune_sweep_ncw = 0, tune_ew_waves = 0, tune_ew_prio = 0;
    int tune_ew_warmup = 0, tune_sweep_lines = 0;  // in-sweep E/W lines: warmup columns, -1 off / 1 on
    int tune_ew_guess = 0;                         // 1: the lines start from a wrong state (tests)
    int tune_ew_start = 0;  // SM_TUNE_EW_START: 0 automatic, 1..4 the cost-derived start state, -1 the zero state
    int tune_ew_patch = 0;  // SM_TUNE_EW_PATCH: 0 automatic, 1 the E/W patch inside the up sweep, -1 its own launch
    int tune_bands = 0, tune_band_warmup = 0, tune_band_guess = 0;  // MODE 3 row bands (SM_TUNE_BANDS ...)
    int tune_cost_wgs = 0;  // k_sgbm_cost2 workgroups a launch aims for (SM_TUNE_COST_WGS; 0: SGBM_COST2_WGS)
    int tune_ply_stage = 0;  // SM_TUNE_PLY_STAGE: 0 / 1 the PLY rows staged in LDS, -1 written directly
    int tune_mcacc_chunk = 0;  // SM_TUNE_MCACC_CHUNK: 0 automatic, else the cells per pass of the scorer
    int tune_sweep_xcd = 0;  // SM_TUNE_SWEEP_XCD: 1 the XCD-aware strip placement, -1 / 0 off
    long long line_groups = 0;  // launch groups run with the in-sweep E/W lines (SM_COUNTER_LINE_GROUPS)
    long long band_groups = 0;  // of them, with row bands (SM_COUNTER_BAND_GROUPS)
    long long line_strips = 0;  // strips x pairs of those groups (SM_COUNTER_LINE_STRIPS)
    std::vector<TimedEvent> pending;
    std::vector<hipEvent_t> free_events;
    double stage_ms[SM_NUM_STAGES] = {0};
    long long stage_launches[SM_NUM_STAGES] = {0};
    long long stage_pairs[SM_NUM_STAGES] = {0};
    std::string err;
};

// records the message in the context (when given) and in the calling thread's last error
int fail(sm_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                           \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail((ctx), SM_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                          \
    } while (0)

// (re)allocate; callers make sure no queued work still uses the old buffer
int ensure(sm_ctx* ctx, DevBuf& b, size_t bytes);

hipEvent_t get_event(sm_ctx* ctx);

// sticky device-side error of the unguarded (hybrid) sweep use; clears it
int check_sweep_errors(sm_ctx* ctx);

struct StageTimer {
    sm_ctx* ctx;
    hipStream_t s;
    int stage, pairs;
    hipEvent_t a = nullptr;
    StageTimer(sm_ctx* c, hipStream_t st, int stg, int np) : ctx(c), s(st), stage(stg), pairs(np)
    {
        if (ctx->timing & (1u << stage)) {
            a = get_event(ctx);
            (void)hipEventRecord(a, s);
        }
    }
    ~StageTimer()
    {
        if (a) {
            hipEvent_t b = get_event(ctx);
            (void)hipEventRecord(b, s);
            ctx->pending.push_back({stage, pairs, a, b});
        }
    }
};

// Page-locked staging for the host-pointer entry points: inputs are packed row
// by row into pinned memory and cross PCIe as one DMA each (a pageable
// hipMemcpy2D moves one row per transfer: ~3 ms for a KITTI image); outputs
// land in pinned memory and are copied out once the stream has synchronised.
// The whole call's bytes are reserved up front, so the buffer never moves
// while a DMA of this call is queued (host entry points are synchronous, so
// nothing of a previous call is in flight either).
struct HostStage {
    struct Out {
        void* dst;
        size_t off, bytes;
    };
    sm_ctx* ctx;
    size_t used = 0;
    std::vector<Out> outs;
    explicit HostStage(sm_ctx* c) : ctx(c) {}
    int reserve(size_t bytes)
    {
        if (ctx->pin_n >= bytes && ctx->pin) return SM_OK;
        if (ctx->pin) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipHostFree(ctx->pin);
            ctx->pin = nullptr;
            ctx->pin_n = 0;
        }
        HIP_TRY(ctx, hipHostMalloc(&ctx->pin, bytes, hipHostMallocDefault));
        ctx->pin_n = bytes;
        return SM_OK;
    }
    uint8_t* take(size_t bytes)
    {
        uint8_t* p = (uint8_t*)ctx->pin + used;
        used += (bytes + 255) & ~size_t(255);
        return p;
    }
    // rows x row_bytes from host (pitch src_pitch) -> contiguous device buffer
    int in(void* dev, const void* src, size_t rows, size_t row_bytes, size_t src_pitch)
    {
        uint8_t* p = take(rows * row_bytes);
        if (src_pitch == row_bytes)
            std::memcpy(p, src, rows * row_bytes);
        else
            for (size_t r = 0; r < rows; r++) std::memcpy(p + r * row_bytes, (const uint8_t*)src + r * src_pitch, row_bytes);
        StageTimer t(ctx, ctx->stream, SM_STAGE_H2D, 1);
        HIP_TRY(ctx, hipMemcpyAsync(dev, p, rows * row_bytes, hipMemcpyHostToDevice, ctx->stream));
        return SM_OK;
    }
    int out(void* dst, const void* dev, size_t bytes)
    {
        uint8_t* p = take(bytes);
        outs.push_back({dst, (size_t)(p - (uint8_t*)ctx->pin), bytes});
        StageTimer t(ctx, ctx->stream, SM_STAGE_D2H, 1);
        HIP_TRY(ctx, hipMemcpyAsync(p, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return SM_OK;
    }
    int finish()
    {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (const Out& o : outs) std::memcpy(o.dst, (const uint8_t*)ctx->pin + o.off, o.bytes);
        return SM_OK;
    }
};
// staged bytes of n buffers of `bytes` each (256-byte slots)
inline size_t stage_bytes(size_t bytes, int n = 1) { return (size_t)n * ((bytes + 255) & ~size_t(255)); }

// The leaf subsystems' host-pointer wrappers copy straight between the caller's (pageable)
// memory and a context buffer.  One transfer: `bytes` between buf and host, or `rows` rows of
// `bytes` each with the host's rows `host_pitch` apart (the device rows are packed).
struct StageCopy {
    DevBuf& buf;
    const void* host;
    size_t bytes, rows = 0, host_pitch = 0;
};
// ensures every buffer for bytes (x rows), then copies in those with a host pointer, in order,
// as one timed SM_STAGE_H2D group; a NULL host only sizes the buffer (an output of the call)
int stage_in(sm_ctx* ctx, std::initializer_list<StageCopy> copies);
// copies out those with a host pointer, in order, as one timed SM_STAGE_D2H group, and waits
// for the stream
int stage_out(sm_ctx* ctx, std::initializer_list<StageCopy> copies);

// sm_api_mcsgm.hip: the normalised float32 images (§4.18's grey-level table; a constant image is all
// zeros) of `sets` groups of n images each into dst[s] ([n][H][W]), on the context's stream; waits
// for the images' sums.  Shared with sm_api_mccbca.hip.
int mcsgm_normalise(sm_ctx* ctx, int sets, const uint8_t* const* d_gray, int n, size_t image_stride, int H, int W,
                    size_t row_stride, DevBuf* const* dst);

// largest side of an image of the rectify, NLM and filter entry points
constexpr int kRectMaxDim = 16384;

#pragma GCC visibility pop
