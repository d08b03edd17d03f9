/*
 * stereo_match_amd.h — C-ABI of the MI355X stereo disparity engine.
 *
 * Drop-in boundary for the reference hot path
 *   stereo_vision/stereo_vision.py:132  compute_disparity(gray_l, gray_r, disparity_settings, method="SGBM")
 * whose arithmetic the reference reaches through
 *   stereo_vision/stereo_vision.py:153  cv2.StereoSGBM_create(minDisparity=..., ..., preFilterCap=...)
 *   stereo_vision/stereo_vision.py:178  left_matcher.compute(gray_l, gray_r)   -> int16 disparity x16
 *   stereo_vision/stereo_vision.py:179  right_matcher.compute(gray_r, gray_l)  (createRightMatcher, :171)
 * Python binds this header with ctypes (stereo_match_amd/_lib.py); see
 * INTEGRATION.md for the binding a maintainer adds on the reference side.
 *
 * Conventions: plain pointers + sizes, no torch types.  Every function
 * returns 0 on success or a negative SM_E* code; sm_last_error() gives the
 * text.  One context per device, not shared by concurrent threads.
 * Host-pointer entry points are synchronous on return; *_device entry
 * points are asynchronous on the context's stream (sm_set_stream).
 */
#ifndef STEREO_MATCH_AMD_H
#define STEREO_MATCH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  3: sm_compute takes the nullable wta_out (9 arguments; SURVEY §8b's
 * signature).  The shared object carries it in its soname (libstereo_match_amd.so.3), so a
 * binary linked against an older ABI fails to load instead of passing a stray pointer as
 * wta_out; dlopen/ctypes callers compare sm_abi_version() with the value they were written
 * against (stereo_match_amd/_lib.py does). */
#define SM_ABI_VERSION 3

#define SM_OK 0
#define SM_E_ARG (-1)         /* bad argument: mirrors OpenCV's CV_Assert failures */
#define SM_E_HIP (-2)         /* HIP runtime / launch error */
#define SM_E_UNSUPPORTED (-4) /* valid for OpenCV but not implemented / outside exact range */
#define SM_E_DATA (-5)        /* corrupt input data (a PNG file that does not decode) */

#define SM_COST_SGBM 0   /* OpenCV StereoSGBM cost: BT(Sobel-x clip) + BT(raw)>>2, blockSize^2 box */
#define SM_COST_CENSUS 1 /* north-star cost: 9x7 census + Hamming (no reference counterpart) */
#define SM_COST_VOLUME 2 /* external float32 cost volume (mc-cnn), set by sm_aggregate_cost_f32* */

#define SM_MODE_SGBM 5 /* cv2.STEREO_SGBM_MODE_SGBM: 5 paths (reference default) */
#define SM_MODE_HH 8   /* cv2.STEREO_SGBM_MODE_HH: 8 paths */

/* Field meaning follows cv2.StereoSGBM_create kwargs (reference:
 * stereo_vision/stereo_vision.py:153-163); unnormalised values are accepted
 * and normalised exactly as OpenCV does (P1<=0 -> 2, ...). */
typedef struct sm_params {
    int min_disparity;
    /* > 0, multiple of 16 (OpenCV asserts this), up to 512; cost volumes: any 1..512.  Above 256:
     * gray input, block_size <= 11 and costs in the fast domain only (BGR input and the int16
     * path stop at 256, as sm_bm_params does), on the per-direction engine;
     * everything else is SM_E_UNSUPPORTED with the reason in sm_last_error */
    int num_disparities;
    int block_size;      /* SADWindowSize; <= 0 -> 5 */
    int P1, P2;
    int disp12_max_diff;
    int uniqueness_ratio;
    int pre_filter_cap;
    int speckle_window_size; /* > 0: cv::filterSpeckles after the median (maxSpeckleSize) */
    int speckle_range;
    int cost_kind; /* SM_COST_* */
    int mode;      /* SM_MODE_SGBM | SM_MODE_HH */
} sm_params;

typedef struct sm_ctx sm_ctx;

/* Create a context bound to HIP device `device` (its own non-blocking stream). */
int sm_create(int device, sm_ctx** out);
void sm_destroy(sm_ctx* ctx);

/* Enqueue on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL means the device's default (null) stream. */
int sm_set_stream(sm_ctx* ctx, void* hip_stream);
/* Go back to the context's own non-blocking stream. */
int sm_reset_stream(sm_ctx* ctx);

/* StereoSGBM::compute(left, right) on host buffers (uint8, row stride in
 * bytes >= W).  disp_out: int16[H*W], disparity x16, invalid = (minD-1)*16.
 * Replaces stereo_vision/stereo_vision.py:178 (and :179 with the right
 * matcher's params, see sm_right_matcher_params).
 * wta_out (nullable): int16[H*W] raw integer WTA index, i.e. OpenCV's
 * bestDisp in [0, numDisparities) for pixels in [minX1, maxX1) that pass the
 * uniqueness test (and whose aggregated cost is not saturated), -1 elsewhere;
 * taken before the sub-pixel step, the disp12MaxDiff check and the median. */
int sm_compute(sm_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W, int stride,
               const sm_params* p, int16_t* disp_out, int16_t* wta_out);

/* Same on device pointers already resident in HBM; enqueued on the context
 * stream, returns before completion. */
int sm_compute_device(sm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int H, int W,
                      int stride, const sm_params* p, int16_t* d_disp_out);

/* Batch of npairs same-size pairs on device pointers: pair i reads
 * d_left + i*pair_stride_bytes (same for right) and writes
 * d_disp_out + i*H*W.  Asynchronous on the context stream.  Pairs are
 * processed in launch groups (several pairs per kernel launch) so that one
 * pair's serial horizontal paths overlap other pairs' work. */
int sm_compute_batch_device(sm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int npairs,
                            size_t pair_stride_bytes, int H, int W, int stride, const sm_params* p,
                            int16_t* d_disp_out);

/* sm_compute_batch_device plus the integer WTA index of every pair (as sm_compute's
 * wta_out) at d_wta_out + i*H*W (int16; may be NULL).  Gray images. */
int sm_compute_wta_batch_device(sm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int npairs,
                                size_t pair_stride_bytes, int H, int W, int stride, const sm_params* p,
                                int16_t* d_disp_out, int16_t* d_wta_out);

/* The same two entry points for cn-channel images (OpenCV's StereoSGBM takes
 * gray or BGR; the reference's try_try.py:56-57,81 passes cv2.imread BGR
 * images): channels = 1 or 3 interleaved bytes per pixel, stride in bytes
 * (>= W*channels), pair_stride in bytes.  BGR input and configurations whose
 * sums can reach 2^15 (blockSize > 11, large preFilterCap / P2: e.g.
 * disparity_test.py:165-177) run OpenCV's x86 int16 arithmetic exactly
 * (sm_wide.hpp); the rest take the fast kernels.  blockSize <= 55,
 * preFilterCap <= 126. */
int sm_compute_cn(sm_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W, int stride, int channels,
                  const sm_params* p, int16_t* disp_out);
int sm_compute_batch_device_cn(sm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int npairs,
                               size_t pair_stride, int H, int W, int stride, int channels, const sm_params* p,
                               int16_t* d_out);

/* SGM over an external matching-cost volume (mc-cnn; the reference memmaps
 * one as float32 (1, D, H, W) at mapTo3D_mc_cnn.py:71 and feeds its
 * disparities to the WLS filter, :81-100).  cost: float32 [D][H][W], d-major,
 * plane d = cost of left x against right x - (min_disparity + d); D must equal
 * p->num_disparities, any value in 1..512 (OpenCV's multiple-of-16 rule is
 * StereoSGBM's own; mc-cnn's -disp_max 228 volume has 228 planes: the kernels
 * run the next multiple of 16 with pad planes that never win).
 * Costs are quantised q = rint((c + offset) * scale)
 * (float32), clamped to [0, 4095], NaN -> 4095 (counted: SM_COUNTER_VOLUME_CLAMPED /
 * SM_COUNTER_VOLUME_NAN).  scale == 0 (or NaN) derives the window per pair on the device
 * from the volume itself: offset = -min, scale = 4095 / (max - min) (float32, IEEE division)
 * over the finite costs of the quantised cells (planes < D, columns [minX1, maxX1)), so no
 * finite cost is clamped; offset is then ignored (no finite cost: 0 and 1).  P1 / P2 are in
 * the quantised units.  The result is then aggregated with the
 * path recurrence / WTA / uniqueness / sub-pixel / LR / median of
 * sm_compute (p->mode paths; block_size and pre_filter_cap unused;
 * P2 <= 12288).  Output as sm_compute.  Host version is synchronous. */
int sm_aggregate_cost_f32(sm_ctx* ctx, const float* cost, int D, int H, int W, const sm_params* p, float offset,
                          float scale, int16_t* disp_out);
/* Batch on device pointers: pair i's volume at d_cost + i*pair_stride_elems
 * (elements, >= D*H*W), output d_disp_out + i*H*W.  Asynchronous. */
int sm_aggregate_cost_f32_device(sm_ctx* ctx, const float* d_cost, int npairs, size_t pair_stride_elems, int D,
                                 int H, int W, const sm_params* p, float offset, float scale, int16_t* d_disp_out);

/* ---- WLS post-filter: cv2.ximgproc.createDisparityWLSFilter(left_matcher)
 * + setLambda/setSigmaColor + filter(displ, gray_l, None, dispr)
 * (reference: stereo_vision/stereo_vision.py:172-175,182).  Fields mirror
 * DisparityWLSFilter's setters / the filter's construction parameters. */
typedef struct sm_wls_params {
    double lambda;                  /* setLambda (default 8000; settings.ini lmbda 80000) */
    double sigma_color;             /* setSigmaColor (default 1.0; settings.ini sigma 1.2) */
    int lrc_thresh;                 /* setLRCthresh (24, in 1/16 px) */
    int depth_discontinuity_radius; /* setDepthDiscontinuityRadius (ceil(0.5*blockSize) for SGBM) */
    int use_confidence;             /* 1: LR-confidence WLS (needs dispr); 0: plain FGS (Generic(false)) */
    int min_disp;                   /* fill outside the ROI: 16*(min_disp-1) */
    int left_offset, right_offset, top_offset, bottom_offset; /* valid ROI of the left map */
    int num_iter;                   /* fast global smoother iterations (3) */
    float lambda_attenuation;       /* per-iteration lambda factor (0.25) */
    float roll_off;                 /* depth-discontinuity roll-off (0.001) */
} sm_wls_params;

/* The filter createDisparityWLSFilter(matcher with params `left`) builds. */
int sm_wls_default_params(const sm_params* left, sm_wls_params* out);

/* DisparityWLSFilter::filter on host buffers: displ/dispr int16[H*W] x16
 * (dispr may be NULL when !use_confidence), guide = left gray view uint8
 * (row stride guide_stride).  out int16[H*W].  Synchronous. */
int sm_wls_filter(sm_ctx* ctx, const int16_t* displ, const int16_t* dispr, const uint8_t* guide, int guide_stride,
                  int H, int W, const sm_wls_params* p, int16_t* out);
/* Batch on device pointers (maps at +i*H*W, guides at +i*guide_pair_stride). */
int sm_wls_filter_batch_device(sm_ctx* ctx, const int16_t* d_displ, const int16_t* d_dispr, const uint8_t* d_guide,
                               int npairs, size_t guide_pair_stride, int guide_stride, int H, int W,
                               const sm_wls_params* p, int16_t* d_out);

/* compute_disparity (stereo_vision/stereo_vision.py:132-184) in one call:
 * `left` = the matcher as created from the settings (:153-163); the
 * createDisparityWLSFilter mutation (uniqueness 0, disp12MaxDiff 1e6,
 * speckle 0) is applied to it, the right matcher is derived as
 * createRightMatcher does and runs on the swapped pair, and `wls` (see
 * sm_wls_default_params, then lambda/sigma from the settings) filters.
 * Outputs displ and filtered int16[H*W] x16.  Synchronous. */
int sm_compute_disparity(sm_ctx* ctx, const uint8_t* left_img, const uint8_t* right_img, int H, int W, int stride,
                         const sm_params* left, const sm_wls_params* wls, int16_t* displ, int16_t* filtered);
/* Same over a device batch (pair i at +i*pair_stride bytes; maps at +i*H*W;
 * d_dispr receives the right matcher's maps). Asynchronous. */
int sm_compute_disparity_batch_device(sm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int npairs,
                                      size_t pair_stride, int H, int W, int stride, const sm_params* left,
                                      const sm_wls_params* wls, int16_t* d_displ, int16_t* d_dispr,
                                      int16_t* d_filtered);

/* cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) in place on an
 * int16 map (what StereoSGBM::compute applies when speckleWindowSize > 0,
 * with newVal = 16*(minD-1), maxDiff = 16*speckleRange).  Host version is
 * synchronous; the device version filters nimg maps at d_img + i*H*W. */
int sm_filter_speckles(sm_ctx* ctx, int16_t* img, int H, int W, int new_val, int max_speckle_size, int max_diff);
int sm_filter_speckles_device(sm_ctx* ctx, int16_t* d_img, int nimg, int H, int W, int new_val,
                              int max_speckle_size, int max_diff);

/* cv::reprojectImageTo3D(disparity, Q, handleMissingValues, CV_32F): the
 * reference reprojects the filtered int16 map (disparity_calculation.py:302;
 * mapTo3D_mc_cnn.py:124 with float32) — xyz out float32 [H][W][3].
 * Q: 4x4 row-major float64.  Host version synchronous; the device version
 * handles nimg maps (disp + i*H*W, xyz + i*H*W*3).  handle_missing: Z = 10000 within FLT_EPSILON
 * of the map's minimum, the one a compare-based scan finds: a NaN pixel of either sign and any
 * payload takes no part in it, and a map without a non-NaN pixel marks nothing. */
#define SM_DISP_S16 0
#define SM_DISP_F32 1
int sm_reproject_image_to_3d(sm_ctx* ctx, const void* disp, int disp_type, int H, int W, const double* Q,
                             int handle_missing, float* xyz);
int sm_reproject_image_to_3d_device(sm_ctx* ctx, const void* d_disp, int disp_type, int nimg, int H, int W,
                                    const double* Q, int handle_missing, float* d_xyz);

/* ---- Rectification front end: the reference's rectify_opencv
 * (disparity_calculation.py:131-210: cv2.initUndistortRectifyMap x2, cv2.remap(INTER_LINEAR) x2)
 * and the two cv2.cvtColor(COLOR_BGR2GRAY) calls after it (:286-287).  The arithmetic is
 * stated in DESIGN.md §4.7 (version-scoped restatements; parity with OpenCV unpinned).
 * Image sizes (source and destination) are 1..16384 per side; anything else is SM_E_ARG. */
typedef struct sm_rectify_cam {
    double K[9];    /* camera matrix, row-major: fx = K[0], fy = K[4], cx = K[2], cy = K[5]; skew ignored */
    double dist[5]; /* (k1, k2, p1, p2, k3), OpenCV order */
    double iR[9];   /* inv(P[:3,:3] @ R), row-major, computed by the caller in float64 */
} sm_rectify_cam;

/* initUndistortRectifyMap(K, dist, R, P, (W, H), CV_32FC1): mapx / mapy float32 [H][W].
 * Host version synchronous; the device version asynchronous. */
int sm_rectify_map(sm_ctx* ctx, const sm_rectify_cam* cam, int H, int W, float* mapx, float* mapy);
int sm_rectify_map_device(sm_ctx* ctx, const sm_rectify_cam* cam, int H, int W, float* d_mapx, float* d_mapy);

/* remap(src, mapx, mapy, INTER_LINEAR), constant-0 border, on a uint8 image of `channels`
 * (1 or 3) interleaved bytes per pixel, rows src_stride bytes apart (>= srcW*channels).
 * dst (nullable): [H][W][channels], row stride W*channels.  gray (nullable; channels == 3):
 * cvtColor(dst, COLOR_BGR2GRAY), [H][W], computed from the rounded uint8 BGR values.  At
 * least one output.  Synchronous. */
int sm_remap_u8(sm_ctx* ctx, const uint8_t* src, int srcH, int srcW, int src_stride, int channels,
                const float* mapx, const float* mapy, int H, int W, uint8_t* dst, uint8_t* gray);
/* Batch on device pointers: image i at d_src + i*img_stride_bytes, one map pair shared by
 * the batch, outputs at d_dst + i*H*W*channels and d_gray + i*H*W.  Asynchronous. */
int sm_remap_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t img_stride_bytes, int srcH, int srcW,
                             int src_stride, int channels, const float* d_mapx, const float* d_mapy, int H, int W,
                             uint8_t* d_dst, uint8_t* d_gray);

/* cvtColor(src, COLOR_BGR2GRAY) alone on uint8 BGR images (rows src_stride bytes apart,
 * >= 3*W): gray [H][W].  Host version synchronous; the device batch (image i at
 * d_src + i*img_stride_bytes, gray at d_gray + i*H*W) asynchronous. */
int sm_bgr2gray_u8(sm_ctx* ctx, const uint8_t* src, int H, int W, int src_stride, uint8_t* gray);
int sm_bgr2gray_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t img_stride_bytes, int H, int W,
                                int src_stride, uint8_t* d_gray);

/* ---- fastNlMeansDenoising(src, None, h, templateWindowSize, searchWindowSize) on uint8 gray
 * images: the call in front of the matcher in the reference's test flow
 * (disparity_test.py:94-95).  NORM_L2, one channel; the arithmetic is stated in DESIGN.md §4.8
 * (a version-scoped restatement; parity with OpenCV unpinned).  templateWindowSize 1..9 and
 * searchWindowSize 1..35 (an even size counts as the next odd one; larger: SM_E_UNSUPPORTED),
 * any finite h >= 0, H and W 1..16384, rows src_stride bytes apart (>= W); anything else is
 * SM_E_ARG.  The output is [H][W], densely packed.  Synchronous. */
int sm_nlm_denoise_u8(sm_ctx* ctx, const uint8_t* src, int H, int W, int src_stride, float h, int template_window,
                      int search_window, uint8_t* dst);
/* Image i at d_src + i*img_stride_bytes, output at d_dst + i*H*W; one launch for the batch.
 * Asynchronous, on the ctx stream (the first call with a new (h, template, search) builds and
 * uploads the weight table and waits for that upload). */
int sm_nlm_denoise_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t img_stride_bytes, int H, int W,
                                   int src_stride, float h, int template_window, int search_window, uint8_t* d_dst);
/* The weight table the calls above use: fills tab[0..*n), returns the fixed-point weight of
 * distance 0 (fpm) and the shift applied to a patch distance before the lookup; tab may be NULL
 * to query n.  Needs no context and no device. */
int sm_nlm_weight_table(float h, int template_window, int search_window, int32_t* tab, int* n, int* fpm, int* shift);

/* ---- float64 Gaussian filter, image_measure and pyrDown: the two host image
 * operations left in the reference's scripts: image_measure (disparity_test.py:54-66:
 * cvtColor(BGR2GRAY), scipy.ndimage.gaussian_filter sigma 5 then 3, img + 30 * (img - blurred))
 * and cv2.pyrDown (try_try.py:56-57).
 * A Gaussian axis is given by its half kernel w[0..r], centre first, host memory, computed by the
 * caller (stereo_match_amd.filters.gaussian_kernel1d states scipy's expressions).  Per axis, for
 * output index i on a line of length n:
 *   t = a[i]*w[0];  for j = r..1:  t = t + (a[refl(i-j)] + a[refl(i+j)])*w[j]
 * every operation rounded to float64, no FMA; refl is scipy's 'reflect' (half-sample symmetric,
 * any r); axis 0 (rows, wy) over the whole image first, then axis 1 (wx).  With such weights the
 * result equals scipy.ndimage.gaussian_filter(mode='reflect') bit for bit.  A NULL weight pointer
 * or r = 0 is the identity on that axis.  r 0..64 (larger: SM_E_UNSUPPORTED); H and W 1..16384;
 * anything else is SM_E_ARG.  Strides of float64 images count doubles, of uint8 images bytes. */
/* Images [nimg] at src + i*src_img_stride, rows src_stride apart (>= W); dst is [nimg][H][W],
 * densely packed.  Synchronous. */
int sm_gauss2d_f64(sm_ctx* ctx, const double* src, int nimg, size_t src_img_stride, int H, int W, int src_stride,
                   const double* wy, int ry, const double* wx, int rx, double* dst);
/* Device pointers, destination strides too; one launch for the batch.  Source and destination
 * must not overlap.  Asynchronous, on the ctx stream. */
int sm_gauss2d_f64_batch_device(sm_ctx* ctx, const double* d_src, int nimg, size_t src_img_stride, int H, int W,
                                int src_stride, const double* wy, int ry, const double* wx, int rx, double* d_dst,
                                size_t dst_img_stride, int dst_stride);
/* image_measure of a uint8 BGR image (rows src_stride bytes apart, >= 3*W):
 *   g = (1868*B + 9617*G + 4899*R + 8192) >> 14   (sm_bgr2gray_u8's bytes, exact as float64)
 *   a = gauss(g; w1, r1 on both axes);  b = gauss(a; w2, r2 on both axes)
 *   out = a + alpha*(a - b)                        (subtract, multiply, add, each rounded)
 * out is float64 [H][W], densely packed.  Synchronous. */
int sm_image_measure_u8(sm_ctx* ctx, const uint8_t* bgr, int H, int W, int src_stride, const double* w1, int r1,
                        const double* w2, int r2, double alpha, double* dst);
/* Image i at d_bgr + i*img_stride_bytes, output at d_dst + i*H*W; two launches for the batch,
 * the intermediate a in a buffer of the context.  Asynchronous, on the ctx stream. */
int sm_image_measure_u8_batch_device(sm_ctx* ctx, const uint8_t* d_bgr, int nimg, size_t img_stride_bytes, int H, int W,
                                     int src_stride, const double* w1, int r1, const double* w2, int r2, double alpha,
                                     double* d_dst);
/* cv2.pyrDown(src) with the default size and border, uint8, channels 1 or 3 (interleaved):
 *   dst[y][x][c] = (sum_{i,j=-2..2} k[i]*k[j]*src[r101(2y+i, H)][r101(2x+j, W)][c] + 128) >> 8
 * k = (1,4,6,4,1), r101 = BORDER_REFLECT_101; dst is [(H+1)/2][(W+1)/2][channels], densely
 * packed.  A restatement of OpenCV's documented behaviour; parity with OpenCV unpinned.
 * Synchronous. */
int sm_pyr_down_u8(sm_ctx* ctx, const uint8_t* src, int H, int W, int src_stride, int channels, uint8_t* dst);
/* Device pointers, strides in bytes on both sides; one launch for the batch.  Asynchronous. */
int sm_pyr_down_u8_batch_device(sm_ctx* ctx, const uint8_t* d_src, int nimg, size_t src_img_stride_bytes, int H, int W,
                                int src_stride, int channels, uint8_t* d_dst, size_t dst_img_stride_bytes,
                                int dst_stride);

/* ---- point clouds: the tail of the reference's scripts
 * (disparity_calculation.py:302-320, disparity_test.py:230-265, try_try.py:90-96,
 * mapTo3D_mc_cnn.py:124 ff.): reprojectImageTo3D, cvtColor(BGR2RGB), a disparity-range mask,
 * points[mask] / colors[mask], and the rows io_functions.write_ply writes (io_functions.py:28-44).
 *
 * Mask: lo < d < hi, strict; either bound may be absent.  SM_CLOUD_LO_MIN takes lo from the map
 * itself, one minimum per image, as numpy's `d > d.min()` (try_try.py:92): a map with a NaN
 * pixel, of either sign, has the bound NaN and an empty cloud.  A NaN
 * disparity passes no bound.  For a float32 map a bound is rounded to float32 before it is
 * compared, as numpy >= 2 does with a Python scalar; an int16 map compares as the numbers they
 * are.  A NaN bound is SM_E_ARG.  zero_nonfinite replaces every NaN or +-inf COMPONENT by 0
 * (disparity_calculation.py:316-317).  handle_missing is reprojectImageTo3D's. */
#define SM_CLOUD_LO_NONE 0
#define SM_CLOUD_LO_VALUE 1
#define SM_CLOUD_LO_MIN 2
typedef struct sm_cloud_params {
    double lo, hi;
    int lo_mode; /* SM_CLOUD_LO_* */
    int has_hi;
    int zero_nonfinite;
    int handle_missing;
} sm_cloud_params;

/* Sizes: every output buffer comes with its capacity.  Nothing is ever written past a capacity;
 * the needed size is always reported, and the caller compares.  The host forms return SM_E_ARG
 * (with the size reported, nothing copied out) when the capacity is too small; the device forms
 * are asynchronous and report the size in device memory only (rows or bytes that do not fit are
 * left out).  Capacity 0 with NULL output buffers is the size query.
 *
 * Extraction.  For nimg maps [H][W] (disp_type as sm_reproject_image_to_3d: int16 or float32,
 * densely packed) and their BGR uint8 images (image i at d_bgr + i*bgr_img_stride_bytes, rows
 * bgr_stride bytes apart, >= 3*W): the pixels that pass the mask, compacted in row-major order,
 * image i's rows after image i-1's: verts float32 [N][3], bit for bit the pixels of
 * sm_reproject_image_to_3d, and colors uint8 [N][3] as RGB.  d_counts (nullable): int64 [nimg],
 * the rows of every image.  H*W <= 2^30, nimg <= 65535. */
int sm_cloud_extract_batch_device(sm_ctx* ctx, const void* d_disp, int disp_type, const uint8_t* d_bgr,
                                  size_t bgr_img_stride_bytes, int bgr_stride, int nimg, int H, int W, const double* Q,
                                  const sm_cloud_params* p, size_t capacity_rows, float* d_verts, uint8_t* d_colors,
                                  int64_t* d_counts);
/* One map on host pointers; *count is always set.  Synchronous. */
int sm_cloud_extract(sm_ctx* ctx, const void* disp, int disp_type, const uint8_t* bgr, int bgr_stride, int H, int W,
                     const double* Q, const sm_cloud_params* p, size_t capacity_rows, float* verts, uint8_t* colors,
                     int64_t* count);

/* The PLY body: row i is '%f %f %f %d %d %d ' of (verts[i], colors[i]) and a newline, byte for
 * byte what Python's formatter (np.savetxt) gives for every float32 bit pattern; a row is at most
 * 157 bytes.  d_nbytes (nullable unless d_out is NULL): the body's size.  Asynchronous. */
int sm_ply_format_device(sm_ctx* ctx, const float* d_verts, const uint8_t* d_colors, size_t n, size_t capacity_bytes,
                         char* d_out, uint64_t* d_nbytes);
/* The same rows by the same code on the CPU.  Needs no context and no device.  SM_E_ARG with
 * *nbytes set and nothing written when capacity_bytes is too small. */
int sm_ply_format_host(const float* verts, const uint8_t* colors, size_t n, size_t capacity_bytes, char* out,
                       uint64_t* nbytes);

/* Maps to PLY bytes: extraction and formatting back to back on the ctx stream, the vertices kept
 * in the context's device buffers.  Arguments as the two calls above. */
int sm_cloud_ply_batch_device(sm_ctx* ctx, const void* d_disp, int disp_type, const uint8_t* d_bgr,
                              size_t bgr_img_stride_bytes, int bgr_stride, int nimg, int H, int W, const double* Q,
                              const sm_cloud_params* p, size_t capacity_bytes, char* d_out, int64_t* d_counts,
                              uint64_t* d_nbytes);
/* One map on host pointers to the body in host memory; *count and *nbytes are always set.
 * Synchronous. */
int sm_cloud_ply(sm_ctx* ctx, const void* disp, int disp_type, const uint8_t* bgr, int bgr_stride, int H, int W,
                 const double* Q, const sm_cloud_params* p, size_t capacity_bytes, char* out, int64_t* count,
                 uint64_t* nbytes);

/* ---- PNG output: cv2.imwrite(".png") of the reference's scripts
 * (disparity_calculation.py:247-291, rectified_img_cal.py:316-319, disparity_test.py:114-115) and
 * the KITTI disparity format, encoded on the device.
 *
 * The file: signature, IHDR, one IDAT chunk per SM_PNG_SEG bytes of the filtered stream, IEND; no
 * interlace, no ancillary chunks.  Pixels: uint8 gray (colour type 0), uint8 x 3 (colour type 2;
 * the memory order is BGR and the file's RGB as with cv2.imwrite, unless keep_channel_order),
 * uint16 gray (big-endian samples).  A disparity map (int16 x16 or float32) is converted while
 * it is read:
 *   SM_PNG_DISP_KITTI      uint16 = disparity * 256: int16 d < 0 -> 0, else min(65535, d << 4) (exact up
 *                          to d = 4095, disparity 255.9375); float32 non-finite or <= 0 -> 0, else
 *                          min(65535, rint(d * 256)) (float32, ties to even)
 *   SM_PNG_DISP_LINEAR_U8  int16 maps only: uint8 v = clamp(((d - lo) * 510 + (hi - lo)) / (2 * (hi - lo)),
 *                          0, 255) in 64-bit integers (round half up); hi == lo gives 0 everywhere;
 *                          without has_bounds lo / hi are the map's own minimum and maximum
 *                          (show_disparity's normalize(NORM_MINMAX), plot_functions.py:99-100; the
 *                          rounding is this package's contract, OpenCV's is not pinned).
 * Filter: -1 picks per row the type whose filtered bytes, taken as signed magnitudes
 * (b < 128 ? b : 256 - b), sum to the least, ties to the lowest type (libpng's heuristic);
 * 0..4 fixes the type.  Deflate: every segment on its own (runs as matches at distance 1 +
 * literals, one dynamic Huffman block, or a stored block when that is smaller); a segment that
 * is not the last is closed on a byte boundary by an empty stored block.  The first chunk
 * begins with the zlib header 78 01, the last ends with the stream's Adler-32. */
#define SM_PNG_SEG 32768
#define SM_PNG_SRC_U8 0
#define SM_PNG_SRC_U16 1
#define SM_PNG_SRC_DISP_I16 2
#define SM_PNG_SRC_DISP_F32 3
#define SM_PNG_DISP_KITTI 0
#define SM_PNG_DISP_LINEAR_U8 1
typedef struct sm_png_params {
    int src_kind;           /* SM_PNG_SRC_* */
    int channels;           /* 1, or 3 (SM_PNG_SRC_U8 only) */
    int keep_channel_order; /* 3 channels: 0 swaps BGR -> RGB, 1 writes the memory order */
    int filter;             /* -1 adaptive, 0..4 a fixed type */
    int disp_mode;          /* SM_PNG_DISP_* (disparity sources) */
    int has_bounds;         /* SM_PNG_DISP_LINEAR_U8: lo / hi given (else the map's min / max) */
    int lo, hi;             /* in the map's units (disparity x 16) */
} sm_png_params;

/* The largest file an image of this shape can make (every segment stored); 0 for a shape that
 * is not encoded.  channels / depth are the file's (1 or 3; 8 or 16). */
size_t sm_png_bound(int H, int W, int channels, int depth);
/* nimg images of one shape (image i at d_img + i*img_stride_bytes, rows row_stride_bytes apart):
 * file i at d_out + i*capacity_bytes, its size in d_nbytes[i]; a byte that does not fit the
 * capacity is left out (sm_png_bound always fits).  d_out NULL with capacity 0: sizes only.
 * SM_E_UNSUPPORTED: (W*bpp + 1)*H >= 2^31 (bpp: bytes per pixel of the file).  Rows of up to
 * 12288 bytes are staged in LDS; wider ones are converted where they are used.
 * Asynchronous. */
int sm_png_encode_batch_device(sm_ctx* ctx, const void* d_img, size_t img_stride_bytes, size_t row_stride_bytes,
                               int nimg, int H, int W, const sm_png_params* p, size_t capacity_bytes, uint8_t* d_out,
                               uint64_t* d_nbytes);
/* One image on host pointers; *nbytes is always set; SM_E_ARG with nothing copied out when the
 * capacity is too small.  Synchronous. */
int sm_png_encode(sm_ctx* ctx, const void* img, size_t row_stride_bytes, int H, int W, const sm_png_params* p,
                  size_t capacity_bytes, uint8_t* out, uint64_t* nbytes);
/* The same file by the same functions on the CPU.  Needs no context and no device (one thread, one
 * stream). */
int sm_png_encode_host(const void* img, size_t row_stride_bytes, int H, int W, const sm_png_params* p,
                       size_t capacity_bytes, uint8_t* out, uint64_t* nbytes);

/* ---- PNG input: cv2.imread(".png") of the reference's scripts
 * (disparity_test.py:79-80, mapTo3D.py:78-79, mapTo3D_mc_cnn.py:70-77) and KITTI 16-bit disparity
 * maps, decoded on the device: chunk walk, CRC-32 of every chunk up to IEND, inflate, Adler-32,
 * scanline unfilter, pixel conversion.
 *
 * Files: non-interlaced; colour type 0 at depth 8 or 16, colour type 2 at depth 8, colour type 6
 * at depth 8 (alpha dropped); (W*bpp + 1)*H < 2^31 as for output.  Ancillary chunks are skipped.
 * Interlace, palette, depths 1/2/4, 16-bit colour and gray+alpha are SM_E_UNSUPPORTED with a
 * message that names the field.
 * Inflate: the IDAT chunks are first inflated each on its own (a wave per chunk), which is exact
 * when every chunk is a run of whole deflate blocks ending on a byte boundary that never reaches
 * back before itself and makes at most SM_PNGDEC_CAP bytes (the files of sm_png_encode*, or
 * pieces closed by Z_FULL_FLUSH); an image that fails any of these checks, or has more than
 * 2*ceil(stream/SM_PNGDEC_CAP) + 4 IDAT chunks, is inflated serially (a wave per image), which is
 * exact for every zlib stream.
 * Output by out_kind and flags (cv2.imread's): SM_PNGDEC_U8 with flags 1 -> BGR uint8 [H][W][3]
 * (gray replicated, 16-bit samples >> 8; RGB order with keep_channel_order), flags 0 -> gray
 * uint8 [H][W] (a colour file through (1868*B + 9617*G + 4899*R + 8192) >> 14, sm_bgr2gray_u8's
 * formula; OpenCV's decoder-side conversion is not pinned), flags -1 -> the file's own channels
 * (8-bit files); SM_PNGDEC_U16 (flags -1, 16-bit gray files) -> uint16 [H][W];
 * SM_PNGDEC_DISP_I16 / _F32 (16-bit gray files, SM_PNG_DISP_KITTI): v != 0 ? v >> 4 : invalid_i16
 * (int16 x16) and v != 0 ? v / 256.f : invalid_f32. */
#define SM_PNGDEC_CAP 32768
#define SM_PNGDEC_U8 0
#define SM_PNGDEC_U16 1
#define SM_PNGDEC_DISP_I16 2
#define SM_PNGDEC_DISP_F32 3
typedef struct sm_pngdec_params {
    int out_kind;           /* SM_PNGDEC_* */
    int flags;              /* 1, 0, -1 as cv2.imread (SM_PNGDEC_U8; -1 for the other kinds) */
    int keep_channel_order; /* 3-channel output: 0 gives BGR, 1 the file's RGB */
    int disp_mode;          /* SM_PNG_DISP_KITTI (disparity kinds) */
    int invalid_i16;        /* SM_PNGDEC_DISP_I16: the value of a 0 sample */
    float invalid_f32;      /* SM_PNGDEC_DISP_F32: the value of a 0 sample */
    int file_channels;      /* of the files: 1, 3, or 4 (RGBA); 0: taken from the file (host-pointer calls) */
    int file_depth;         /* 8 or 16; 0 as above */
    int max_chunks;         /* batch: chunks a file may have; 0: 2*ceil(stream/SM_PNG_SEG) + 64 */
    uint64_t max_file_bytes;/* batch: bytes a file may have; 0: twice sm_png_bound of the geometry */
} sm_pngdec_params;

/* IHDR of a PNG file in host memory: *channels 1, 3 or 4 (RGBA), *depth 8 or 16.  SM_E_DATA for
 * bytes that are no PNG file, SM_E_UNSUPPORTED for a file this package does not decode.  Host
 * only, no context. */
int sm_png_info(const uint8_t* file, size_t nbytes, int* H, int* W, int* channels, int* depth);
/* nimg files of one geometry (H, W, p->file_channels, p->file_depth) in device memory, file i at
 * d_files + d_offsets[i] with d_sizes[i] bytes: image i to d_out + i*img_stride_bytes, rows
 * row_stride_bytes apart.  d_status[i]: 0, or a positive code of the first fault found in file i
 * (sm_pngdec_status_message); the pixels of such an image are undefined.  Asynchronous. */
int sm_png_decode_batch_device(sm_ctx* ctx, const uint8_t* d_files, const uint64_t* d_offsets, const uint64_t* d_sizes,
                               int nimg, int H, int W, const sm_pngdec_params* p, void* d_out, size_t img_stride_bytes,
                               size_t row_stride_bytes, int* d_status);
/* One file on host pointers (H x W pixels of the output kind at `out`).  A faulty file is
 * SM_E_DATA (not a PNG, truncated, corrupt) or SM_E_UNSUPPORTED with the message of its status;
 * *status (may be NULL) gets the code.  Synchronous. */
int sm_png_decode(sm_ctx* ctx, const uint8_t* file, size_t nbytes, const sm_pngdec_params* p, void* out,
                  size_t row_stride_bytes, int* status);
/* The same pixels, status and inflate path by the same functions on the CPU.  Needs no context
 * and no device. */
int sm_png_decode_host(const uint8_t* file, size_t nbytes, const sm_pngdec_params* p, void* out,
                       size_t row_stride_bytes, int* status);
/* How many images of the last decode call took the chunk-parallel and the serial inflate path
 * (ctx NULL: the last sm_png_decode_host of this thread).  Synchronises the stream. */
int sm_png_decode_stats(sm_ctx* ctx, int* n_parallel, int* n_serial);
/* The message of a status code of the decoder, and the SM_E_* code the host-pointer calls return
 * for it (SM_OK, SM_E_DATA or SM_E_UNSUPPORTED). */
const char* sm_pngdec_status_message(int status);
int sm_pngdec_status_code(int status);

/* ---- JPEG input: cv2.imread(".jpg") of the reference's production flow
 * (build_npz.py:229, io_functions.py:92, try_try.py:56-57), decoded on the device with
 * libjpeg-turbo's default arithmetic (islow IDCT, fancy upsampling, jdcolor's tables) restated bit
 * for bit.
 *
 * Files: baseline sequential Huffman (SOF0, or SOF1 at 8 bits), one interleaved scan, 1 component
 * or 3 that libjpeg's rule reads as YCbCr, sampling 4:4:4, 4:2:2 (luma 2x1) or 4:2:0 (luma 2x2),
 * with or without restart markers; APPn / COM are skipped and the EXIF orientation is not
 * applied.  Progressive, lossless or arithmetic coding, 12-bit precision, several scans, other
 * sampling factors, 4 components, Adobe RGB and DNL are SM_E_UNSUPPORTED with a message that names
 * the reason.  Anything else that does not decode (truncated, a code in no table, a coefficient
 * index past 63, restart markers missing or out of sequence, data left over, a wrong segment
 * length) is SM_E_DATA; libjpeg warns and returns a picture for some of these, this package
 * refuses them.
 * Output by flags (cv2.imread's): 1 -> BGR uint8 [H][W][3] (a gray file replicated; RGB order with
 * keep_channel_order), 0 -> the Y plane uint8 [H][W] (chroma is never transformed, as libjpeg
 * does for JCS_GRAYSCALE), -1 -> gray for a gray file, BGR for a colour file. */
typedef struct sm_jpegdec_params {
    int flags;               /* 1, 0, -1 as cv2.imread */
    int keep_channel_order;  /* 3-channel output: 0 gives BGR, 1 RGB */
    int file_channels;       /* of the files: 1 or 3; 0: taken from the file (host-pointer calls) */
    int subsampling;         /* of the files: 0 (gray), 444, 422 or 420; ignored when file_channels is 0 */
    uint64_t max_file_bytes; /* batch: bytes a file may have (sizes the work buffers) */
    const void* d_desc;      /* batch: nimg descriptors of sm_jpeg_parse in device memory,
                                sm_jpeg_desc_bytes() apart */
} sm_jpegdec_params;

/* Frame header of a JPEG file in host memory: *channels 1 or 3, *subsampling 0 (gray), 444, 422 or
 * 420.  SM_E_DATA for bytes that are no JPEG file, SM_E_UNSUPPORTED for a file this package does
 * not decode.  Host only, no context. */
int sm_jpeg_info(const uint8_t* file, size_t nbytes, int* H, int* W, int* channels, int* subsampling);
/* The descriptor the device decodes from (geometry, tables, the scan's byte range), parsed on the
 * host from the segments before the scan: sm_jpeg_desc_bytes() bytes at desc.  *status (may be
 * NULL) gets the decoder's status code.  Host only, no context. */
size_t sm_jpeg_desc_bytes(void);
int sm_jpeg_parse(const uint8_t* file, size_t nbytes, void* desc, int* status);
/* nimg files of one geometry (H, W, p->file_channels, p->subsampling) in device memory, file i at
 * d_files + d_offsets[i] with d_sizes[i] bytes and its descriptor at p->d_desc: image i to
 * d_out + i*img_stride_bytes, rows row_stride_bytes apart.  d_status[i]: 0, or a positive code of
 * the first fault found in file i (sm_jpegdec_status_message); the pixels of such an image are
 * undefined.  Asynchronous. */
int sm_jpeg_decode_batch_device(sm_ctx* ctx, const uint8_t* d_files, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                int nimg, int H, int W, const sm_jpegdec_params* p, void* d_out, size_t img_stride_bytes,
                                size_t row_stride_bytes, int* d_status);
/* One file on host pointers.  A faulty file is SM_E_DATA or SM_E_UNSUPPORTED with the message of
 * its status; *status (may be NULL) gets the code.  Synchronous. */
int sm_jpeg_decode(sm_ctx* ctx, const uint8_t* file, size_t nbytes, const sm_jpegdec_params* p, void* out,
                   size_t row_stride_bytes, int* status);
/* The same pixels and status from a plain serial decoder built from the same functions, on the
 * CPU: its verdict is the reference.  Needs no context and no device. */
int sm_jpeg_decode_host(const uint8_t* file, size_t nbytes, const sm_jpegdec_params* p, void* out,
                        size_t row_stride_bytes, int* status);
/* Of the last decode call: the sub-sequences (lanes) its entropy decode used, summed over the
 * images, and the largest number of synchronisation rounds an image needed (ctx NULL: the lanes
 * the last sm_jpeg_decode_host of this thread would have used, and 0).  Synchronises the stream. */
int sm_jpeg_decode_stats(sm_ctx* ctx, int* n_subsequences, int* n_sync_rounds);
const char* sm_jpegdec_status_message(int status);
int sm_jpegdec_status_code(int status);

/* ---- StereoBM (the reference's method="BM" branch,
 * stereo_vision/stereo_vision.py:164-166: cv2.StereoBM_create(numDisparities,
 * blockSize)).  Fields follow cv::StereoBM's setters. */
typedef struct sm_bm_params {
    int min_disparity;
    int num_disparities;   /* > 0, multiple of 16 */
    int block_size;        /* SADWindowSize: odd, 5..255, < min(H, W) */
    int pre_filter_type;   /* 1 = PREFILTER_XSOBEL (default); 0 = NORMALIZED_RESPONSE (SM_E_UNSUPPORTED) */
    int pre_filter_size;   /* odd 5..255 (used by NORMALIZED_RESPONSE only) */
    int pre_filter_cap;    /* 1..63 (31) */
    int texture_threshold; /* 10 */
    int uniqueness_ratio;  /* 15 */
    int speckle_window_size;
    int speckle_range;     /* in disparity x16 units, as cv::StereoBM */
    int disp12_max_diff;   /* < 0: no left-right check (default -1) */
} sm_bm_params;

/* cv2.StereoBM_create(numDisparities, blockSize) defaults. */
int sm_bm_default_params(int num_disparities, int block_size, sm_bm_params* out);
/* ximgproc::createRightMatcher(StereoBM). */
int sm_bm_right_matcher_params(const sm_bm_params* left, sm_bm_params* right_out);
/* StereoBM::compute on host buffers (synchronous) / a device batch (asynchronous;
 * pair i at +i*pair_stride_bytes, output at +i*H*W).  int16 disparity x16,
 * invalid = 16*(minDisparity-1). */
int sm_bm_compute(sm_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W, int stride,
                  const sm_bm_params* p, int16_t* disp_out);
int sm_bm_compute_batch_device(sm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int npairs,
                               size_t pair_stride_bytes, int H, int W, int stride, const sm_bm_params* p,
                               int16_t* d_disp_out);

/* Multi-device batch from ONE process (SURVEY §8b sm_compute_batch): ctxs[k]
 * (one per device) computes the contiguous shard [k*npairs/ngpu,
 * (k+1)*npairs/ngpu) of the host pairs left[i]/right[i] (uint8 H x W,
 * C-contiguous) into out + i*H*W (host).  One host thread per context;
 * synchronous.  The scaling path the benchmark uses is one process per GPU
 * (torch.distributed / RCCL); this is the single-process convenience. */
int sm_compute_batch(sm_ctx** ctxs, int ngpu, const uint8_t* const* left, const uint8_t* const* right, int npairs,
                     int H, int W, const sm_params* p, int16_t* out);

/* ximgproc::createRightMatcher(StereoSGBM) parameter derivation
 * (reference call: stereo_vision/stereo_vision.py:171). */
int sm_right_matcher_params(const sm_params* left, sm_params* right_out);

/* Wait for all work enqueued on the context stream.  The fused-sweep engine's
 * strips wait on their neighbours; when one gives up (its neighbours could not
 * be resident, e.g. other work held the CUs), the launch group is recomputed on
 * the device by the per-direction engine, so results stay exact and the call
 * succeeds (counted by sm_get_counters).  Only the opt-in hybrid engine reports
 * such a give-up as SM_E_HIP here (and synchronous entry points check it). */
int sm_synchronize(sm_ctx* ctx);

/* Counters since sm_create: launch groups the fused sweeps handed to the
 * guarded per-direction fallback.  Synchronises the context stream. */
int sm_get_counters(sm_ctx* ctx, long long* sweep_fallbacks);

/* One counter since sm_create (synchronises the context's streams):
 *   SM_COUNTER_SWEEP_FALLBACKS  launch groups the guarded per-direction fallback recomputed;
 *   SM_COUNTER_EW_REPAIRS       E/W strip segments of the in-sweep lines whose speculative
 *                               start state differed from the true one and that the patch
 *                               pass recomputed (results stay exact; a measure of the
 *                               speculation);
 *   SM_COUNTER_VOLUME_CLAMPED   external cost-volume cells (sm_aggregate_cost_f32*) whose
 *                               quantised value fell outside [0, 4095] and was clamped;
 *   SM_COUNTER_VOLUME_NAN       external cost-volume cells that were NaN (cost 4095);
 *   SM_COUNTER_LINE_GROUPS      launch groups whose horizontal paths ran inside the down
 *                               sweep (host-side count of the engine's choice);
 *   SM_COUNTER_EW_OPEN          of the EW_REPAIRS segments, those whose recomputed values had
 *                               not met the speculative ones by the strip's far end (the true
 *                               state was carried into the next strip);
 *   SM_COUNTER_BAND_REPAIRS     vertical (S / SE / SW) chains of the row-band engine (5 paths,
 *                               one or two pairs per launch group) whose speculative state
 *                               entering a band differed from the true one and that the band
 *                               patch recomputed;
 *   SM_COUNTER_BAND_OPEN        of those, chains whose repair walk had not met the speculative
 *                               trajectory by the band's last row (it continued into the next
 *                               band);
 *   SM_COUNTER_BAND_GROUPS      launch groups that ran with row bands (host-side count);
 *   SM_COUNTER_LINE_STRIPS      sweep strips x pairs of the LINE_GROUPS launch groups (host-side:
 *                               divided by the pairs, the strips per pair, whose boundary states
 *                               the patch pass reads). */
#define SM_COUNTER_SWEEP_FALLBACKS 0
#define SM_COUNTER_EW_REPAIRS 1
#define SM_COUNTER_VOLUME_CLAMPED 2
#define SM_COUNTER_VOLUME_NAN 3
#define SM_COUNTER_LINE_GROUPS 4
#define SM_COUNTER_EW_OPEN 5
#define SM_COUNTER_BAND_REPAIRS 6
#define SM_COUNTER_BAND_OPEN 7
#define SM_COUNTER_BAND_GROUPS 8
#define SM_COUNTER_LINE_STRIPS 9
int sm_get_counter(sm_ctx* ctx, int which, long long* value);

/* Restrict the context's own streams (the default stream and its internal
 * second stream) to a CU subset: mask = nwords 32-bit words, bit i = CU i
 * (hipExtStreamCreateWithCUMask); nwords = 0 restores unmasked streams.  The
 * fused sweeps size their co-resident launches from the CUs the stream can
 * reach.  Waits for queued work; resets sm_set_stream to the own stream. */
int sm_set_cu_mask(sm_ctx* ctx, const uint32_t* mask, int nwords);

/* Per-stage device timing with hipEvents on the context stream.
 * stage: 0 cost, 1 path aggregation, 2 WTA+LR, 3 median, 4 whole matcher
 * call, 5 WLS filter (confidence + smoother + final), 6 speckle filter.
 * total_ms: summed duration; launches: timed launches; pairs: pairs they covered. */
#define SM_STAGE_COST 0
#define SM_STAGE_PATHS 1
#define SM_STAGE_WTA 2
#define SM_STAGE_MEDIAN 3
#define SM_STAGE_TOTAL 4
#define SM_STAGE_WLS 5
#define SM_STAGE_SPECKLE 6
/* fused-sweep engine kernels (inside stages 1 and 2): E/W volumes, the
 * first (down) sweep writing the partial sums, the sweep fused with the WTA */
#define SM_STAGE_HORIZONTAL 7
#define SM_STAGE_SWEEP 8
#define SM_STAGE_SWEEP_WTA 9
/* host-pointer entry points: host->device copies of the images, device->host
 * copies of the maps (kept out of every other stage) */
#define SM_STAGE_H2D 10
#define SM_STAGE_D2H 11
/* guarded per-direction recomputation after the fused sweeps (near zero unless a
 * sweep strip gave up waiting for its neighbours; see sm_get_counters) */
#define SM_STAGE_FALLBACK 12
/* one whole compute_disparity call (sm_compute_disparity[_batch_device]): fork of the
 * right matcher, both matchers, join, WLS, on the caller's stream; the two matchers
 * run concurrently, so this (not the sum of their stages) is the call's device time */
#define SM_STAGE_CALL 13
#define SM_NUM_STAGES 14
/* enable: 0 off, 1 every stage, SM_TIMING_ONLY | (1 << stage) | ... only those
 * stages.  Every timed stage records two hipEvents per launch on its stream,
 * which delays the stream (KITTI census8, 8 pairs per call: every stage timed
 * costs about 12 us per pair of wall time), so a throughput measurement times
 * only the stages it reports. */
#define SM_TIMING_ONLY 0x40000000
int sm_set_timing(sm_ctx* ctx, int enable);
int sm_get_timing(sm_ctx* ctx, int stage, double* total_ms, long long* launches, long long* pairs);
int sm_reset_timing(sm_ctx* ctx);

/* Debug / parity: copy an intermediate of the LAST pair computed to host.
 * what: 0 cost volume C[H][width1][D] (uint8 census / uint16 SGBM, volume),
 *       1 path volumes L[P][H][width1][D] (uint8 census / uint16 SGBM),
 *         direction order E, W, SE, S, SW, NE, N, NW,
 *       2 pre-median disparity int16[H][W],
 *       3 census images uint64[2][H][W] (census mode).
 * Returns the byte size when host == NULL. */
long long sm_debug_fetch(sm_ctx* ctx, int what, void* host, size_t bytes);

/* Engine selection for measurements and parity debugging; every flag below gives
 * the same disparities as 0 (normal operation):
 *   4096     per-direction engine (one path volume per direction + WTA kernel), so
 *            sm_debug_fetch(1) returns every direction;
 *   16384    the fused sweeps wherever their preconditions hold (by default launch
 *            groups below 7 census / 3 other pairs run per-direction);
 *   8192     one pair per fused-sweep launch;  1 << 19 narrow sweep strips only;
 *   1 << 21  wide sweep strips wherever built;  256 the sweeps' E/W volumes from the
 *            per-direction engine's row lines;
 *   1 << 23  flag every sweep group as given up (the guarded fallback recomputes it);
 *   64       WTA + median on a second stream, overlapped with the next launch group;
 *   8, 512   16-lane vertical / 64-lane horizontal lines in the per-direction engine;
 *   1024, 2048  census Hamming costs on the fly (all / horizontal directions);
 *   1 << 22  tiled SGBM cost kernel;  bits 16-18 launch-group size cap;
 *   1 << 30  no Infinity-Cache-sized launch groups for the per-direction engine;
 *   1 << 20  sm_compute_disparity*: the right matcher beside the left one on the twin
 *            context's stream (default: before it, on the caller's stream).
 * The measured ablations (row-WTA kernel 16/32, k_sweep2 128 / 1 << 27, hybrid engine
 * 32768) and the timing switches whose results are wrong (1, 2, 4, 1 << 24..26,
 * 1 << 28, 1 << 29, 1 << 31) exist only in the ablation build (make ablation ->
 * libstereo_match_amd_ablate.so); this library returns SM_E_UNSUPPORTED for them. */
int sm_set_debug_flags(sm_ctx* ctx, int flags);

/* Launch-shape knobs for measurements (every value gives the same disparities):
 *   SM_TUNE_EW_LANES   lanes per line of the fused-sweep engine's E/W kernel:
 *                      0 automatic (32 where D % 64 == 0, 16 where D % 32 == 0), 8 / 16 /
 *                      32 / 64 the packed line kernel with that many lanes (where built
 *                      for D), -1 the per-direction engine's 16-lane row lines;
 *   SM_TUNE_SWEEP_NCW  compute waves per fused-sweep strip: 0 automatic (modelled per
 *                      launch), else 5 (latency strips), 7 (narrow) or the wide
 *                      instance's count where built; unbuilt counts fail the call.
 *   SM_TUNE_EW_WAVES   waves per workgroup of the packed E/W lines: 0 automatic, 1..4.
 *   SM_TUNE_EW_PRIO    issue priority (s_setprio 0..3) of the packed E/W lines' waves.
 *   SM_TUNE_EW_WARMUP  columns each in-sweep E/W strip segment runs before its strip
 *                      (0 automatic: 9 with the cost-derived start state on u8 costs, else
 *                      16; 54 for u16 costs in row bands; 1..4096; rounded up to the line
 *                      loop's load chunk).  Any value is exact (the patch pass repairs
 *                      segments that started wrong); large values cost line work.
 *   SM_TUNE_EW_GUESS   0 the segments start from the state SM_TUNE_EW_START selects; 1
 *                      (tests) from a deliberately wrong state, so that nearly every segment
 *                      is repaired.
 *   SM_TUNE_EW_START   start state of the in-sweep E/W strip segments: 0 automatic (u8 costs
 *                      cost-derived, u16 costs zero), 1 cost-derived (the costs of the 4
 *                      columns before the first warmup column, minus their minimum, times 8,
 *                      capped at P2; 2..4: from that many columns), -1 the zero state.  Any
 *                      value is exact; a better start leaves the patch pass fewer repairs.
 *   SM_TUNE_SWEEP_LINES the fused-sweep engine's horizontal paths: 0 automatic (inside the
 *                      down sweep wherever that instance is built), 1 the same, -1 the E/W
 *                      volume kernel (k_ew) before / beside the sweeps.
 *   SM_TUNE_BANDS      row bands of the 5-path lines engine: 0 automatic (enough bands to
 *                      occupy the CUs at one or two pairs per launch group), 1 none, 2..H that
 *                      many (speculative vertical paths patched at the band boundaries,
 *                      exact for any value).
 *   SM_TUNE_BAND_WARMUP rows each band's vertical paths run above it (0 automatic: 16 census,
 *                      24 u16 costs; 1..4096).  Any value is exact.
 *   SM_TUNE_BAND_GUESS 0 the bands start from the zero state; 1 (tests) from a deliberately
 *                      wrong state inside the domain, so that nearly every chain is repaired.
 *   SM_TUNE_COST_WGS   workgroups the SGBM cost kernel aims for per launch (0 automatic:
 *                      2048; its row bands are sized from it).
 *   SM_TUNE_SWEEP_XCD  fused sweeps: 1 place each XCD's workgroups on a run of adjacent strips
 *                      (their cost rows shared in its L2), 0 / -1 the plain grid order.
 *   SM_TUNE_LR_STAGGER sm_compute_disparity*: 0 automatic / 1 the left matcher starts on a
 *                      second stream once the right one's down sweep is done (overlapping its
 *                      patch passes and WTA); -1 the matchers strictly one after the other.
 *   SM_TUNE_PLY_STAGE  the PLY formatter's write pass: 0 automatic / 1 a block's rows staged in
 *                      LDS and streamed out in 16-byte stores, -1 every row straight to global
 *                      memory (the same bytes; DESIGN.md §4.9 has the measurement).
 *   SM_TUNE_EW_PATCH   where the E/W patch pass of the 8-path lines chain runs: 0 automatic
 *                      (inside the up + WTA sweep where that sweep runs its wide strips anyway),
 *                      1 inside the up + WTA sweep (extra waves of its workgroups patch each
 *                      row before the sweep reaches it; the instances built for it: u8 costs,
 *                      128 disparities, all pairs of a group in one launch), -1 a launch of its
 *                      own between the sweeps.  The same results and repair counters either way;
 *                      other chains (5 paths, u16 costs, row bands) always use the launch.
 *   SM_TUNE_HOP_EPOCH  (tests) v in 1..65535 sets the epoch counter whose low 16 bits tag the
 *                      fused sweeps' boundary granules to v, once: the next sweep launch uses
 *                      v + 1, and the launch after 65535 clears the granules and restarts at 1.
 *                      v must be no smaller than the counter is (tags of later epochs would
 *                      otherwise read as fresh); 0 changes nothing.
 *   SM_TUNE_MCACC_CHUNK cells (plane values) the accurate MC-CNN scorer runs per pass through its
 *                      scratch buffers: 0 automatic (up to 2^20, bounded by a
 *                      quarter of the free device memory), 1..2^22.  Any value gives the same bits.
 * Returns SM_E_ARG for an unknown key or value. */
#define SM_TUNE_EW_LANES 1
#define SM_TUNE_SWEEP_NCW 2
#define SM_TUNE_EW_WAVES 3
#define SM_TUNE_EW_PRIO 4
#define SM_TUNE_EW_WARMUP 5
#define SM_TUNE_SWEEP_LINES 6
#define SM_TUNE_EW_GUESS 7
#define SM_TUNE_BANDS 8
#define SM_TUNE_BAND_WARMUP 9
#define SM_TUNE_BAND_GUESS 10
#define SM_TUNE_COST_WGS 11
#define SM_TUNE_LR_STAGGER 12
#define SM_TUNE_SWEEP_XCD 13
#define SM_TUNE_PLY_STAGE 14
#define SM_TUNE_EW_START 15
#define SM_TUNE_EW_PATCH 16
#define SM_TUNE_HOP_EPOCH 17
#define SM_TUNE_MCACC_CHUNK 18
int sm_set_tuning(sm_ctx* ctx, int key, int value);

/* ---- MC-CNN fast matching cost: two gray images to the float32 cost volume
 * sm_aggregate_cost_f32[_device] takes.  The network: L (1..6) convolutions 3x3, stride 1, zero
 * padding 1, 64 feature maps, ReLU after every layer but the last; the 64 features of a pixel
 * scaled to unit length; plane d of the volume at (y, x) is minus the dot product of image a's
 * features at x and image b's at x - (min_disparity + d), NaN where that column is outside the
 * image.  Every value is one fixed chain of fused multiply-adds, so the device and the *_host
 * functions (plain C++, no context, no device) give the same bits.
 *
 * Weights: w[0] float32 [64][1][3][3], w[i] [64][64][3][3], b[i] [64] (the layout of torch's
 * conv2d).  Images: uint8 gray, n of them image_stride bytes apart with rows row_stride bytes
 * apart; each is normalised to zero mean and unit (unbiased) standard deviation, and a constant
 * image fails the call with SM_E_ARG.  H * W < 2^24.  Feature maps: float32 [n][H][W][64]
 * (channel last); device feature pointers (d_feat, d_feat_a, d_feat_b) must be 16-byte aligned
 * (SM_E_ARG otherwise).  Volumes: float32 [n][D][H][W], D in 1..256, any min_disparity.  Rows:
 * sm_mccnn_features_device (and sm_mccnn_features on it) takes H <= 524280, sm_mccnn_join_device
 * (and the join and volume entry points on it) H <= 65535; more rows fail with SM_E_UNSUPPORTED
 * and a message that states the limit, before anything is launched.
 * The device entry points run on the context's stream; the features wait for the images' sums (the
 * check for a constant image) and for the upload of the grey-level tables, the join does not
 * wait.  The scratch buffers belong to the context: a caller that moves it to another stream
 * between calls orders the two streams itself. */
int sm_mccnn_set_weights(sm_ctx* ctx, int L, const float* const* w, const float* const* b);
int sm_mccnn_features_device(sm_ctx* ctx, const uint8_t* d_gray, int n, size_t image_stride, int H, int W,
                             size_t row_stride, float* d_feat);
int sm_mccnn_join_device(sm_ctx* ctx, const float* d_feat_a, const float* d_feat_b, int n, int H, int W, int D,
                         int min_disparity, float* d_vol);
int sm_mccnn_volume_device(sm_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int n, size_t image_stride, int H,
                           int W, size_t row_stride, int D, int min_disparity, float* d_vol);
/* Host pointers in and out (images packed: rows W bytes, images H * W bytes apart). */
int sm_mccnn_features(sm_ctx* ctx, const uint8_t* gray, int n, int H, int W, float* feat);
int sm_mccnn_join(sm_ctx* ctx, const float* feat_a, const float* feat_b, int n, int H, int W, int D,
                  int min_disparity, float* vol);
int sm_mccnn_volume(sm_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D, int min_disparity,
                    float* vol);
/* The CPU twin of the two steps. */
int sm_mccnn_features_host(int L, const float* const* w, const float* const* b, const uint8_t* gray, int n,
                           size_t image_stride, int H, int W, size_t row_stride, float* feat);
int sm_mccnn_join_host(const float* feat_a, const float* feat_b, int n, int H, int W, int D, int min_disparity,
                       float* vol);

/* ---- MC-CNN accurate matching cost: the 112-map feature net and the fully
 * connected scorer.  Features: L (1..6) convolutions 3x3, zero padding 1, 112 feature maps, ReLU
 * after every layer, no unit-length step; float32 [n][H][W][112], channel last.  Scorer: F (1..4)
 * hidden layers of U units (a multiple of 32, 32..384) with ReLU, one linear unit, a sigmoid.
 * Plane d of the volume at (y, x) is minus the sigmoid (raw != 0: minus the logit) of the scorer
 * on image a's features at x and image b's at x - (min_disparity + d), NaN where that column is
 * outside the image; a_is_left says which of the two feeds the left half of the first layer
 * (columns 0..111 of fw[0]) -- the right view's volume is (a = right, b = left, a_is_left = 0,
 * min_disparity = -(min_disparity + D) + 1).  Every value is one fixed chain of fused
 * multiply-adds in ascending k (the first layer split into a per-pixel projection of each image
 * and one float add per cell), so the device and the *_host functions give the same bits.
 *
 * Weights: w[0] float32 [112][1][3][3], w[i] [112][112][3][3], b[i] [112]; fw[0] [U][224],
 * fw[1..F-1] [U][U], fw[F] [1][U] (nn.Linear's [out][in]), fb[i] [U], fb[F] [1].  Images,
 * alignment, D, min_disparity and streams as for the fast net above; its weights in the same
 * context are not disturbed.  Rows: sm_mcacc_features_device (and the features and volume entry
 * points on it) takes H <= 131070 (SM_E_UNSUPPORTED beyond); sm_mcacc_join_device takes every H the
 * pixel limit allows.  The scorer works through scratch buffers of the context in chunks of
 * cells (SM_TUNE_MCACC_CHUNK); their size is bounded and does not grow with H * W * D. */
int sm_mcacc_set_weights(sm_ctx* ctx, int L, const float* const* w, const float* const* b, int F, int U,
                         const float* const* fw, const float* const* fb);
int sm_mcacc_features_device(sm_ctx* ctx, const uint8_t* d_gray, int n, size_t image_stride, int H, int W,
                             size_t row_stride, float* d_feat);
int sm_mcacc_join_device(sm_ctx* ctx, const float* d_feat_a, const float* d_feat_b, int n, int H, int W, int D,
                         int min_disparity, int a_is_left, int raw, float* d_vol);
int sm_mcacc_volume_device(sm_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int n, size_t image_stride, int H,
                           int W, size_t row_stride, int D, int min_disparity, int a_is_left, int raw, float* d_vol);
/* Host pointers in and out (images packed: rows W bytes, images H * W bytes apart). */
int sm_mcacc_features(sm_ctx* ctx, const uint8_t* gray, int n, int H, int W, float* feat);
int sm_mcacc_join(sm_ctx* ctx, const float* feat_a, const float* feat_b, int n, int H, int W, int D,
                  int min_disparity, int a_is_left, int raw, float* vol);
int sm_mcacc_volume(sm_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D, int min_disparity,
                    int a_is_left, int raw, float* vol);
/* The CPU twin of the two steps, and the scorer's sigmoid on n values. */
int sm_mcacc_features_host(int L, const float* const* w, const float* const* b, const uint8_t* gray, int n,
                           size_t image_stride, int H, int W, size_t row_stride, float* feat);
int sm_mcacc_join_host(int F, int U, const float* const* fw, const float* const* fb, const float* feat_a,
                       const float* feat_b, int n, int H, int W, int D, int min_disparity, int a_is_left, int raw,
                       float* vol);
int sm_mcacc_sigmoid_host(const float* z, size_t n, float* s);

/* The scorer's precision, a state of the context; the default is SM_MCACC_F32, the
 * arithmetic above.  SM_MCACC_BF16 changes only the hidden layers 1 .. F-1: both operands of every
 * product (the previous layer's activations and the weights, rounded once at sm_mcacc_set_weights)
 * are rounded to bfloat16 -- nearest, ties to even, subnormals kept, a finite value past bf16's
 * largest becomes infinity, a NaN a quiet NaN with its sign: sm_mcacc_bf16_host -- and the sum
 * of a unit is accumulated in float32 from its float32 bias.  The features, the projections, the
 * first layer's add, the output unit (float32 on the unrounded last hidden layer), the sigmoid and
 * the NaN border do not change.  The device runs the hidden layers on the bf16 matrix instruction
 * in one fused kernel per image, with no scratch (SM_TUNE_MCACC_CHUNK is ignored); the order of its
 * sums is the instruction's, so it equals sm_mcacc_join_host_bf16 (ascending k) bit for bit only
 * where every sum is exact, and to accumulation order otherwise.  In this mode a hidden-layer
 * weight that is not finite or rounds to infinity fails sm_mcacc_set_weights (precision set first)
 * or the join (set later) with SM_E_ARG.  sm_mcacc_join[_device] and sm_mcacc_volume[_device]
 * follow the state; the fast net is not concerned.  An unknown value: SM_E_ARG. */
#define SM_MCACC_F32 0
#define SM_MCACC_BF16 1
int sm_mcacc_set_precision(sm_ctx* ctx, int precision);
int sm_mcacc_join_host_bf16(int F, int U, const float* const* fw, const float* const* fb, const float* feat_a,
                            const float* feat_b, int n, int H, int W, int D, int min_disparity, int a_is_left, int raw,
                            float* vol);
int sm_mcacc_bf16_host(const float* x, size_t n, uint16_t* out);

/* ---- MC-CNN's stereo method after the matching cost: the paper's semi-global
 * matching on the float32 volume, left-right interpolation, sub-pixel step, 5x5 median and
 * bilateral filter.  Section 4 of the paper restated; parity with mc-cnn's code is unpinned.
 * The device and the *_host functions (plain C++, no context, no device) give the same values.
 *
 * Volumes: float32 [n][D][H][W], D in 1..256, NaN where a cell does not exist: what
 * sm_mccnn_volume[_device] writes for (a, b, D, min_disparity).  a is the view's own uint8 gray
 * image and b the other one (n of them image_stride bytes apart, rows row_stride bytes apart);
 * both go through the grey-level table of 4.15, and a constant image counts as all zeros.  The
 * right view is the same call with the images swapped and min_disparity = -(min_disparity + D) + 1.
 *
 * sm_mcsgm_aggregate*: four paths (from the left, right, above, below), averaged; sgm_i repeats
 * the step on its own result.  W <= 4096.  The output may not overlap the input (SM_E_ARG).
 * pi1 and pi2 may be 0; sgm_q1, sgm_q2, sgm_v, sgm_d must be positive and finite, sgm_i 1..16.
 *
 * sm_mcsgm_disparity*: the left view's disparity map float32 [n][H][W] from the two aggregated
 * volumes (agg_r that of the right view) and the left image; an invalid pixel is
 * float(min_disparity - 1).  |min_disparity| and |min_disparity + D| <= 2^23; blur_sigma and
 * blur_t positive, ceil(3 blur_sigma) <= 48.  stages (may be NULL, and so may each member)
 * receives the maps in between, [n][H][W] each: the integer disparities of both views after
 * winner-take-all (invalid: min_disparity - 1), the status of the left pixels (0 correct,
 * 1 mismatch, 2 occluded), the interpolated map, and the maps after the sub-pixel step and the
 * median.  The device entry points run on the context's stream and wait once for the images'
 * sums; scratch belongs to the context. */
typedef struct sm_mcsgm_params {
    float pi1, pi2, sgm_q1, sgm_q2, sgm_v, sgm_d;
    int sgm_i;
    float blur_sigma, blur_t;
} sm_mcsgm_params;
typedef struct sm_mcsgm_stages {
    int32_t *wta_left, *wta_right, *status, *filled;
    float *subpixel, *median;
} sm_mcsgm_stages;
/* The paper's KITTI fast values as recalled (unverified): 4, 55.72, 3, 2.5, 1.5, 0.02, 1, 7.74, 5. */
int sm_mcsgm_default_params(sm_mcsgm_params* out);
int sm_mcsgm_aggregate_device(sm_ctx* ctx, const float* d_vol, const uint8_t* d_a, const uint8_t* d_b, int n,
                              size_t image_stride, int H, int W, size_t row_stride, int D, int min_disparity,
                              const sm_mcsgm_params* params, float* d_agg);
int sm_mcsgm_disparity_device(sm_ctx* ctx, const float* d_agg_l, const float* d_agg_r, const uint8_t* d_a, int n,
                              size_t image_stride, int H, int W, size_t row_stride, int D, int min_disparity,
                              const sm_mcsgm_params* params, float* d_disp, const sm_mcsgm_stages* d_stages);
/* Host pointers in and out (images packed: rows W bytes, images H * W bytes apart). */
int sm_mcsgm_aggregate(sm_ctx* ctx, const float* vol, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D,
                       int min_disparity, const sm_mcsgm_params* params, float* agg);
int sm_mcsgm_disparity(sm_ctx* ctx, const float* agg_l, const float* agg_r, const uint8_t* a, int n, int H, int W, int D,
                       int min_disparity, const sm_mcsgm_params* params, float* disp, const sm_mcsgm_stages* stages);
/* The CPU twin of the two steps. */
int sm_mcsgm_aggregate_host(const float* vol, const uint8_t* a, const uint8_t* b, int n, size_t image_stride, int H,
                            int W, size_t row_stride, int D, int min_disparity, const sm_mcsgm_params* params,
                            float* agg);
int sm_mcsgm_disparity_host(const float* agg_l, const float* agg_r, const uint8_t* a, int n, size_t image_stride, int H,
                            int W, size_t row_stride, int D, int min_disparity, const sm_mcsgm_params* params,
                            float* disp, const sm_mcsgm_stages* stages);

/* ---- Cross-based cost aggregation of MC-CNN's stereo method: the matching cost
 * averaged over a support region that follows the edges of both images (section 4.1 of the paper
 * restated; parity with mc-cnn's code is unpinned).  The device and the *_host functions (plain
 * C++, no context, no device) give the same values.
 *
 * Images, volumes, a / b and min_disparity are those of sm_mcsgm_aggregate*; W <= 4096.
 *
 * sm_mccbca_arms*: uint8 [n][4][H][W], the arms of every pixel to the left, right, up and down:
 * the largest k <= l1 - 1 such that every pixel up to k steps away is inside the image and differs
 * from the pixel by less than tau1 (through the grey-level table of 4.15; a constant image counts
 * as all zeros).
 *
 * sm_mccbca_aggregate*: `iterations` (1..16) steps.  One step leaves a cell whose column of b is
 * outside the image as it is; every other cell becomes the sum of the costs over its region
 * divided by the region's size, where the region's arms are the shorter of a's at x and b's at
 * x - (min_disparity + d): first along the rows, then the row sums down the columns, float32 adds
 * in ascending order.  The output may not overlap the input (SM_E_ARG).  l1 1..32, tau1 finite and
 * positive, i1 and i2 0..16 (the iterations before and after the semi-global matching; these
 * functions validate them and use `iterations`).  The device entry points run on the context's
 * stream and wait once for the images' sums; scratch belongs to the context. */
typedef struct sm_mccbca_params {
    int l1;
    float tau1;
    int i1, i2;
} sm_mccbca_params;
/* The paper's KITTI accurate values as recalled (unverified): 5, 0.13, 2, 0. */
int sm_mccbca_default_params(sm_mccbca_params* out);
int sm_mccbca_arms_device(sm_ctx* ctx, const uint8_t* d_gray, int n, size_t image_stride, int H, int W, size_t row_stride,
                          const sm_mccbca_params* params, uint8_t* d_arms);
int sm_mccbca_aggregate_device(sm_ctx* ctx, const float* d_vol, const uint8_t* d_a, const uint8_t* d_b, int n,
                               size_t image_stride, int H, int W, size_t row_stride, int D, int min_disparity,
                               const sm_mccbca_params* params, int iterations, float* d_agg);
/* Host pointers in and out (images packed: rows W bytes, images H * W bytes apart). */
int sm_mccbca_arms(sm_ctx* ctx, const uint8_t* gray, int n, int H, int W, const sm_mccbca_params* params, uint8_t* arms);
int sm_mccbca_aggregate(sm_ctx* ctx, const float* vol, const uint8_t* a, const uint8_t* b, int n, int H, int W, int D,
                        int min_disparity, const sm_mccbca_params* params, int iterations, float* agg);
/* The CPU twin of the two steps. */
int sm_mccbca_arms_host(const uint8_t* gray, int n, size_t image_stride, int H, int W, size_t row_stride,
                        const sm_mccbca_params* params, uint8_t* arms);
int sm_mccbca_aggregate_host(const float* vol, const uint8_t* a, const uint8_t* b, int n, size_t image_stride, int H,
                             int W, size_t row_stride, int D, int min_disparity, const sm_mccbca_params* params,
                             int iterations, float* agg);

/* Last error text of ctx (or of the calling thread when ctx == NULL). */
const char* sm_last_error(sm_ctx* ctx);

/* Library version string. */
const char* sm_version(void);
/* SM_ABI_VERSION the library was built with. */
int sm_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* STEREO_MATCH_AMD_H */
