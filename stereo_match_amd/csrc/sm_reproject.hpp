// sm_reproject.hpp — cv::reprojectImageTo3D on the GPU (the
// reference reprojects the filtered int16 map at disparity_calculation.py:302,
// and float32 disparity/16 in stereo_vision.py:203-209 project_points_3D).
// Semantics: oracle/reproject_np.py.  Per pixel, in float64 with FP
// contraction off:
//   qx = Q01*y + Q03 + Q00*x   (likewise qy, qz, qw with rows 1..3)
//   iW = 1/(qw + Q32*d);  X = (qx + Q02*d)*iW;  Y = (qy + Q12*d)*iW;
//   Z = (qz + Q22*d)*iW, or 10000 when handleMissingValues and d is the map's
//   minimum; stored as float32 xyz.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smk {

struct ReprojArgs {
    const void* disp;  // [img][H][W] int16 or float32
    float* xyz;        // [img][H][W][3]
    double Q[16];
    int H, W, handle_missing;
    const float* min_disp;  // [img] (handle_missing)
};

__device__ inline float disp_value(const int16_t* p, size_t i) { return (float)p[i]; }
__device__ inline float disp_value(const float* p, size_t i) { return p[i]; }

// one pixel: the arithmetic above.  Shared by k_reproject and the point-cloud extraction
// (sm_cloud.hpp), so that a compacted vertex is the full image's pixel bit for bit.
__device__ inline void reproject_point(const double* Q, int x, int y, double d, int handle_missing, double md,
                                       float* o)
{
#pragma clang fp contract(off)
    const double qx = Q[1] * y + Q[3] + Q[0] * x;
    const double qy = Q[5] * y + Q[7] + Q[4] * x;
    const double qz = Q[9] * y + Q[11] + Q[8] * x;
    const double qw = Q[13] * y + Q[15] + Q[12] * x;
    const double iW = 1.0 / (qw + Q[14] * d);
    const double X = (qx + Q[2] * d) * iW;
    const double Y = (qy + Q[6] * d) * iW;
    double Z = (qz + Q[10] * d) * iW;
    if (handle_missing && fabs(d - md) <= 1.1920928955078125e-07) Z = 10000.0;  // FLT_EPSILON, bigZ
    o[0] = (float)X;
    o[1] = (float)Y;
    o[2] = (float)Z;
}

template <typename T>
__global__ void __launch_bounds__(256) k_reproject(ReprojArgs a)
{
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, img = blockIdx.z;
    if (x >= a.W) return;
    const size_t npx = (size_t)a.H * a.W;
    const size_t i = img * npx + (size_t)y * a.W + x;
    const double d = (double)disp_value(reinterpret_cast<const T*>(a.disp), i);
    const double md = a.handle_missing ? (double)a.min_disp[img] : 0.0;
    reproject_point(a.Q, x, y, d, a.handle_missing, md, a.xyz + 3 * i);
}

// per-image minimum (handleMissingValues, the cloud's lo = "min"): order-preserving int key of a
// float.  The minimum is the one a compare-based scan finds (`if (v < min) min = v`): a NaN of
// either sign and any payload takes no part in it.  Every NaN gets KEY_NONE, the key the
// reduction starts from and above +inf's (0x7F800000), so no other value has it: a map without a
// non-NaN pixel keeps KEY_NONE, which key_float turns into a NaN, and `|d - NaN| <= eps` marks
// no pixel.  -0 sorts below +0; as a minimum the two are the same number.
constexpr int KEY_NONE = 0x7FFFFFFF;

__device__ inline int float_key(float f)
{
    const int b = __float_as_int(f);
    if ((b & 0x7FFFFFFF) > 0x7F800000) return KEY_NONE;
    return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
__device__ inline float key_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

// keys: [2][nimg], both rows initialised to KEY_NONE.  Row 0: the minimum's key.  Row 1: 0 once
// any pixel of the image is a NaN (numpy's `d.min()` is then NaN), found in the same pass.
template <typename T>
__global__ void __launch_bounds__(256) k_disp_min(const T* disp, int* keys, size_t npx)
{
    const int img = blockIdx.y, nimg = gridDim.y;
    int m = KEY_NONE;
    bool nan = false;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const int k = float_key(disp_value(disp, img * npx + i));
        nan |= k == KEY_NONE;
        m = min(m, k);
    }
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
    const bool wave_nan = __any(nan);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(keys + img, m);
        if (wave_nan) atomicMin(keys + nimg + img, 0);
    }
}

// out: [2][n].  Row 0: the minimum of the non-NaN pixels (handleMissingValues).  Row 1: numpy's
// `d.min()`, NaN when the image holds a NaN (the cloud's lo = "min": `d > NaN` passes nothing).
__global__ void k_keys_to_float(const int* keys, float* out, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    out[i] = key_float(keys[i]);
    out[n + i] = key_float(keys[n + i] == 0 ? KEY_NONE : keys[i]);
}

}  // namespace smk
