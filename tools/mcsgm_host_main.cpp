// mcsgm_host_main.cpp — the CPU twin of MC-CNN's stereo method (sm_mcsgm.hpp) under
// the host compiler's sanitizers: a stand-alone program that launches nothing, nothing preloaded.
//
//   mcsgm_host SEED
//
// Runs the aggregation and the disparity step on a few odd shapes (one pixel, one row, one column,
// strided rows, batches, more planes than columns, offsets far outside the image, two iterations,
// windows larger than the image) with every buffer an exact-size heap block, so one element out
// of bounds is a report.  Prints a checksum per case and "cases ok N"; exit 0 when all of it ran.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "sm_mcsgm.hpp"

namespace {

using namespace smk;

struct Case {
    int n, H, W, pad, D, m, iters;
    float sigma;
};

int run(const Case& c, std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(0.0f, 40.0f);
    const size_t row = (size_t)c.W + c.pad, img = row * (c.H - 1) + c.W + (size_t)c.pad * 3;
    const size_t gbytes = img * (c.n - 1) + row * (c.H - 1) + c.W;  // ends with the last pixel
    const size_t npix = (size_t)c.H * c.W, cells = (size_t)c.n * c.D * npix;
    std::unique_ptr<uint8_t[]> a(new uint8_t[gbytes]), b(new uint8_t[gbytes]);
    for (size_t k = 0; k < gbytes; k++) a[k] = (uint8_t)(rng() & 255), b[k] = (uint8_t)(rng() & 192);
    std::unique_ptr<float[]> vol[2], agg[2];
    const long long mr = -((long long)c.m + c.D) + 1;  // the right view's offset, kept inside int
    const int ms[2] = {c.m, (int)(mr > 2147483647LL ? 2147483647LL : mr < -2147483647LL - 1 ? -2147483647LL - 1 : mr)};
    const McsPen pen = mcs_penalties(4.0f, 55.72f, 3.0f, 2.5f, 1.5f, 0.02f);
    for (int side = 0; side < 2; side++) {
        vol[side].reset(new float[cells]);
        agg[side].reset(new float[cells]);
        const long long m = mc_clamp_min_disparity(ms[side], c.W, c.D);
        for (int i = 0; i < c.n; i++)
            for (int d = 0; d < c.D; d++)
                for (int y = 0; y < c.H; y++)
                    for (int x = 0; x < c.W; x++) {
                        const long long xb = x - (m + d);
                        vol[side][(((size_t)i * c.D + d) * c.H + y) * c.W + x] = (xb >= 0 && xb < c.W) ? u(rng) : mcs_nan();
                    }
        mcsgm_aggregate_host(vol[side].get(), side ? b.get() : a.get(), side ? a.get() : b.get(), c.n, img, c.H, c.W, row, c.D,
                             ms[side], pen, c.iters, agg[side].get());
    }
    if (c.m < -MCS_MAXOFF || c.m > MCS_MAXOFF - c.D) {  // the C-ABI refuses the disparity step here
        std::printf("case n=%d %dx%d D=%d m=%d: aggregated only\n", c.n, c.H, c.W, c.D, c.m);
        return 0;
    }
    const size_t maps = (size_t)c.n * npix;
    std::unique_ptr<int[]> wl(new int[maps]), st(new int[maps]);
    std::unique_ptr<float[]> med(new float[maps]), out(new float[maps]);
    // some maps given, some left to the function's own scratch
    mcsgm_disparity_host(agg[0].get(), agg[1].get(), a.get(), c.n, img, c.H, c.W, row, c.D, c.m, c.sigma, 0.7f,
                         McsMaps{wl.get(), nullptr, st.get(), nullptr, nullptr, med.get(), out.get()});
    double sum = 0;
    size_t invalid = 0, status[3] = {0, 0, 0};
    for (size_t k = 0; k < maps; k++) {
        if (out[k] == (float)(c.m - 1))
            invalid++;
        else
            sum += out[k];
        if (st[k] < 0 || st[k] > 2) return 1;
        status[st[k]]++;
    }
    std::printf("case n=%d %dx%d pad=%d D=%d m=%d i=%d sigma=%g: sum %.9g invalid %zu status %zu/%zu/%zu\n", c.n, c.H, c.W, c.pad,
                c.D, c.m, c.iters, (double)c.sigma, sum, invalid, status[0], status[1], status[2]);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::mt19937 rng(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    const Case cases[] = {
        {1, 1, 1, 0, 1, 0, 1, 1.0f},       {1, 1, 7, 0, 3, 0, 1, 7.74f},       {1, 9, 1, 5, 2, -1, 2, 1.0f},
        {3, 5, 11, 3, 4, 2, 1, 0.4f},      {1, 7, 13, 0, 20, -3, 2, 1.3f},     {2, 3, 33, 1, 256, -100, 1, 2.0f},
        {1, 4, 6, 0, 5, 2147483647, 1, 1.0f}, {1, 4, 6, 2, 5, -2147483647 - 1, 1, 1.0f}, {1, 6, 40, 0, 9, 35, 1, 16.0f},
    };
    int n = 0;
    for (const Case& c : cases) {
        if (run(c, rng)) return 1;
        n++;
    }
    std::printf("cases ok %d\n", n);
    return 0;
}
