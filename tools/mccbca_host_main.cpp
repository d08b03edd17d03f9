// mccbca_host_main.cpp — the CPU twin of the cross-based cost aggregation (sm_mccbca.hpp, DESIGN.md
// §4.19) under the host compiler's sanitizers: a stand-alone program that launches nothing, nothing
// preloaded.
//
//   mccbca_host SEED
//
// Runs the arms and the aggregation on a few odd shapes (one pixel, one row, one column, arms longer
// than the image, strided rows, a batch, offsets at the ends of int, several iterations) with every
// buffer an exact-size heap block, so one element out of bounds is a report.  Prints a checksum per
// case and "cases ok N"; exit 0 when all of it ran.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "sm_mccbca.hpp"

namespace {

using namespace smk;

struct Case {
    int n, H, W, pad, D, m, l1, iters;
    float tau1;
};

int run(const Case& c, std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(0.0f, 40.0f);
    const size_t row = (size_t)c.W + c.pad, img = row * (c.H - 1) + c.W + (size_t)c.pad * 3;
    const size_t gbytes = img * (c.n - 1) + row * (c.H - 1) + c.W;  // ends with the last pixel
    const size_t npix = (size_t)c.H * c.W, cells = (size_t)c.n * c.D * npix;
    std::unique_ptr<uint8_t[]> a(new uint8_t[gbytes]), b(new uint8_t[gbytes]);
    // few grey levels: arms of every length
    for (size_t k = 0; k < gbytes; k++) a[k] = (uint8_t)(100 + (rng() & 3)), b[k] = (uint8_t)(rng() & 1 ? 40 : 41);
    std::unique_ptr<uint8_t[]> arms(new uint8_t[(size_t)c.n * 4 * npix]);
    mccbca_arms_host(a.get(), c.n, img, c.H, c.W, row, c.l1, c.tau1, arms.get());
    size_t arm_sum = 0;
    for (size_t k = 0; k < (size_t)c.n * 4 * npix; k++) {
        if (arms[k] >= c.l1) return 1;
        arm_sum += arms[k];
    }
    std::unique_ptr<float[]> vol(new float[cells]), agg(new float[cells]);
    const long long m = mc_clamp_min_disparity(c.m, c.W, c.D);
    size_t live = 0;
    for (int i = 0; i < c.n; i++)
        for (int d = 0; d < c.D; d++)
            for (int y = 0; y < c.H; y++)
                for (int x = 0; x < c.W; x++) {
                    const long long xb = x - (m + d);
                    const bool in = xb >= 0 && xb < c.W;
                    live += in;
                    vol[(((size_t)i * c.D + d) * c.H + y) * c.W + x] = in ? u(rng) : mcs_nan();
                }
    mccbca_aggregate_host(vol.get(), a.get(), b.get(), c.n, img, c.H, c.W, row, c.D, c.m, c.l1, c.tau1, c.iters, agg.get());
    double sum = 0;
    size_t seen = 0;
    for (size_t k = 0; k < cells; k++)
        if (agg[k] == agg[k]) sum += agg[k], seen++;
    if (seen != live) return 1;  // an average of existing cells is a number
    std::printf("case n=%d %dx%d pad=%d D=%d m=%d l1=%d i=%d tau1=%g: arms %zu sum %.9g of %zu cells\n", c.n, c.H, c.W, c.pad, c.D,
                c.m, c.l1, c.iters, (double)c.tau1, arm_sum, sum, seen);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::mt19937 rng(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    const Case cases[] = {
        {1, 1, 1, 0, 1, 0, 5, 1, 0.05f},        {1, 1, 9, 0, 3, 0, 5, 2, 0.05f},   {1, 11, 1, 5, 2, -1, 14, 1, 0.05f},
        {1, 3, 5, 0, 4, -1, 32, 3, 3.0e38f},    {3, 5, 11, 3, 4, 2, 5, 1, 0.02f},  {2, 7, 13, 1, 20, -3, 2, 2, 0.05f},
        {1, 4, 6, 0, 5, 2147483647, 5, 1, 0.05f}, {1, 4, 6, 2, 5, -2147483647 - 1, 5, 1, 0.05f}, {1, 6, 40, 0, 9, 35, 1, 1, 0.05f},
        {1, 9, 33, 0, 256, -250, 14, 1, 0.05f},
    };
    int n = 0;
    for (const Case& c : cases) {
        if (run(c, rng)) return 1;
        n++;
    }
    std::printf("cases ok %d\n", n);
    return 0;
}
