// mccnn_host_main.cpp — the MC-CNN matching cost's CPU twin (sm_mccnn.hpp) under
// the host compiler's sanitizers: a stand-alone program that launches nothing, nothing preloaded.
//
//   mccnn_host SEED
//
// Runs the features and the join on a few odd shapes (one pixel, one row, one column, strided
// rows, batches; 1, 2 and 5 layers; more planes than columns, far offsets) with every buffer an
// exact-size heap block, so one element out of bounds is a report.  Prints a checksum per case
// and "cases ok N"; exit 0 when all of it ran.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "sm_mccnn.hpp"

namespace {

using namespace smk;

struct Case {
    int L, n, H, W, pad, D, m;
};

int run(const Case& c, std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(-0.3f, 0.3f);
    std::vector<std::unique_ptr<float[]>> w, b;
    std::vector<const float*> wp, bp;
    for (int i = 0; i < c.L; i++) {
        const size_t nw = (size_t)MC_C * (i ? MC_C : 1) * 9;
        w.emplace_back(new float[nw]);
        b.emplace_back(new float[MC_C]);
        for (size_t k = 0; k < nw; k++) w.back()[k] = u(rng);
        for (int k = 0; k < MC_C; k++) b.back()[k] = u(rng);
        wp.push_back(w.back().get()), bp.push_back(b.back().get());
    }
    std::unique_ptr<float[]> packed(new float[mc_pack_floats(c.L)]), bias(new float[(size_t)c.L * MC_C]);
    mc_pack_weights(c.L, wp.data(), packed.get());
    for (int i = 0; i < c.L; i++) std::memcpy(bias.get() + (size_t)i * MC_C, bp[i], MC_C * sizeof(float));

    const size_t row = (size_t)c.W + c.pad, img = row * (c.H - 1) + c.W + (size_t)c.pad * 3;
    const size_t gbytes = img * (c.n - 1) + row * (c.H - 1) + c.W;  // ends with the last pixel
    const size_t npix = (size_t)c.H * c.W, fn = (size_t)c.n * npix * MC_C;
    std::unique_ptr<float[]> feat[2] = {std::unique_ptr<float[]>(new float[fn]), std::unique_ptr<float[]>(new float[fn])};
    for (int side = 0; side < 2; side++) {
        std::unique_ptr<uint8_t[]> gray(new uint8_t[gbytes]);
        for (size_t k = 0; k < gbytes; k++) gray[k] = (uint8_t)(rng() & 255);
        for (int i = 0; i < c.n; i++) gray[i * img] = 3, gray[i * img + (npix > 1 ? (c.W > 1 ? 1 : row) : 0)] = npix > 1 ? 200 : 3;
        const int bad = mccnn_features_host(c.L, packed.get(), bias.get(), gray.get(), c.n, img, c.H, c.W, row, feat[side].get());
        if (npix == 1 ? bad != 0 : bad != -1) {
            std::printf("case L=%d %dx%dx%d: constant-image verdict %d\n", c.L, c.n, c.H, c.W, bad);
            return 1;
        }
        if (npix == 1) return 0;  // a one-pixel image is constant: rejected before any layer runs
    }
    const size_t vn = (size_t)c.n * c.D * npix;
    std::unique_ptr<float[]> vol(new float[vn]);
    mccnn_join_host(feat[0].get(), feat[1].get(), c.n, c.H, c.W, c.D, c.m, vol.get());
    double sum = 0;
    size_t nan = 0;
    for (size_t k = 0; k < vn; k++) {
        if (vol[k] != vol[k])
            nan++;
        else
            sum += vol[k];
    }
    std::printf("case L=%d n=%d %dx%d pad=%d D=%d m=%d: sum %.9g nan %zu of %zu\n", c.L, c.n, c.H, c.W, c.pad, c.D, c.m, sum, nan, vn);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::mt19937 rng(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    const Case cases[] = {
        {1, 1, 1, 1, 0, 1, 0},      {1, 1, 1, 7, 0, 3, 0},         {2, 1, 9, 1, 5, 2, -1},   {2, 3, 5, 11, 3, 4, 2},
        {5, 1, 7, 13, 0, 20, -3},   {4, 2, 3, 33, 1, 256, -100},   {1, 1, 4, 6, 0, 5, 2147483647},
        {1, 1, 4, 6, 2, 5, -2147483647 - 1},
    };
    int n = 0;
    for (const Case& c : cases) {
        if (run(c, rng)) return 1;
        n++;
    }
    std::printf("cases ok %d\n", n);
    return 0;
}
