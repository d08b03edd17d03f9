// mcacc_host_main.cpp — the MC-CNN accurate matching cost's CPU twin (sm_mcacc.hpp)
// under the host compiler's sanitizers: a stand-alone program that launches nothing, nothing
// preloaded.
//
//   mcacc_host SEED
//
// Runs the features and the join on a few odd shapes (one pixel, one row, one column, strided
// rows, batches; 1, 2 and 5 convolutions; 1 to 4 hidden layers of 32 to 96 units; both roles, raw
// and squashed; more planes than columns, far offsets) with every buffer an exact-size heap block,
// so one element out of bounds is a report.  Prints a checksum per case and "cases ok N"; exit 0
// when all of it ran.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "sm_mcacc.hpp"

namespace {

using namespace smk;

struct Case {
    int L, F, U, n, H, W, pad, D, m, a_is_left, raw;
};

int run(const Case& c, std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(-0.3f, 0.3f);
    std::vector<std::unique_ptr<float[]>> w, b, fw, fb;
    std::vector<const float*> wp, bp, fwp, fbp;
    for (int i = 0; i < c.L; i++) {
        const size_t nw = (size_t)AC_C * (i ? AC_C : 1) * 9;
        w.emplace_back(new float[nw]);
        b.emplace_back(new float[AC_C]);
        for (size_t k = 0; k < nw; k++) w.back()[k] = u(rng);
        for (int k = 0; k < AC_C; k++) b.back()[k] = u(rng);
        wp.push_back(w.back().get()), bp.push_back(b.back().get());
    }
    for (int i = 0; i <= c.F; i++) {
        const size_t out = i == c.F ? 1 : c.U, in = i == 0 ? 2 * AC_C : c.U;
        fw.emplace_back(new float[out * in]);
        fb.emplace_back(new float[out]);
        for (size_t k = 0; k < out * in; k++) fw.back()[k] = u(rng);
        for (size_t k = 0; k < out; k++) fb.back()[k] = u(rng);
        fwp.push_back(fw.back().get()), fbp.push_back(fb.back().get());
    }
    AcFc fc;
    fc.F = c.F, fc.U = c.U;
    std::unique_ptr<float[]> packed(new float[ac_pack_conv_floats(c.L)]), bias(new float[(size_t)c.L * AC_CP]);
    std::unique_ptr<float[]> fcp(new float[fc.floats()]);
    ac_pack_conv(c.L, wp.data(), bp.data(), packed.get(), bias.get());
    ac_pack_fc(fc, fwp.data(), fbp.data(), fcp.get());

    const size_t row = (size_t)c.W + c.pad, img = row * (c.H - 1) + c.W + (size_t)c.pad * 3;
    const size_t gbytes = img * (c.n - 1) + row * (c.H - 1) + c.W;  // ends with the last pixel
    const size_t npix = (size_t)c.H * c.W, fn = (size_t)c.n * npix * AC_C;
    std::unique_ptr<float[]> feat[2] = {std::unique_ptr<float[]>(new float[fn]), std::unique_ptr<float[]>(new float[fn])};
    for (int side = 0; side < 2; side++) {
        std::unique_ptr<uint8_t[]> gray(new uint8_t[gbytes]);
        for (size_t k = 0; k < gbytes; k++) gray[k] = (uint8_t)(rng() & 255);
        for (int i = 0; i < c.n; i++) gray[i * img] = 3, gray[i * img + (npix > 1 ? (c.W > 1 ? 1 : row) : 0)] = npix > 1 ? 200 : 3;
        const int bad = mcacc_features_host(c.L, packed.get(), bias.get(), gray.get(), c.n, img, c.H, c.W, row, feat[side].get());
        if (npix == 1 ? bad != 0 : bad != -1) {
            std::printf("case L=%d %dx%dx%d: constant-image verdict %d\n", c.L, c.n, c.H, c.W, bad);
            return 1;
        }
        if (npix == 1) return 0;  // a one-pixel image is constant: rejected before any layer runs
    }
    const size_t vn = (size_t)c.n * c.D * npix;
    std::unique_ptr<float[]> vol(new float[vn]);
    mcacc_join_host(fc, fcp.get(), feat[0].get(), feat[1].get(), c.n, c.H, c.W, c.D, c.m, c.a_is_left != 0, c.raw != 0, vol.get());
    double sum = 0;
    size_t nan = 0;
    for (size_t k = 0; k < vn; k++) {
        if (vol[k] != vol[k]) {
            nan++;
        } else {
            if (!c.raw && !(vol[k] >= -1.0f && vol[k] <= 0.0f)) {
                std::printf("case L=%d F=%d U=%d: cost %g outside [-1, 0]\n", c.L, c.F, c.U, vol[k]);
                return 1;
            }
            sum += vol[k];
        }
    }
    std::printf("case L=%d F=%d U=%d n=%d %dx%d pad=%d D=%d m=%d left=%d raw=%d: sum %.9g nan %zu of %zu\n", c.L, c.F, c.U,
                c.n, c.H, c.W, c.pad, c.D, c.m, c.a_is_left, c.raw, sum, nan, vn);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::mt19937 rng(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    const Case cases[] = {
        {1, 1, 32, 1, 1, 1, 0, 1, 0, 1, 0},
        {1, 1, 32, 1, 1, 7, 0, 3, 0, 1, 0},
        {2, 2, 32, 1, 9, 1, 5, 2, -1, 0, 0},
        {2, 3, 64, 3, 5, 11, 3, 4, 2, 1, 1},
        {5, 4, 96, 1, 4, 9, 0, 12, -3, 0, 0},
        {2, 2, 32, 2, 3, 17, 1, 256, -100, 1, 0},
        {1, 1, 64, 1, 4, 6, 0, 5, 2147483647, 1, 0},
        {1, 2, 32, 1, 4, 6, 2, 5, -2147483647 - 1, 0, 1},
    };
    int n = 0;
    for (const Case& c : cases) {
        if (run(c, rng)) return 1;
        n++;
    }
    // the sigmoid's special values
    const float inf = __builtin_inff();
    const float zs[] = {0.0f, -0.0f, inf, -inf, 80.0f, -80.0f, 1e30f, -1e30f, __builtin_nanf("")};
    for (float z : zs) {
        const float s = ac_sigmoid(z);
        std::printf("sigmoid(%g) = %.9g\n", z, s);
        if (z == z && !(s > 0.0f && s <= 1.0f)) return 1;
        if (z != z && s == s) return 1;
    }
    std::printf("cases ok %d\n", n);
    return 0;
}
