// mcacc16_host_main.cpp — the CPU twin of the accurate MC-CNN scorer's precision "bf16"
// (sm_mcacc.hpp) under the host compiler's sanitizers: a stand-alone program that
// launches nothing, nothing preloaded.
//
//   mcacc16_host SEED
//
// Runs the bf16 join on feature maps of odd shapes (one pixel, one row, one column, batches; 1 to 4
// hidden layers of 32 to 96 units; both roles, raw and squashed; more planes than columns, offsets
// at the ends of int), the check for weights bf16 cannot hold, the device's weight packing and
// ac_bf16 on its special values, with every buffer an exact-size heap block, so one element out
// of bounds is a report.  Prints a checksum per case and "cases ok N"; exit 0 when all of it ran.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "sm_mcacc.hpp"

namespace {

using namespace smk;

struct Case {
    int F, U, n, H, W, D, m, a_is_left, raw;
};

int run(const Case& c, std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(-0.3f, 0.3f);
    std::vector<std::unique_ptr<float[]>> fw, fb;
    std::vector<const float*> fwp, fbp;
    for (int i = 0; i <= c.F; i++) {
        const size_t out = i == c.F ? 1 : c.U, in = i == 0 ? 2 * AC_C : c.U;
        fw.emplace_back(new float[out * in]);
        fb.emplace_back(new float[out]);
        for (size_t k = 0; k < out * in; k++) fw.back()[k] = u(rng);
        for (size_t k = 0; k < out; k++) fb.back()[k] = u(rng);
        fwp.push_back(fw.back().get()), fbp.push_back(fb.back().get());
    }
    if (ac_fc_bf16_bad(c.F, c.U, fwp.data())) return 1;
    AcFc fc;
    fc.F = c.F, fc.U = c.U;
    std::unique_ptr<float[]> fcp(new float[fc.floats()]);
    ac_pack_fc(fc, fwp.data(), fbp.data(), fcp.get());
    ac_round_fc(fc, fcp.get());
    for (size_t j = fc.hid(1); j < fc.last(); j++)
        if (ac_bf16_float(ac_bf16(fcp[j])) != fcp[j]) return 1;  // rounded once: a second rounding changes nothing

    // the device's packing: every hidden weight exactly once
    const size_t nq = ac_pack_fc_bf16_count(c.F, c.U);
    std::unique_ptr<uint16_t[]> wq(new uint16_t[nq ? nq : 1]);
    ac_pack_fc_bf16(c.F, c.U, fwp.data(), wq.get());
    unsigned long long s_packed = 0, s_plain = 0;
    for (size_t j = 0; j < nq; j++) s_packed += wq[j];
    for (int i = 1; i < c.F; i++)
        for (size_t j = 0; j < (size_t)c.U * c.U; j++) s_plain += ac_bf16(fw[i][j]);
    if (s_packed != s_plain) {
        std::printf("case F=%d U=%d: the packed weights are not a permutation\n", c.F, c.U);
        return 1;
    }

    const size_t npix = (size_t)c.H * c.W, fn = (size_t)c.n * npix * AC_C;
    std::unique_ptr<float[]> feat[2] = {std::unique_ptr<float[]>(new float[fn]), std::unique_ptr<float[]>(new float[fn])};
    std::uniform_real_distribution<float> f(0.0f, 2.0f);
    for (int side = 0; side < 2; side++)
        for (size_t k = 0; k < fn; k++) feat[side][k] = f(rng);
    const size_t vn = (size_t)c.n * c.D * npix;
    std::unique_ptr<float[]> vol(new float[vn]);
    mcacc_join_host(fc, fcp.get(), feat[0].get(), feat[1].get(), c.n, c.H, c.W, c.D, c.m, c.a_is_left != 0, c.raw != 0,
                    vol.get(), true);
    double sum = 0;
    size_t nan = 0;
    for (size_t k = 0; k < vn; k++) {
        if (vol[k] != vol[k]) {
            nan++;
        } else {
            if (!c.raw && !(vol[k] >= -1.0f && vol[k] <= 0.0f)) {
                std::printf("case F=%d U=%d: cost %g outside [-1, 0]\n", c.F, c.U, vol[k]);
                return 1;
            }
            sum += vol[k];
        }
    }
    std::printf("case F=%d U=%d n=%d %dx%d D=%d m=%d left=%d raw=%d: sum %.9g nan %zu of %zu\n", c.F, c.U, c.n, c.H, c.W, c.D,
                c.m, c.a_is_left, c.raw, sum, nan, vn);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::mt19937 rng(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    const Case cases[] = {
        {1, 32, 1, 1, 1, 1, 0, 1, 0},
        {2, 32, 1, 1, 7, 3, 0, 1, 0},
        {2, 32, 1, 9, 1, 2, -1, 0, 0},
        {3, 64, 3, 5, 11, 4, 2, 1, 1},
        {4, 96, 1, 4, 9, 12, -3, 0, 0},
        {2, 32, 2, 3, 17, 256, -100, 1, 0},
        {2, 64, 1, 4, 6, 5, 2147483647, 1, 0},
        {3, 32, 1, 4, 6, 5, -2147483647 - 1, 0, 1},
    };
    int n = 0;
    for (const Case& c : cases) {
        if (run(c, rng)) return 1;
        n++;
    }
    // the rounding's special values: ties to even, the carry into the exponent, the overflow,
    // subnormals, infinities, NaNs with their sign
    const struct {
        uint32_t in;
        uint16_t out;
    } rs[] = {{0x00000000u, 0x0000}, {0x80000000u, 0x8000}, {0x3F800000u, 0x3F80}, {0x3F808000u, 0x3F80},
              {0x3F818000u, 0x3F82}, {0x3F808001u, 0x3F81}, {0x3FFF8000u, 0x4000}, {0x7F7F8000u, 0x7F80},
              {0x7F7F7FFFu, 0x7F7F}, {0xFF7FFFFFu, 0xFF80}, {0x00008000u, 0x0000}, {0x00018000u, 0x0002},
              {0x007FFFFFu, 0x0080}, {0x7F800000u, 0x7F80}, {0xFF800000u, 0xFF80}, {0x7F800001u, 0x7FC0},
              {0xFFC12345u, 0xFFC1}, {0x7FFFFFFFu, 0x7FFF}};
    for (const auto& r : rs) {
        float x;
        __builtin_memcpy(&x, &r.in, 4);
        const uint16_t got = ac_bf16(x);
        std::printf("bf16(%08x) = %04x\n", r.in, got);
        if (got != r.out) return 1;
    }
    // a weight bf16 cannot hold is found, in the hidden layers only
    {
        std::unique_ptr<float[]> w0(new float[32 * 2 * AC_C]()), w1(new float[32 * 32]()), w2(new float[32]());
        const float* fw[3] = {w0.get(), w1.get(), w2.get()};
        w0[3] = __builtin_inff(), w2[31] = __builtin_nanf("");
        if (ac_fc_bf16_bad(2, 32, fw) != 0) return 1;
        w1[32 * 32 - 1] = 3.4e38f;
        if (ac_fc_bf16_bad(2, 32, fw) != 1) return 1;
    }
    std::printf("cases ok %d\n", n);
    return 0;
}
