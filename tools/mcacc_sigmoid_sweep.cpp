// mcacc_sigmoid_sweep.cpp — the accurate MC-CNN scorer's sigmoid (sm_mcacc.hpp ac_sigmoid) over every
// float32 of its clamp range [-80, 80]: the largest error against float64 1 / (1 + exp(-z)) in
// units of the last place of that value as a float32, where it occurs, and whether the function is
// monotone.  A one-off: DESIGN.md §4.20 records its output and tests/test_mcacc_host.py checks a
// sample against it.
//
//   c++ -O2 -std=c++17 -ffp-contract=off -D__host__= -D__device__= -I<hip include> \
//       -Istereo_match_amd/csrc -pthread -o mcacc_sigmoid_sweep tools/mcacc_sigmoid_sweep.cpp
//   mcacc_sigmoid_sweep [THREADS]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "sm_mcacc.hpp"

namespace {

float from_bits(uint32_t b)
{
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// the floats of [-80, 80] in ascending order: index 0 is -80, index top is -0, top + 1 is +0
float nth(uint64_t i, uint32_t top)
{
    return i <= top ? from_bits(0x80000000u | (uint32_t)(top - i)) : from_bits((uint32_t)(i - top - 1));
}

struct Part {
    double max_ulp = 0;
    float at = 0;
    uint64_t decreases = 0;
};

}  // namespace

int main(int argc, char** argv)
{
    const int nt = argc > 1 ? std::atoi(argv[1]) : 8;
    uint32_t top;
    const float eighty = 80.0f;
    std::memcpy(&top, &eighty, 4);
    const uint64_t total = 2 * ((uint64_t)top + 1);
    std::vector<Part> parts(nt);
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            const uint64_t lo = total * t / nt, hi = total * (t + 1) / nt;
            Part p;
            float prev = lo ? smk::ac_sigmoid(nth(lo - 1, top)) : 0.0f;
            for (uint64_t i = lo; i < hi; i++) {
                const float z = nth(i, top), s = smk::ac_sigmoid(z);
                const double ref = 1.0 / (1.0 + std::exp(-(double)z));
                const double ulp = std::ldexp(1.0, (int)std::floor(std::log2(ref)) - 23);
                const double e = std::fabs((double)s - ref) / ulp;
                if (e > p.max_ulp) p.max_ulp = e, p.at = z;
                if (s < prev) p.decreases++;
                prev = s;
            }
            parts[t] = p;
        });
    for (auto& x : th) x.join();
    Part all;
    for (const Part& p : parts) {
        if (p.max_ulp > all.max_ulp) all.max_ulp = p.max_ulp, all.at = p.at;
        all.decreases += p.decreases;
    }
    std::printf("values %llu  max error %.4f ulp at z = %.9g  decreasing steps %llu (%s)\n", (unsigned long long)total,
                all.max_ulp, all.at, (unsigned long long)all.decreases, all.decreases ? "not monotone" : "monotone");
    return 0;
}
