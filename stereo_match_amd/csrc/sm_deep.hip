// sm_deep.hip — one translation unit per DEEP_UNIT (0..7): the path and WTA kernels of
// numDisparities 16 * (17 + 2 * DEEP_UNIT) and 16 * (18 + 2 * DEEP_UNIT).
#include "sm_deep.hpp"
#include "sm_deep_host.hpp"

#ifndef DEEP_UNIT
#error "compile with -DDEEP_UNIT=0..7"
#endif

namespace smk {

namespace {

template <int DPL, typename LT>
void paths_t(dim3 grid, hipStream_t st, const PathsArgs& pa)
{
    hipLaunchKernelGGL((k_deep_paths<DPL, LT>), grid, dim3(256), 0, st, pa);
}

template <int DPL, typename LT>
void wta_t(dim3 grid, size_t smem, hipStream_t st, const WtaArgs& wa)
{
    hipLaunchKernelGGL((k_wta<DPL, LT, kDeepWtaThreads>), grid, dim3(kDeepWtaThreads), smem, st, wa);
}

constexpr int kLo = 17 + 2 * DEEP_UNIT;

}  // namespace

template <>
bool deep_unit_paths<DEEP_UNIT>(int dpl, bool u8, dim3 grid, hipStream_t st, const PathsArgs& pa)
{
    if (dpl == kLo)
        u8 ? paths_t<kLo, uint8_t>(grid, st, pa) : paths_t<kLo, uint16_t>(grid, st, pa);
    else if (dpl == kLo + 1)
        u8 ? paths_t<kLo + 1, uint8_t>(grid, st, pa) : paths_t<kLo + 1, uint16_t>(grid, st, pa);
    else
        return false;
    return true;
}

template <>
bool deep_unit_wta<DEEP_UNIT>(int dpl, bool u8, dim3 grid, size_t smem, hipStream_t st, const WtaArgs& wa)
{
    if (dpl == kLo)
        u8 ? wta_t<kLo, uint8_t>(grid, smem, st, wa) : wta_t<kLo, uint16_t>(grid, smem, st, wa);
    else if (dpl == kLo + 1)
        u8 ? wta_t<kLo + 1, uint8_t>(grid, smem, st, wa) : wta_t<kLo + 1, uint16_t>(grid, smem, st, wa);
    else
        return false;
    return true;
}

}  // namespace smk
