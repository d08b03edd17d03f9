// sm_deep_host.hpp — launchers of the 256 < D <= 512 instances (sm_deep.hpp's path kernel and
// the 256-thread k_wta), compiled in kDeepUnits translation units of sm_deep.hip: unit U holds
// dpl = D / 16 = 17 + 2U and 18 + 2U, for u8 (census) and u16 sums.  sm_api.hip fills the
// arguments and sizes the grids.
#pragma once
#include "sm_paths.hpp"

#pragma GCC visibility push(hidden)
namespace smk {

constexpr int kDeepUnits = 8;
// threads per k_wta workgroup of the new range: the scalar row loop keeps D / 16 sums per lane
// (no LDS row of S), and 16 column groups per row leave registers for 32 of them
constexpr int kDeepWtaThreads = 256;

// false: dpl is not one of the unit's
template <int U>
bool deep_unit_paths(int dpl, bool u8, dim3 grid, hipStream_t st, const PathsArgs& pa);
template <int U>
bool deep_unit_wta(int dpl, bool u8, dim3 grid, size_t smem, hipStream_t st, const WtaArgs& wa);

}  // namespace smk
#pragma GCC visibility pop
