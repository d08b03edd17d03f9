// sm_deep.hpp — SGM path aggregation for 256 < D <= 512.
//
// The per-direction engine of sm_paths.hpp, restated for 17..32 disparities per lane:
//  * every line is 16 lanes (D/16 disparities per lane), four lines per wave, in both families,
//    with sm_paths.hpp's line numbering (the host sizes both grids with the same arithmetic);
//  * costs always come from a volume with the layout of the path volumes, [H][W1][D] with d
//    fastest: u8 Hamming costs in census mode (k_census_cost), u16 else.  No census window in
//    registers or LDS, so a lane holds Lp, C, Ln and the prefetch ring only;
//  * addressing: a buffer descriptor covers whole image rows from a 64-bit row base (the
//    wave's four rows of a horizontal line group; the one row a vertical-family step sits on),
//    and lane offsets count from there.  They stay below 4 * W1 * D * 2 < 2^28 bytes at
//    W1 <= 32767, whatever the volume's size (2880 x 1988 at D = 512: 2.4 GB of u8, 4.8 GB
//    of u16 per direction), and the hardware range check works per row.
#pragma once
#include <type_traits>

#include "sm_paths.hpp"

namespace smk {

template <int DPL, typename LT>
using DeepRaw = typename std::conditional<sizeof(LT) == 1, RawBytes<DPL>, RawU16<DPL>>::type;

template <int DPL, typename LT>
__device__ __forceinline__ void deep_unpack(const DeepRaw<DPL, LT>& r, uint32_t (&C)[DPL])
{
    if constexpr (sizeof(LT) == 1) {
#pragma unroll
        for (int i = 0; i < DPL; i++) C[i] = r.template get<uint8_t>(i);
    } else {
        r.unpack(C);
    }
}

// loads in flight per line (the ring of sm_paths.hpp; DPL = 32 u16: 16 words per slot)
#ifndef DEEP_PF
#define DEEP_PF 4
#endif

template <typename LT>
__device__ __forceinline__ const uint8_t* deep_cost(const PathsArgs& a, int pair)
{
    const uint8_t* c = sizeof(LT) == 1 ? a.cost8 : (const uint8_t*)a.cost;
    return c + (size_t)pair * a.cost_pair * sizeof(LT);
}

// ------------------------------------------------------- horizontal family
// A wave owns rows wline .. wline + 3; step s of line kl is column x1 = s (E) or W1 - 1 - s (W).
template <int DIR, int DPL, typename LT>
__device__ __forceinline__ void deep_horz(const PathsArgs& a, int pair, int hb)
{
    constexpr int PF = DEEP_PF, SZ = (int)sizeof(LT);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane & 15, kl = lane >> 4;
    const int H = a.H, W1 = a.width1, D = a.D;
    const int wline = ((hb - DIR * a.hblocks) * 4 + wave) * 4;
    if (wline >= H) return;  // wave-uniform
    const bool line_ok = wline + kl < H;
    const uint32_t row_bytes = (uint32_t)W1 * (uint32_t)D * SZ;
    const uint64_t span = (uint64_t)min(4, H - wline) * row_bytes;  // the wave's rows
    const size_t row0 = (size_t)wline * row_bytes;
    const rsrc_t rc = make_rsrc(deep_cost<LT>(a, pair) + row0, span);
    const rsrc_t rout = make_rsrc(a.L + (size_t)pair * a.L_pair_bytes + (size_t)DIR * a.slot_bytes + row0, span);
    const uint32_t step_bytes = (uint32_t)(DIR == 0 ? D * SZ : -D * SZ);
    // this lane's slice at step 0 (lines past the last row sit past the descriptor's range)
    uint32_t off = (uint32_t)kl * row_bytes + (uint32_t)(DIR == 0 ? 0 : W1 - 1) * (uint32_t)(D * SZ) + (uint32_t)(g * DPL * SZ);
    const uint32_t P1 = (uint32_t)a.P1, P2 = (uint32_t)a.P2;

    uint32_t Lp[DPL];
#pragma unroll
    for (int i = 0; i < DPL; i++) Lp[i] = 0;
    uint32_t minLp = 0;
    DeepRaw<DPL, LT> ring[PF];
#pragma unroll
    for (int k = 0; k < PF; k++) {
        ring[k].load(rc, (line_ok && k < W1) ? off + (uint32_t)k * step_bytes : kOOB);
        asm volatile("" ::: "memory");  // issue order = slot order
    }
    for (int s0 = 0; s0 < W1; s0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const int s = s0 + k;
            uint32_t C[DPL], Ln[DPL];
            deep_unpack<DPL, LT>(ring[k], C);
            // the slot's values leave it before its refill is issued (see sm_paths.hpp)
#pragma unroll
            for (int i = 0; i < DPL; i++) asm volatile("" : "+v"(C[i])::"memory");
            ring[k].load(rc, (line_ok && s + PF < W1) ? off + (uint32_t)PF * step_bytes : kOOB);
            const uint32_t mn = sgm_step<16, DPL>(Lp, minLp, C, P1, P2, Ln);
            bstore_n<LT, DPL, PATHS_STORE_AUX>(rout, (line_ok && s < W1) ? off : kOOB, Ln);
            off += step_bytes;
#pragma unroll
            for (int i = 0; i < DPL; i++) Lp[i] = Ln[i];
            minLp = mn;
        }
    }
}

// --------------------------------------------------------- vertical family
// sm_paths.hpp's vert_family at VL = 16: a wave owns lines b0 + 8 * kl, all on one image row
// per step, so one descriptor per step (that row) serves the four lines.
template <int DPL, typename LT>
__device__ __forceinline__ void deep_vert(const PathsArgs& a, int pair, int vb)
{
    constexpr int PF = DEEP_PF, SZ = (int)sizeof(LT), LPW = 4;
    int k = 0;
#pragma unroll
    for (int i = 1; i < 6; i++)
        if (i < a.nv && vb >= a.v_blk_start[i]) k = i;
    const int dx = a.v_dx[k], dy = a.v_dy[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane & 15, kl = lane >> 4;
    const int wv = (vb - a.v_blk_start[k]) * 4 + wave;
    const int wline = (wv >> 3) * (8 * LPW) + (wv & 7);  // relative line index of kl = 0
    if (wline >= a.v_nlines[k]) return;                  // wave-uniform
    const bool line_ok = wline + 8 * kl < a.v_nlines[k];
    const int b0 = a.v_line_lo[k] + wline;  // x1 of line 0 at step 0 (unwrapped)
    const int H = a.H, W1 = a.width1, D = a.D;
    const uint32_t P1 = (uint32_t)a.P1, P2 = (uint32_t)a.P2;
    int s_lo, s_hi;  // steps where at least one of the wave's lines is inside [0, W1)
    if (dx == 0) {
        s_lo = 0;
        s_hi = H;
    } else if (dx > 0) {
        s_lo = max(0, -(b0 + 8 * (LPW - 1)));
        s_hi = min(H, W1 - b0);
    } else {
        s_lo = max(0, b0 - W1 + 1);
        s_hi = min(H, b0 + 8 * (LPW - 1) + 1);
    }
    const int nsteps = s_hi - s_lo;
    if (nsteps <= 0) return;  // wave-uniform
    const int ysgn = dy > 0 ? 1 : -1;
    const int y_lo = dy > 0 ? s_lo : H - 1 - s_lo;
    const uint32_t row_bytes = (uint32_t)W1 * (uint32_t)D * SZ;
    const ptrdiff_t row_step = (ptrdiff_t)ysgn * (ptrdiff_t)row_bytes;
    // rows of the step being computed (orow) and of the step PF ahead whose cost is loaded (crow)
    uint8_t* orow = a.L + (size_t)pair * a.L_pair_bytes + (size_t)a.v_slot[k] * a.slot_bytes + (size_t)y_lo * row_bytes;
    const uint8_t* crow = deep_cost<LT>(a, pair) + (size_t)y_lo * row_bytes;
    int x1 = b0 + 8 * kl + dx * s_lo;
    const uint32_t lane_bytes = (uint32_t)(g * DPL * SZ);
    auto col_off = [&](int x, bool ok) {
        return (ok && x >= 0 && x < W1) ? (uint32_t)x * (uint32_t)(D * SZ) + lane_bytes : kOOB;
    };
    // a line enters the domain one step after x1 == enter_x; its state must be 0 then
    const int enter_x = dx > 0 ? -1 : W1;

    uint32_t Lp[DPL];
#pragma unroll
    for (int i = 0; i < DPL; i++) Lp[i] = 0;
    uint32_t minLp = 0;
    DeepRaw<DPL, LT> ring[PF];
#pragma unroll
    for (int j = 0; j < PF; j++) {
        // (rows past the last step are never addressed: their offset is out of range)
        ring[j].load(make_rsrc(crow, row_bytes), col_off(x1 + j * dx, line_ok && j < nsteps));
        crow += row_step;
        asm volatile("" ::: "memory");  // issue order = slot order
    }
    for (int s0 = 0; s0 < nsteps; s0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            const int s = s0 + j;
            uint32_t C[DPL], Ln[DPL];
            deep_unpack<DPL, LT>(ring[j], C);
#pragma unroll
            for (int i = 0; i < DPL; i++) asm volatile("" : "+v"(C[i])::"memory");
            ring[j].load(make_rsrc(crow, row_bytes), col_off(x1 + PF * dx, line_ok && s + PF < nsteps));
            crow += row_step;
            const uint32_t mn = sgm_step<16, DPL>(Lp, minLp, C, P1, P2, Ln);
            bstore_n<LT, DPL, PATHS_STORE_AUX>(make_rsrc(orow, row_bytes), col_off(x1, line_ok && s < nsteps), Ln);
            orow += row_step;
#pragma unroll
            for (int i = 0; i < DPL; i++) Lp[i] = Ln[i];
            minLp = mn;
            if (dx != 0) {
                const bool ent = x1 == enter_x;
                if (__builtin_amdgcn_ballot_w64(ent)) {  // wave-uniform, at most 4 times per wave
#pragma unroll
                    for (int i = 0; i < DPL; i++) Lp[i] = ent ? 0u : Lp[i];
                    minLp = ent ? 0u : minLp;
                }
            }
            x1 += dx;
        }
    }
}

// grid (2 * hblocks + vertical blocks, pairs), 256 threads; LT: u8 (census) or u16 costs and sums
template <int DPL, typename LT>
__global__ void __launch_bounds__(256) k_deep_paths(PathsArgs a)
{
    const int b = blockIdx.x, pair = blockIdx.y;
    if (b < a.hblocks)
        deep_horz<0, DPL, LT>(a, pair, b);
    else if (b < 2 * a.hblocks)
        deep_horz<1, DPL, LT>(a, pair, b);
    else
        deep_vert<DPL, LT>(a, pair, b - 2 * a.hblocks);
}

}  // namespace smk
