// What the one-wave-per-sample solvers share (walksat.hip, dpll.hip): the ordering of a wave's own LDS traffic,
// the literal code's variable, and the staging of a sample's instance row into LDS.
#pragma once

#include "common.h"

namespace msat {

// LDS written by one lane and read by another lane of the same wave: the LDS serves a wave's operations in
// issue order, so only the compiler has to be kept from moving them.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int lane_rank(uint64_t b) {  // set bits of b below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

__device__ __forceinline__ int var_of(uint32_t code) { return code < MSAT_LIT_ABSENT ? (int)(code >> 1) : -1; }

// Row clamp(problem_idx[s], 0, N-1) of the packed pool (N,C,4) into LDS, 8 bytes per clause.  The caller orders
// it against its readers (wave_lds_sync).  lits_extent: debug builds, elements to the end of the allocation.
__device__ __forceinline__ void wave_stage_row(const uint16_t *lits, const int32_t *problem_idx, int N, int C, int s,
                                               int lane, uint2 *row, long long lits_extent) {
    const int p = min(max(problem_idx[s], 0), N - 1);
    const uint2 *src = reinterpret_cast<const uint2 *>(lits + (size_t)p * C * MSAT_LIT_SLOTS);
    for (int c = lane; c < C; c += 64) {
        MSAT_DCHECK(((size_t)p * C + c) * MSAT_LIT_SLOTS + 3, lits_extent);
        row[c] = src[c];
    }
}

}  // namespace msat
