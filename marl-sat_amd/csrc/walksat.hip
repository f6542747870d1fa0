// Batched WalkSAT/SKC over the packed problem pool (msat_walksat, include/marlsat.h): the stochastic local
// search that produces the expert solutions of behavioural cloning for any CNF directory (the reference runs
// pysat's Glucose3, src/utils/sat_solver.py) and the classical baseline beside the learned policy.
//
// One wave per sample (a workgroup of 64 lanes), no workgroup barrier anywhere: the chain of dependent flips
// is latency-bound, so a CU is kept busy by many independent samples, not by many lanes per sample.  Every
// decision is a function of the assignment and of the Philox stream alone (never of lane order), so a host
// replay of include/marlsat.h's algorithm reproduces the outputs bit for bit.
//
// Register forms (NPL = 2 / 4 / 8 / 16 clauses per lane): clause c lives on lane c % 64, slot c / 64, so the
// ballots of slots 0, 1, ... are already in ascending clause order.  Per clause the lane keeps the three
// variable indices (-1 for a null or absent slot), a 3-bit mask of its true slots and its *critical variable*:
// the variable whose single flip would break the clause (true slots non-empty and equal to the slots on that
// variable), -1 if there is none.  A flip of the wave-uniform v updates the masks by comparing indices with v
// (no assignment lookup) and recomputes the critical variable of the clauses that hold v.  Then
//   - the unsatisfied count is one ballot + popcount per slot,
//   - the picked clause is a prefix over the slot popcounts and a k-th-set-bit select (mbcnt),
//   - break_j is, per slot, one compare of the critical variable with v_j whose result IS the ballot: the
//     counts are summed on the scalar unit, with no cross-lane reduction at all.
// The picked clause's codes are read from an LDS copy of the instance row (8 bytes, broadcast), never by
// indexing the register arrays with a runtime slot (that would put them in scratch).  The assignment bytes
// live in LDS, written by lane 0 once per flip and read back only at the end.
//
// Generic form: the same steps over an LDS-resident row, 64 clauses per pass; the true-slot mask of a clause is
// kept in the row's fourth (always absent) literal slot, the critical variable is recomputed where needed.
//
// Occurrence-list form (form 6, further down): the incremental WalkSAT, whose flip costs the clauses of one
// variable instead of a pass over all of them.
//
// LDS per sample: 8 * C + V bytes (V rounded up to 16), at most 64 KiB; larger shapes are refused.  The
// occurrence-list form needs 14 * C + 9 * V bytes (plus rounding) and is refused on its own where that is more.
#include <algorithm>

#include "common.h"
#include "wave_sat.h"

namespace msat {
namespace {

constexpr int kWsLdsMax = 64 * 1024;
constexpr int kWsRegForms = 4;               // forms 1..4: 2 / 4 / 8 / 16 clauses per lane
constexpr int kWsGeneric = kWsRegForms + 1;  // form 5: generic (LDS-resident row)
constexpr int kWsOcc = kWsRegForms + 2;      // form 6: occurrence lists (incremental)
constexpr int kWsForms = kWsOcc;
constexpr int kWsRegMaxClauses = 1023;       // break counts of the register forms are < 1024

struct WsArgs {
    const uint16_t *lits;
    const int32_t *problem_idx;
    const uint8_t *init_assign;
    uint8_t *assign_out, *solved;
    int32_t *flips, *num_unsat;
    int N, V, C, S, max_flips;
    uint32_t noise_p32;
    uint64_t seed, counter;
    long long lits_extent, assign_extent;  // debug builds: elements to the end of the allocations
};

__host__ __device__ constexpr int ws_assign_bytes(int V) { return (V + 15) & ~15; }

__device__ __forceinline__ uint32_t on_mask(int v0, int v1, int v2, int v) {
    return (v0 == v ? 1u : 0u) | (v1 == v ? 2u : 0u) | (v2 == v ? 4u : 0u);
}

// the variable whose flip alone breaks the clause, or -1 (tm: mask of true slots; true slots are real)
__device__ __forceinline__ int critical_var(int v0, int v1, int v2, uint32_t tm) {
    if (tm == 0u) return -1;
    const int w = (tm & 1u) ? v0 : (tm & 2u) ? v1 : v2;
    return on_mask(v0, v1, v2, w) == tm ? w : -1;
}

// Row of the sample's instance into LDS, the start assignment into LDS bytes.
__device__ __forceinline__ void ws_stage(const WsArgs &a, int s, int lane, uint2 *row, uint8_t *x) {
    wave_stage_row(a.lits, a.problem_idx, a.N, a.C, s, lane, row, a.lits_extent);
    if (a.init_assign != nullptr) {
        for (int v = lane; v < a.V; v += 64) {
            MSAT_DCHECK((size_t)s * a.V + v, a.assign_extent);
            x[v] = a.init_assign[(size_t)s * a.V + v] & 1u;
        }
    } else {
        for (int v = lane; v < a.V; v += 64) {  // msat_env_reset's draw for env s (common.h, reset_rng_block)
            const uint4 q = reset_rng_block(a.seed, a.counter, (uint32_t)s, 1u + (uint32_t)(v >> 7));
            const int wi = (v >> 5) & 3;
            const uint32_t word = wi == 0 ? q.x : wi == 1 ? q.y : wi == 2 ? q.z : q.w;
            x[v] = (uint8_t)((word >> (v & 31)) & 1u);
        }
    }
    wave_lds_sync();
}

__device__ __forceinline__ void ws_finish(const WsArgs &a, int s, int lane, const uint8_t *x, int solved, int flips,
                                          int n) {
    wave_lds_sync();
    for (int v = lane; v < a.V; v += 64) a.assign_out[(size_t)s * a.V + v] = x[v];
    if (lane == 0) {
        a.solved[s] = (uint8_t)solved;
        a.flips[s] = flips;
        a.num_unsat[s] = n;
    }
}

// The picked clause's candidates: its real slots in slot order.  Wave-uniform.
struct WsPick {
    int cv[3];
    int m;
};

__device__ __forceinline__ WsPick ws_candidates(const uint2 *row, int cidx) {
    const uint2 w = row[cidx];  // one address for the whole wave: a broadcast read
    const uint32_t lo = __builtin_amdgcn_readfirstlane(w.x), hi = __builtin_amdgcn_readfirstlane(w.y);
    const int v0 = var_of(lo & 0xFFFFu), v1 = var_of(lo >> 16), v2 = var_of(hi & 0xFFFFu);
    WsPick p;
    p.m = 0;
    p.cv[0] = p.cv[1] = p.cv[2] = -2;  // matches no critical variable
    if (v0 >= 0) p.cv[p.m++] = v0;
    if (v1 >= 0) {
        if (p.m == 0) p.cv[0] = v1; else p.cv[1] = v1;
        ++p.m;
    }
    if (v2 >= 0) {
        if (p.m == 0) p.cv[0] = v2; else if (p.m == 1) p.cv[1] = v2; else p.cv[2] = v2;
        ++p.m;
    }
    return p;
}

// Step 5 of the algorithm: the candidate to flip among m >= 1 with break counts bk.
__device__ __forceinline__ int ws_choose_slot(const WsPick &p, const int bk[3], uint32_t q1, uint32_t q2,
                                         uint32_t noise_p32) {
    int b = bk[0], jb = 0;
    if (p.m > 1 && bk[1] < b) { b = bk[1]; jb = 1; }
    if (p.m > 2 && bk[2] < b) { b = bk[2]; jb = 2; }
    int j = jb;
    if (b != 0 && q1 < noise_p32) j = (int)mulhi32(q2, (uint32_t)p.m);
    return j;
}

__device__ __forceinline__ int ws_choose(const WsPick &p, const int bk[3], uint32_t q1, uint32_t q2,
                                         uint32_t noise_p32) {
    const int j = ws_choose_slot(p, bk, q1, q2, noise_p32);
    return j == 0 ? p.cv[0] : j == 1 ? p.cv[1] : p.cv[2];
}

// x[v] ^= 1 by one lane, as an LDS atomic on the byte's word: nothing comes back, so the wave does not wait for it
// (the assignment bytes start on a 4-byte boundary in every form).
__device__ __forceinline__ void ws_flip_x(uint8_t *x, int v, int lane) {
    if (lane == 0) atomicXor(reinterpret_cast<uint32_t *>(x) + (v >> 2), 1u << (8 * (v & 3)));
}

template <int NPL>
__global__ void __launch_bounds__(64) walksat_reg_kernel(const WsArgs a) {
    extern __shared__ __align__(16) unsigned char ws_lds[];
    const int lane = threadIdx.x, s = blockIdx.x;
    uint2 *row = reinterpret_cast<uint2 *>(ws_lds);
    uint8_t *x = ws_lds + (size_t)a.C * 8;
    ws_stage(a, s, lane, row, x);

    int v0[NPL], v1[NPL], v2[NPL], crit[NPL];
    uint32_t tm[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int c = k * 64 + lane;
        v0[k] = v1[k] = v2[k] = crit[k] = -1;
        tm[k] = 1u;  // a slot past the last clause: satisfied for ever, on no variable
        if (c < a.C) {
            const uint2 w = row[c];
            const uint32_t c0 = w.x & 0xFFFFu, c1 = w.x >> 16, c2 = w.y & 0xFFFFu;
            v0[k] = var_of(c0);
            v1[k] = var_of(c1);
            v2[k] = var_of(c2);
            MSAT_DCHECK(max(max(v0[k], v1[k]), max(v2[k], 0)), a.V);
            uint32_t t = 0;
            if (v0[k] >= 0) t |= (x[v0[k]] ^ c0) & 1u;
            if (v1[k] >= 0) t |= ((x[v1[k]] ^ c1) & 1u) << 1;
            if (v2[k] >= 0) t |= ((x[v2[k]] ^ c2) & 1u) << 2;
            tm[k] = t;
            crit[k] = critical_var(v0[k], v1[k], v2[k], t);
        }
    }

    uint64_t ub[NPL];
    int n = 0;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        ub[k] = __ballot(tm[k] == 0u);
        n += __popcll(ub[k]);
    }
    int t = 0;
    for (t = 0; t < a.max_flips; ++t) {
        if (n == 0) break;
        const uint4 q = philox4x32_10(make_uint4((uint32_t)a.counter, (uint32_t)(a.counter >> 32), (uint32_t)s,
                                                 0x80000000u + (uint32_t)t),
                                      (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        // the r-th unsatisfied clause in ascending clause index
        const int r = (int)mulhi32(q.x, (uint32_t)n);
        int pre = 0, mine = 0;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            if (tm[k] == 0u && pre + lane_rank(ub[k]) == r) mine = k + 1;
            pre += __popcll(ub[k]);
        }
        const uint64_t selb = __ballot(mine != 0);
        const int L = selb ? __builtin_ctzll(selb) : 0;
        const int ksel = max(__builtin_amdgcn_readlane(mine, L) - 1, 0);
        const int cidx = min(ksel * 64 + L, a.C - 1);
        MSAT_DCHECK(selb ? ksel * 64 + L : -1, a.C);
        const WsPick p = ws_candidates(row, cidx);
        if (p.m > 0) {
            int bk[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j < p.m) {
#pragma unroll
                    for (int k = 0; k < NPL; ++k) bk[j] += __popcll(__ballot(crit[k] == p.cv[j]));
                }
            }
            const int v = ws_choose(p, bk, q.y, q.z, a.noise_p32);
            MSAT_DCHECK(v, a.V);
            ws_flip_x(x, v, lane);
            n = 0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const uint32_t on = on_mask(v0[k], v1[k], v2[k], v);
                if (on) {
                    tm[k] ^= on;
                    crit[k] = critical_var(v0[k], v1[k], v2[k], tm[k]);
                }
                ub[k] = __ballot(tm[k] == 0u);
                n += __popcll(ub[k]);
            }
        }
    }
    ws_finish(a, s, lane, x, n == 0, t, n);
}

// ------------------------------------------------------------------ generic ----
// The row stays in LDS; entry c is (code0 | code1 << 16, code2 | true-slot mask << 16).  Lane l owns the clauses
// c = l (mod 64) and is the only writer of their masks.
__global__ void __launch_bounds__(64) walksat_lds_kernel(const WsArgs a) {
    extern __shared__ __align__(16) unsigned char ws_lds[];
    const int lane = threadIdx.x, s = blockIdx.x;
    uint2 *row = reinterpret_cast<uint2 *>(ws_lds);
    uint8_t *x = ws_lds + (size_t)a.C * 8;
    ws_stage(a, s, lane, row, x);
    const int passes = (a.C + 63) / 64;

    int n = 0;
    for (int i = 0; i < passes; ++i) {
        const int c = i * 64 + lane;
        bool uns = false;
        if (c < a.C) {
            uint2 w = row[c];
            const uint32_t c0 = w.x & 0xFFFFu, c1 = w.x >> 16, c2 = w.y & 0xFFFFu;
            const int u0 = var_of(c0), u1 = var_of(c1), u2 = var_of(c2);
            MSAT_DCHECK(max(max(u0, u1), max(u2, 0)), a.V);
            uint32_t t = 0;
            if (u0 >= 0) t |= (x[u0] ^ c0) & 1u;
            if (u1 >= 0) t |= ((x[u1] ^ c1) & 1u) << 1;
            if (u2 >= 0) t |= ((x[u2] ^ c2) & 1u) << 2;
            w.y = c2 | (t << 16);
            row[c] = w;
            uns = t == 0u;
        }
        n += __popcll(__ballot(uns));
    }
    int t = 0;
    for (t = 0; t < a.max_flips; ++t) {
        if (n == 0) break;
        wave_lds_sync();
        const uint4 q = philox4x32_10(make_uint4((uint32_t)a.counter, (uint32_t)(a.counter >> 32), (uint32_t)s,
                                                 0x80000000u + (uint32_t)t),
                                      (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        const int r = (int)mulhi32(q.x, (uint32_t)n);
        int pre = 0, cidx = 0;
        for (int i = 0; i < passes; ++i) {
            const int c = i * 64 + lane;
            const bool uns = c < a.C && (row[c].y >> 16) == 0u;
            const uint64_t b = __ballot(uns);
            const int cnt = __popcll(b);
            if (r < pre + cnt) {
                const uint64_t selb = __ballot(uns && lane_rank(b) == r - pre);
                MSAT_DCHECK(selb ? 0 : -1, 1);
                cidx = min(i * 64 + (selb ? __builtin_ctzll(selb) : 0), a.C - 1);
                break;
            }
            pre += cnt;
        }
        const WsPick p = ws_candidates(row, cidx);
        if (p.m > 0) {
            int bk[3] = {0, 0, 0};
            for (int i = 0; i < passes; ++i) {
                const int c = i * 64 + lane;
                int cr = -1;
                if (c < a.C) {
                    const uint2 w = row[c];
                    cr = critical_var(var_of(w.x & 0xFFFFu), var_of(w.x >> 16), var_of(w.y & 0xFFFFu), w.y >> 16);
                }
                bk[0] += __popcll(__ballot(cr == p.cv[0]));
                bk[1] += __popcll(__ballot(cr == p.cv[1]));
                bk[2] += __popcll(__ballot(cr == p.cv[2]));
            }
            const int v = ws_choose(p, bk, q.y, q.z, a.noise_p32);
            MSAT_DCHECK(v, a.V);
            ws_flip_x(x, v, lane);
            n = 0;
            for (int i = 0; i < passes; ++i) {
                const int c = i * 64 + lane;
                bool uns = false;
                if (c < a.C) {
                    uint2 w = row[c];
                    const uint32_t on = on_mask(var_of(w.x & 0xFFFFu), var_of(w.x >> 16), var_of(w.y & 0xFFFFu), v);
                    if (on) {
                        w.y ^= on << 16;
                        row[c] = w;
                    }
                    uns = (w.y >> 16) == 0u;
                }
                n += __popcll(__ballot(uns));
            }
        }
    }
    ws_finish(a, s, lane, x, n == 0, t, n);
}

// -------------------------------------------------------- occurrence lists ----
// The incremental form: a flip of v touches only the clauses that hold v.  LDS per sample, beside the row (whose
// fourth slot holds the true-slot mask, as in the generic form) and the assignment bytes:
//   bitmap  one bit per clause, set while it is unsatisfied (64-bit words: ascending clause order is bit order),
//   brk     per variable the number of clauses whose critical variable it is: break_j is one read,
//   off     V + 1 offsets into list, list: per variable the clauses that hold it (each clause once per variable;
//           the order inside a variable's run is whatever the LDS atomics gave and changes no result, since the
//           clauses of a run are distinct and every update of a count or a bit commutes).
// Per flip: the picked clause is a walk over the bitmap words' popcounts and a k-th-set-bit select; the flip
// gives one lane per clause of v (64 at a time), which rewrites the clause's mask, moves its critical variable's
// count, toggles its bitmap bit and votes on the change of the unsatisfied count.
struct WsOccLayout {
    int w64;
    size_t bitmap, brk, off, list, x, total;
};

__host__ __device__ inline WsOccLayout ws_occ_layout(int V, int C) {
    WsOccLayout L;
    L.w64 = (C + 63) / 64;
    size_t o = 8 * (size_t)C;
    L.bitmap = o;
    o += 8 * (size_t)L.w64;
    L.brk = o;
    o += 4 * (size_t)V;
    L.off = o;
    o += 4 * ((size_t)V + 1);
    L.list = o;
    o += 2 * 3 * (size_t)C;
    o = (o + 15) & ~(size_t)15;
    L.x = o;
    L.total = o + ws_assign_bytes(V);
    return L;
}

__global__ void __launch_bounds__(64) walksat_occ_kernel(const WsArgs a) {
    extern __shared__ __align__(16) unsigned char ws_lds[];
    const int lane = threadIdx.x, s = blockIdx.x;
    const WsOccLayout L = ws_occ_layout(a.V, a.C);
    uint2 *row = reinterpret_cast<uint2 *>(ws_lds);
    uint32_t *bm32 = reinterpret_cast<uint32_t *>(ws_lds + L.bitmap);
    uint32_t *brk = reinterpret_cast<uint32_t *>(ws_lds + L.brk);
    uint32_t *off = reinterpret_cast<uint32_t *>(ws_lds + L.off);
    uint16_t *list = reinterpret_cast<uint16_t *>(ws_lds + L.list);
    uint8_t *x = ws_lds + L.x;
    ws_stage(a, s, lane, row, x);
    const int passes = (a.C + 63) / 64;
    for (int i = lane; i < 2 * L.w64; i += 64) bm32[i] = 0u;
    for (int v = lane; v < a.V; v += 64) brk[v] = 0u;
    wave_lds_sync();

    // masks, bitmap, the unsatisfied count, and per variable the number of clauses that hold it (in brk)
    int n = 0;
    for (int i = 0; i < passes; ++i) {
        const int c = i * 64 + lane;
        bool uns = false;
        if (c < a.C) {
            uint2 w = row[c];
            const uint32_t c0 = w.x & 0xFFFFu, c1 = w.x >> 16, c2 = w.y & 0xFFFFu;
            const int u0 = var_of(c0), u1 = var_of(c1), u2 = var_of(c2);
            MSAT_DCHECK(max(max(u0, u1), max(u2, 0)), a.V);
            uint32_t t = 0;
            if (u0 >= 0) t |= (x[u0] ^ c0) & 1u;
            if (u1 >= 0) t |= ((x[u1] ^ c1) & 1u) << 1;
            if (u2 >= 0) t |= ((x[u2] ^ c2) & 1u) << 2;
            w.y = c2 | (t << 16);
            row[c] = w;
            uns = t == 0u;
            if (uns) atomicOr(&bm32[c >> 5], 1u << (c & 31));
            if (u0 >= 0) atomicAdd(&brk[u0], 1u);
            if (u1 >= 0 && u1 != u0) atomicAdd(&brk[u1], 1u);
            if (u2 >= 0 && u2 != u0 && u2 != u1) atomicAdd(&brk[u2], 1u);
        }
        n += __popcll(__ballot(uns));
    }
    wave_lds_sync();
    // off = exclusive prefix of the counts
    uint32_t running = 0;
    for (int base = 0; base < a.V; base += 64) {
        const int v = base + lane;
        const uint32_t val = v < a.V ? brk[v] : 0u;
        uint32_t incl = val;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (v < a.V) off[v] = running + incl - val;
        running += __shfl(incl, 63, 64);
    }
    if (lane == 0) off[a.V] = running;
    wave_lds_sync();
    for (int v = lane; v < a.V; v += 64) brk[v] = 0u;  // now the fill cursors
    wave_lds_sync();
    for (int i = 0; i < passes; ++i) {
        const int c = i * 64 + lane;
        if (c < a.C) {
            const uint2 w = row[c];
            const int u0 = var_of(w.x & 0xFFFFu), u1 = var_of(w.x >> 16), u2 = var_of(w.y & 0xFFFFu);
            if (u0 >= 0) {
                const uint32_t at = off[u0] + atomicAdd(&brk[u0], 1u);
                MSAT_DCHECK(at, 3 * a.C);
                list[at] = (uint16_t)c;
            }
            if (u1 >= 0 && u1 != u0) {
                const uint32_t at = off[u1] + atomicAdd(&brk[u1], 1u);
                MSAT_DCHECK(at, 3 * a.C);
                list[at] = (uint16_t)c;
            }
            if (u2 >= 0 && u2 != u0 && u2 != u1) {
                const uint32_t at = off[u2] + atomicAdd(&brk[u2], 1u);
                MSAT_DCHECK(at, 3 * a.C);
                list[at] = (uint16_t)c;
            }
        }
    }
    wave_lds_sync();
    for (int v = lane; v < a.V; v += 64) brk[v] = 0u;  // now the break counts
    wave_lds_sync();
    for (int i = 0; i < passes; ++i) {
        const int c = i * 64 + lane;
        if (c < a.C) {
            const uint2 w = row[c];
            const int cr = critical_var(var_of(w.x & 0xFFFFu), var_of(w.x >> 16), var_of(w.y & 0xFFFFu), w.y >> 16);
            if (cr >= 0) atomicAdd(&brk[cr], 1u);
        }
    }

    int t = 0;
    for (t = 0; t < a.max_flips; ++t) {
        if (n == 0) break;
        wave_lds_sync();
        const uint4 q = philox4x32_10(make_uint4((uint32_t)a.counter, (uint32_t)(a.counter >> 32), (uint32_t)s,
                                                 0x80000000u + (uint32_t)t),
                                      (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        const int r = (int)mulhi32(q.x, (uint32_t)n);
        // the r-th set bit of the bitmap: lane k holds word k of the current 64 words and its popcount
        int cidx = -1, pre = 0;
        for (int cb = 0; cb < L.w64 && cidx < 0; cb += 64) {
            uint64_t wd = 0ull;
            if (cb + lane < L.w64) wd = (uint64_t)bm32[2 * (cb + lane)] | ((uint64_t)bm32[2 * (cb + lane) + 1] << 32);
            const int pc = __popcll(wd);
            const int lim = min(64, L.w64 - cb);
            for (int k = 0; k < lim; ++k) {
                const int ck = __builtin_amdgcn_readlane(pc, k);
                if (r < pre + ck) {
                    const uint64_t mask = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wd, k) |
                                          ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(wd >> 32), k)
                                           << 32);
                    const uint64_t selb = __ballot(((mask >> lane) & 1ull) && lane_rank(mask) == r - pre);
                    cidx = (cb + k) * 64 + (selb ? __builtin_ctzll(selb) : 0);
                    break;
                }
                pre += ck;
            }
        }
        MSAT_DCHECK(cidx, a.C);
        cidx = min(max(cidx, 0), a.C - 1);
        const WsPick p = ws_candidates(row, cidx);
        if (p.m > 0) {
            // break counts and list bounds of every candidate in one round of LDS reads
            int bk[3] = {0, 0, 0}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j < p.m) {
                    MSAT_DCHECK(p.cv[j], a.V);
                    bk[j] = (int)__builtin_amdgcn_readfirstlane(brk[p.cv[j]]);
                    lo[j] = (int)__builtin_amdgcn_readfirstlane(off[p.cv[j]]);
                    hi[j] = (int)__builtin_amdgcn_readfirstlane(off[p.cv[j] + 1]);
                }
            }
            const int js = ws_choose_slot(p, bk, q.y, q.z, a.noise_p32);
            const int v = js == 0 ? p.cv[0] : js == 1 ? p.cv[1] : p.cv[2];
            MSAT_DCHECK(v, a.V);
            ws_flip_x(x, v, lane);
            const int o0 = js == 0 ? lo[0] : js == 1 ? lo[1] : lo[2];
            const int cnt = min(max((js == 0 ? hi[0] : js == 1 ? hi[1] : hi[2]) - o0, 0), a.C);
            int dn = 0;
            for (int base = 0; base < cnt; base += 64) {
                const int i = base + lane;
                bool was = false, now = false;
                if (i < cnt) {
                    MSAT_DCHECK(o0 + i, 3 * a.C);
                    const int c = min((int)list[o0 + i], a.C - 1);
                    const uint2 w = row[c];
                    const int u0 = var_of(w.x & 0xFFFFu), u1 = var_of(w.x >> 16), u2 = var_of(w.y & 0xFFFFu);
                    const uint32_t old = w.y >> 16, nw = old ^ on_mask(u0, u1, u2, v);
                    row[c].y = (w.y & 0xFFFFu) | (nw << 16);
                    const int oc = critical_var(u0, u1, u2, old), nc = critical_var(u0, u1, u2, nw);
                    if (oc != nc) {
                        if (oc >= 0) atomicSub(&brk[oc], 1u);
                        if (nc >= 0) atomicAdd(&brk[nc], 1u);
                    }
                    was = old == 0u;
                    now = nw == 0u;
                    if (was != now) atomicXor(&bm32[c >> 5], 1u << (c & 31));
                }
                dn += __popcll(__ballot(now && !was)) - __popcll(__ballot(was && !now));
            }
            n += dn;
        }
    }
    ws_finish(a, s, lane, x, n == 0, t, n);
}

int ws_form_capacity(int form) {  // clauses a register form holds (forms 1..kWsRegForms)
    return std::min(64 * (2 << (form - 1)), kWsRegMaxClauses);
}

}  // namespace
}  // namespace msat

using namespace msat;

extern "C" int msat_walksat_forms(void) { return kWsForms; }

extern "C" int msat_walksat(const uint16_t *lits, int32_t num_problems, int32_t num_vars, int32_t num_clauses,
                            const int32_t *problem_idx, int32_t num_samples, const uint8_t *init_assign,
                            int32_t max_flips, uint32_t noise_p32, uint64_t seed, uint64_t counter, int32_t form,
                            uint8_t *assign_out, uint8_t *solved, int32_t *flips, int32_t *num_unsat, void *stream) {
    MSAT_REQUIRE(num_samples >= 0, "walksat: num_samples %d < 0", num_samples);
    MSAT_REQUIRE(num_vars >= 1 && num_vars <= 32000, "walksat: num_vars %d out of [1,32000]", num_vars);
    MSAT_REQUIRE(num_clauses >= 1, "walksat: num_clauses %d < 1", num_clauses);
    MSAT_REQUIRE(num_problems >= 1, "walksat: num_problems %d < 1", num_problems);
    MSAT_REQUIRE(max_flips >= 0, "walksat: max_flips %d < 0", max_flips);
    MSAT_REQUIRE(form >= 0 && form <= kWsForms, "walksat: form %d out of [0,%d]", form, kWsForms);
    if (form >= 1 && form <= kWsRegForms)
        MSAT_REQUIRE(num_clauses <= ws_form_capacity(form), "walksat: form %d holds num_clauses <= %d, got %d", form,
                     ws_form_capacity(form), num_clauses);
    long long lds = 8ll * num_clauses + ws_assign_bytes(num_vars);
    MSAT_REQUIRE(lds <= kWsLdsMax, "walksat: num_clauses %d, num_vars %d need %lld bytes of LDS per sample (8 C + V), "
                 "more than %d", num_clauses, num_vars, lds, kWsLdsMax);
    const long long occ_lds = (long long)ws_occ_layout(num_vars, num_clauses).total;
    if (form == kWsOcc)
        MSAT_REQUIRE(occ_lds <= kWsLdsMax, "walksat: form %d needs %lld bytes of LDS per sample for num_clauses %d, "
                     "num_vars %d (14 C + 9 V), more than %d", form, occ_lds, num_clauses, num_vars, kWsLdsMax);
    if (num_samples == 0) return MSAT_OK;
    MSAT_REQUIRE(lits && problem_idx && assign_out && solved && flips && num_unsat, "walksat: NULL pointer");
    if (form == 0) {
        // measured per flip of a launch's longest run: 4 clauses per lane 1.23 us against the
        // occurrence lists' 1.33 at uf50-218; 8 per lane 1.87 against 1.45 at uf100-430, 16 per lane 2.94 against
        // 1.70 at uf200-860.  So: registers up to 256 clauses, then the occurrence lists where they fit in LDS.
        form = kWsGeneric;
        for (int f = kWsRegForms; f >= 1; --f)
            if (num_clauses <= ws_form_capacity(f)) form = f;
        if (num_clauses > ws_form_capacity(2) && occ_lds <= kWsLdsMax) form = kWsOcc;
    }
    if (form == kWsOcc) lds = occ_lds;
    WsArgs a;
    a.lits = lits;
    a.problem_idx = problem_idx;
    a.init_assign = init_assign;
    a.assign_out = assign_out;
    a.solved = solved;
    a.flips = flips;
    a.num_unsat = num_unsat;
    a.N = num_problems;
    a.V = num_vars;
    a.C = num_clauses;
    a.S = num_samples;
    a.max_flips = max_flips;
    a.noise_p32 = noise_p32;
    a.seed = seed;
    a.counter = counter;
    a.lits_extent = dbg_extent(lits, sizeof(uint16_t));
    a.assign_extent = dbg_extent(init_assign, 1);
    const dim3 grid((unsigned)num_samples), block(64);
    hipStream_t st = (hipStream_t)stream;
    switch (form) {
        case 1: hipLaunchKernelGGL(walksat_reg_kernel<2>, grid, block, (size_t)lds, st, a); break;
        case 2: hipLaunchKernelGGL(walksat_reg_kernel<4>, grid, block, (size_t)lds, st, a); break;
        case 3: hipLaunchKernelGGL(walksat_reg_kernel<8>, grid, block, (size_t)lds, st, a); break;
        case 4: hipLaunchKernelGGL(walksat_reg_kernel<16>, grid, block, (size_t)lds, st, a); break;
        case kWsOcc: hipLaunchKernelGGL(walksat_occ_kernel, grid, block, (size_t)lds, st, a); break;
        default: hipLaunchKernelGGL(walksat_lds_kernel, grid, block, (size_t)lds, st, a); break;
    }
    return check_launch("walksat_kernel");
}
