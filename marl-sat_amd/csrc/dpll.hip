// Batched DPLL over the packed problem pool (msat_dpll, include/marlsat.h): the complete search beside
// walksat.hip's local search.  It returns a model or the verdict that none exists, which no local search can
// (the reference's expert tool runs pysat's Glucose3 and decides every file, src/utils/sat_solver.py).
//
// One wave per sample (a workgroup of 64 lanes), no workgroup barrier anywhere, the execution shape of
// walksat.hip: a sample is one (instance, cube), a CU is kept busy by many independent samples.  Every decision
// is a function of the assignment alone (never of lane order), so a host replay of include/marlsat.h's
// algorithm reproduces the outputs bit for bit:
//   - a propagation pass judges 64 clauses at a time against the assignment of the pass's start: it only marks
//     the unit codes (cnt[code] = 1, the same value from whichever lane), and a pass over the variables then
//     assigns the marked ones, finds opposite marks on one variable and clears the marks;
//   - the branching counts are LDS integer adds (they commute), the arg-max is a wave reduction on
//     (score, -index, phase);
//   - backtracking is one pass over the level array: there is no trail whose order could leak into a result.
// Control flow is wave-uniform (ballots), every loop is counted: the node budget bounds the outer loop, V + 1 the
// passes of a propagation, L the pops of a backtrack.
//
// LDS per sample: the instance row 8 * C, the count array 8 * V (u32 per code: positive and negative literal of
// each variable), the decision stack 4 * V, the levels 2 * V, the value bytes V (rounded up to 16); at most 64 KiB,
// larger shapes are refused.
#include "common.h"
#include "wave_sat.h"

namespace msat {
namespace {

constexpr int kDpLdsMax = 64 * 1024;
constexpr uint32_t kDpUnset = 2u;         // value byte of an unassigned variable (0 / 1: assigned)
constexpr uint32_t kDpNoCode = 0xFFFFFFFFu;

struct DpArgs {
    const uint16_t *lits;
    const int32_t *problem_idx, *cube;
    uint8_t *status, *assign_out;
    int32_t *nodes, *conflicts, *propagations;
    int N, V, C, S, cube_bits, max_nodes;
    long long lits_extent;  // debug builds: elements to the end of the allocation
};

__host__ __device__ constexpr long long dp_value_bytes(long long V) { return (V + 15) & ~15ll; }
__host__ __device__ constexpr long long dp_lds_bytes(long long V, long long C) {
    return 8 * C + 14 * V + dp_value_bytes(V);
}

// A clause against the current assignment.  open: no true slot; k: its unassigned real slots; ucode: their common
// code, kDpNoCode when there is none (k == 0) or they differ.
struct DpClause {
    bool open;
    int k;
    uint32_t ucode;
    uint32_t code[3];
    bool unset[3];
};

__device__ __forceinline__ DpClause dp_judge(const uint2 w, const uint8_t *x, int V) {
    DpClause q;
    q.code[0] = w.x & 0xFFFFu;
    q.code[1] = w.x >> 16;
    q.code[2] = w.y & 0xFFFFu;
    q.open = true;
    q.k = 0;
    q.ucode = kDpNoCode;
    bool same = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        q.unset[j] = false;
        const int v = var_of(q.code[j]);
        if (v < 0) continue;
        MSAT_DCHECK(v, V);
        const uint32_t xv = x[min(v, V - 1)];
        if (xv == kDpUnset) {
            q.unset[j] = true;
            if (q.k == 0) q.ucode = q.code[j];
            else same = same && q.code[j] == q.ucode;
            ++q.k;
        } else if ((xv ^ q.code[j]) & 1u) {
            q.open = false;
        }
    }
    if (!same) q.ucode = kDpNoCode;
    return q;
}

__global__ void __launch_bounds__(64) dpll_kernel(const DpArgs a) {
    extern __shared__ __align__(16) unsigned char dp_lds[];
    const int lane = threadIdx.x, s = blockIdx.x;
    const int V = a.V, C = a.C;
    uint2 *row = reinterpret_cast<uint2 *>(dp_lds);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(dp_lds + 8 * (size_t)C);
    uint32_t *stack = cnt + 2 * (size_t)V;
    uint16_t *level = reinterpret_cast<uint16_t *>(stack + V);
    uint8_t *x = reinterpret_cast<uint8_t *>(level + V);
    wave_stage_row(a.lits, a.problem_idx, a.N, C, s, lane, row, a.lits_extent);
    for (int v = lane; v < V; v += 64) {
        x[v] = (uint8_t)kDpUnset;
        level[v] = 0;
        cnt[2 * v] = 0u;
        cnt[2 * v + 1] = 0u;
    }
    wave_lds_sync();
    const uint32_t cube = a.cube != nullptr ? (uint32_t)a.cube[s] : 0u;
    const int passes = (C + 63) / 64;

    int L = 0, nodes = 0, conflicts = 0, props = 0, status = MSAT_DPLL_UNKNOWN;
    for (uint32_t it = 0; it <= (uint32_t)a.max_nodes; ++it) {
        // ---- step 1: propagate.  state: 0 no fixpoint (cannot be), 1 conflict, 2 fixpoint with an open clause,
        // 3 fixpoint and every clause has a true slot
        int state = 0;
        for (int pass = 0; pass <= V; ++pass) {
            bool conflict = false, unit_any = false, open_any = false;
            for (int i = 0; i < passes; ++i) {
                const int c = i * 64 + lane;
                bool cf = false, op = false;
                uint32_t ucode = kDpNoCode;
                if (c < C) {
                    const DpClause q = dp_judge(row[c], x, V);
                    op = q.open;
                    cf = q.open && q.k == 0;
                    if (q.open) ucode = q.ucode;
                }
                if (ucode != kDpNoCode) {
                    MSAT_DCHECK(ucode, 2 * V);
                    cnt[min(ucode, 2u * (uint32_t)V - 1u)] = 1u;
                }
                conflict = conflict || __ballot(cf) != 0ull;
                unit_any = unit_any || __ballot(ucode != kDpNoCode) != 0ull;
                open_any = open_any || __ballot(op) != 0ull;
                if (conflict) break;
            }
            wave_lds_sync();
            if (!conflict && !unit_any) {
                state = open_any ? 2 : 3;
                break;
            }
            // the marked variables: assigned at level L unless the pass met a conflict; the marks are cleared
            bool contra = false;
            int assigned = 0;
            for (int base = 0; base < V; base += 64) {
                const int v = base + lane;
                bool both = false, one = false;
                if (v < V) {
                    const uint32_t p = cnt[2 * v], n = cnt[2 * v + 1];
                    if (p | n) {
                        cnt[2 * v] = 0u;
                        cnt[2 * v + 1] = 0u;
                        both = p != 0u && n != 0u;
                        one = !both;
                        if (one && !conflict) {
                            x[v] = (uint8_t)(p != 0u ? 1u : 0u);
                            level[v] = (uint16_t)L;
                        }
                    }
                }
                contra = contra || __ballot(both) != 0ull;
                assigned += __popcll(__ballot(one));
            }
            wave_lds_sync();
            if (conflict || contra) {
                state = 1;
                break;
            }
            props += assigned;
        }

        if (state == 1) {
            // ---- step 2: conflict
            ++conflicts;
            for (int i = 0, depth = L; i < depth; ++i) {
                MSAT_DCHECK(L - 1, V);
                const uint32_t e = __builtin_amdgcn_readfirstlane(stack[L - 1]);
                if ((e & 1u) == 0u) break;
                --L;
            }
            if (L == 0) {
                status = MSAT_DPLL_UNSAT;
                break;
            }
            for (int v = lane; v < V; v += 64)
                if (x[v] != kDpUnset && (int)level[v] >= L) x[v] = (uint8_t)kDpUnset;
            wave_lds_sync();
            if (nodes == a.max_nodes) break;  // UNKNOWN
            ++nodes;
            MSAT_DCHECK(L - 1, V);
            const uint32_t e = __builtin_amdgcn_readfirstlane(stack[L - 1]);
            const int v = min((int)(e >> 2), V - 1);
            const uint32_t ph = ((e >> 1) & 1u) ^ 1u;
            MSAT_DCHECK(e >> 2, V);
            if (lane == 0) {
                stack[L - 1] = ((uint32_t)v << 2) | (ph << 1) | 1u;
                x[v] = (uint8_t)ph;
                level[v] = (uint16_t)L;
            }
            wave_lds_sync();
            continue;
        }
        if (state == 3) {
            status = MSAT_DPLL_SAT;  // ---- step 3
            break;
        }
        if (state != 2) break;  // the passes ran out: cannot be, UNKNOWN
        // ---- step 4: decide
        if (nodes == a.max_nodes) break;  // UNKNOWN
        for (int i = 0; i < passes; ++i) {
            const int c = i * 64 + lane;
            if (c < C) {
                const DpClause q = dp_judge(row[c], x, V);
                if (q.open) {
                    const uint32_t w = q.k == 2 ? 4u : 1u;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (q.unset[j]) {
                            MSAT_DCHECK(q.code[j], 2 * V);
                            atomicAdd(&cnt[min(q.code[j], 2u * (uint32_t)V - 1u)], w);
                        }
                    }
                }
            }
        }
        wave_lds_sync();
        // key = (score, -index, phase): the maximum is the highest score at the lowest index
        unsigned long long best = 0ull;
        for (int v = lane; v < V; v += 64) {
            const uint32_t p = cnt[2 * v], n = cnt[2 * v + 1];
            cnt[2 * v] = 0u;
            cnt[2 * v + 1] = 0u;
            if (x[v] == kDpUnset) {
                const unsigned long long key = ((unsigned long long)(p + n) << 32) |
                                               ((unsigned long long)(0x7FFFFFFFu - (uint32_t)v) << 1) |
                                               (p >= n ? 1ull : 0ull);
                best = key > best ? key : best;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best, d, 64);
            const uint32_t ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), d, 64);
            const unsigned long long other = ((unsigned long long)ohi << 32) | olo;
            best = other > best ? other : best;
        }
        const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)best);
        MSAT_DCHECK(0x7FFFFFFFu - (blo >> 1), V);
        const int v = min((int)(0x7FFFFFFFu - (blo >> 1)), V - 1);
        uint32_t ph = blo & 1u, closed = 0u;
        MSAT_DCHECK(L, V);
        if (L >= V) break;  // every level holds another variable: cannot be, UNKNOWN
        ++L;
        ++nodes;
        if (L <= a.cube_bits) {
            ph = (cube >> (L - 1)) & 1u;
            closed = 1u;
        }
        if (lane == 0) {
            stack[L - 1] = ((uint32_t)v << 2) | (ph << 1) | closed;
            x[v] = (uint8_t)ph;
            level[v] = (uint16_t)L;
        }
        wave_lds_sync();
    }

    wave_lds_sync();
    for (int v = lane; v < V; v += 64)
        a.assign_out[(size_t)s * V + v] = (uint8_t)(status == MSAT_DPLL_SAT && x[v] == 1u ? 1u : 0u);
    if (lane == 0) {
        a.status[s] = (uint8_t)status;
        a.nodes[s] = nodes;
        a.conflicts[s] = conflicts;
        a.propagations[s] = props;
    }
}

}  // namespace
}  // namespace msat

using namespace msat;

extern "C" int msat_dpll(const uint16_t *lits, int32_t num_problems, int32_t num_vars, int32_t num_clauses,
                         const int32_t *problem_idx, const int32_t *cube, int32_t num_samples, int32_t cube_bits,
                         int32_t max_nodes, uint8_t *status, uint8_t *assign_out, int32_t *nodes, int32_t *conflicts,
                         int32_t *propagations, void *stream) {
    MSAT_REQUIRE(num_samples >= 0, "dpll: num_samples %d < 0", num_samples);
    MSAT_REQUIRE(num_vars >= 1 && num_vars <= 32000, "dpll: num_vars %d out of [1,32000]", num_vars);
    MSAT_REQUIRE(num_clauses >= 1, "dpll: num_clauses %d < 1", num_clauses);
    MSAT_REQUIRE(num_problems >= 1, "dpll: num_problems %d < 1", num_problems);
    MSAT_REQUIRE(max_nodes >= 0, "dpll: max_nodes %d < 0", max_nodes);
    MSAT_REQUIRE(cube_bits >= 0 && cube_bits <= 30, "dpll: cube_bits %d out of [0,30]", cube_bits);
    const long long lds = dp_lds_bytes(num_vars, num_clauses);
    MSAT_REQUIRE(lds <= kDpLdsMax, "dpll: num_clauses %d, num_vars %d need %lld bytes of LDS per sample "
                 "(8 C + 14 V + V rounded up to 16), more than %d", num_clauses, num_vars, lds, kDpLdsMax);
    if (num_samples == 0) return MSAT_OK;
    MSAT_REQUIRE(lits && problem_idx && status && assign_out && nodes && conflicts && propagations,
                 "dpll: NULL pointer");
    DpArgs a;
    a.lits = lits;
    a.problem_idx = problem_idx;
    a.cube = cube;
    a.status = status;
    a.assign_out = assign_out;
    a.nodes = nodes;
    a.conflicts = conflicts;
    a.propagations = propagations;
    a.N = num_problems;
    a.V = num_vars;
    a.C = num_clauses;
    a.S = num_samples;
    a.cube_bits = cube_bits;
    a.max_nodes = max_nodes;
    a.lits_extent = dbg_extent(lits, sizeof(uint16_t));
    hipLaunchKernelGGL(dpll_kernel, dim3((unsigned)num_samples), dim3(64), (size_t)lds, (hipStream_t)stream, a);
    return check_launch("dpll_kernel");
}
