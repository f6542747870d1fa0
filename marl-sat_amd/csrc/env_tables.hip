// The cold kernels around the batched SAT environment (env_kernels.hip): packing a literal pool, the per-instance
// agent tables, and the mask / feature tensors the learners read.  None of them runs in the env step.
#include "env_params.h"

namespace msat {

constexpr int kThreads = 256;

__global__ void pool_pack_kernel(const int32_t *__restrict__ lits, int NC, int K, int V,
                                 uint16_t *__restrict__ pool, int32_t *__restrict__ err) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= NC) return;
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < MSAT_LIT_SLOTS; ++j) {
        uint32_t code = MSAT_LIT_ABSENT;
        if (j < K) {
            const int lit = lits[(size_t)t * K + j];
            if (lit == 0) {
                code = MSAT_LIT_NULL;
            } else {
                // |lit| as unsigned: INT32_MIN has no int negation, and is out of range like any other |lit| > V
                const uint32_t a = lit < 0 ? 0u - (uint32_t)lit : (uint32_t)lit;
                if (a > (uint32_t)V) {
                    atomicOr(err, 1);
                    code = MSAT_LIT_NULL;
                } else {
                    code = ((uint32_t)(a - 1) << 1) | (lit < 0 ? 1u : 0u);
                }
            }
        }
        w |= (uint64_t)code << (16 * j);
    }
    reinterpret_cast<uint64_t *>(pool)[t] = w;
}

// Per-instance agent tables (env:99-128): rel[i][c] = clause c contains a var of
// agent i; nbr[i][v] = v appears in a clause related to i and is not i's.
__global__ void __launch_bounds__(kThreads)
agent_tables_kernel(EnvParams p, const uint16_t *__restrict__ lits, uint32_t *__restrict__ rel_g,
                    uint32_t *__restrict__ nbr_g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t *rel = smem;
    uint32_t *nbr = rel + (size_t)p.A * p.WC;
    const int n = blockIdx.x;
    for (int t = threadIdx.x; t < p.A * (p.WC + p.WV); t += kThreads) smem[t] = 0u;
    __syncthreads();
    const uint64_t *prow = reinterpret_cast<const uint64_t *>(lits) + (size_t)n * p.C;
    for (int c = threadIdx.x; c < p.C; c += kThreads) {
        const uint64_t w = prow[c];
        int vars[3], ags[3];
        bool nullLit = false;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t lit = (uint32_t)(w >> (16 * j)) & 0xFFFFu;
            vars[j] = lit < MSAT_LIT_ABSENT ? (int)(lit >> 1) : -1;
            ags[j] = vars[j] >= 0 ? agent_of_var(p, vars[j]) : -1;
            nullLit |= (lit == MSAT_LIT_NULL);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (ags[j] < 0) continue;
            atomicOr(&rel[ags[j] * p.WC + (c >> 5)], 1u << (c & 31));
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k == j || vars[k] < 0 || ags[k] == ags[j]) continue;
                atomicOr(&nbr[ags[j] * p.WV + (vars[k] >> 5)], 1u << (vars[k] & 31));
            }
        }
        if (nullLit && p.rem > 0) {
            // Reference quirk: literal 0 decodes to var index -1, equal to the -1 padding of
            // agent_vars rows, so the clause is "related" to every agent owning fewer than M vars.
            for (int i = p.rem; i < p.A; ++i) {
                atomicOr(&rel[i * p.WC + (c >> 5)], 1u << (c & 31));
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (vars[k] < 0 || ags[k] == i) continue;
                    atomicOr(&nbr[i * p.WV + (vars[k] >> 5)], 1u << (vars[k] & 31));
                }
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < p.A * p.WC; t += kThreads) rel_g[(size_t)n * p.A * p.WC + t] = rel[t];
    for (int t = threadIdx.x; t < p.A * p.WV; t += kThreads) nbr_g[(size_t)n * p.A * p.WV + t] = nbr[t];
}

// Per-env materialisation of the reference's mask tensors (env:99-128, :160).
__global__ void __launch_bounds__(kThreads)
env_masks_kernel(EnvParams p, msat_pool pool, const int32_t *__restrict__ problem_idx, int32_t *__restrict__ acm,
                 int32_t *__restrict__ anm, int32_t *__restrict__ l2a) {
    const int b = blockIdx.x;
    const int pidx = problem_idx[b];
    const uint32_t *rel = pool.rel + (size_t)pidx * p.A * p.WC;
    const uint32_t *nbr = pool.nbr + (size_t)pidx * p.A * p.WV;
    if (acm)
        for (int t = threadIdx.x; t < p.A * p.C; t += kThreads) {
            const int i = t / p.C, c = t - i * p.C;
            acm[(size_t)b * p.A * p.C + t] = bit(rel + i * p.WC, c) ? 1 : -1;
        }
    if (anm)
        for (int t = threadIdx.x; t < p.A * p.V; t += kThreads) {
            const int i = t / p.V, v = t - i * p.V;
            anm[(size_t)b * p.A * p.V + t] = bit(nbr + i * p.WV, v) ? 1 : -1;
        }
    if (l2a) {
        const uint64_t *prow = reinterpret_cast<const uint64_t *>(pool.lits) + (size_t)pidx * p.C;
        const int last_agent = agent_of_var(p, p.V - 1);  // var2agent[-1] wraps to the last var
        for (int t = threadIdx.x; t < p.C * p.K; t += kThreads) {
            const int c = t / p.K, j = t - c * p.K;
            const uint32_t lit = (uint32_t)(prow[c] >> (16 * j)) & 0xFFFFu;
            l2a[(size_t)b * p.C * p.K + t] = lit == MSAT_LIT_NULL ? last_agent : agent_of_var(p, (int)(lit >> 1));
        }
    }
}

__global__ void clause_features_kernel(int BC, const uint8_t *__restrict__ sat,
                                       const uint8_t *__restrict__ ntrue, float *__restrict__ f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= BC) return;
    f[3 * (size_t)t + 0] = (float)sat[t];
    f[3 * (size_t)t + 1] = (float)ntrue[t] / 3.0f;
    f[3 * (size_t)t + 2] = 1.0f;
}

__global__ void __launch_bounds__(kThreads)
static_var_features_kernel(const uint16_t *__restrict__ pool, int V, int C, float *__restrict__ f) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    int *deg = reinterpret_cast<int *>(smem);  // [2V]
    const int n = blockIdx.x;
    for (int t = threadIdx.x; t < 2 * V; t += kThreads) deg[t] = 0;
    __syncthreads();
    const uint64_t *prow = reinterpret_cast<const uint64_t *>(pool) + (size_t)n * C;
    for (int c = threadIdx.x; c < C; c += kThreads) {
        const uint64_t w = prow[c];
        for (int j = 0; j < 3; ++j) {
            const uint32_t lit = (uint32_t)(w >> (16 * j)) & 0xFFFFu;
            if (lit < MSAT_LIT_ABSENT) atomicAdd(&deg[2 * (lit >> 1) + (lit & 1)], 1);
        }
    }
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += kThreads) {
        float *o = f + ((size_t)n * V + v) * 3;
        o[0] = (float)deg[2 * v] / (float)C;
        o[1] = (float)deg[2 * v + 1] / (float)C;
        o[2] = 0.0f;
    }
}

// single-agent SatEnv clause features [is_sat, is_unsat, 1] (sat_env.py:143-160)
__global__ void clause_sat_features_kernel(int BC, const uint8_t *__restrict__ sat, float *__restrict__ f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= BC) return;
    const float s = (float)sat[t];
    f[3 * (size_t)t + 0] = s;
    f[3 * (size_t)t + 1] = 1.0f - s;
    f[3 * (size_t)t + 2] = 1.0f;
}

}  // namespace msat

using namespace msat;

extern "C" int msat_pool_pack(const int32_t *lits, int32_t num_problems, int32_t num_clauses,
                              int32_t clause_width, int32_t num_vars, uint16_t *pool,
                              int32_t *err_flag, void *stream) {
    MSAT_REQUIRE(lits && pool && err_flag, "NULL pointer");
    MSAT_REQUIRE(clause_width >= 1 && clause_width <= 3, "clause_width %d out of [1,3]", clause_width);
    MSAT_REQUIRE(num_problems >= 0 && num_clauses >= 1, "bad pool dims");
    const int NC = num_problems * num_clauses;
    if (NC == 0) return MSAT_OK;
    hipLaunchKernelGGL(pool_pack_kernel, dim3((NC + 255) / 256), dim3(256), 0, (hipStream_t)stream, lits,
                       NC, clause_width, num_vars, pool, err_flag);
    return check_launch("pool_pack_kernel");
}

extern "C" int msat_pool_agent_tables(const msat_env_desc *desc, const uint16_t *lits, uint32_t *rel, uint32_t *nbr,
                                      void *stream) {
    EnvParams p;
    int rc = make_params(desc, &p);
    if (rc) return rc;
    MSAT_REQUIRE(lits && rel && nbr, "NULL pointer");
    const size_t lds = (size_t)p.A * (p.WC + p.WV) * 4;
    MSAT_REQUIRE(lds <= 160 * 1024, "agent tables need %zu B of LDS (> 160 KiB)", lds);
    hipLaunchKernelGGL(agent_tables_kernel, dim3(p.N), dim3(kThreads), lds, (hipStream_t)stream, p, lits, rel, nbr);
    return check_launch("agent_tables_kernel");
}

extern "C" int msat_env_masks(const msat_env_desc *desc, const msat_pool *pool,
                              const msat_env_state *state, int32_t *agent_clause_masks,
                              int32_t *agent_neighbor_masks, int32_t *literal_to_agent_idx,
                              void *stream) {
    EnvParams p;
    if (int rc = env_entry(desc, state, pool, &p, /*check_empty=*/true)) return rc;
    if (p.B == 0) return MSAT_OK;
    hipLaunchKernelGGL(env_masks_kernel, dim3(p.B), dim3(kThreads), 0, (hipStream_t)stream, p, *pool,
                       state->problem_idx, agent_clause_masks, agent_neighbor_masks, literal_to_agent_idx);
    return check_launch("env_masks_kernel");
}

extern "C" int msat_clause_features(const msat_env_desc *desc, const msat_env_state *state,
                                    float *clause_features, void *stream) {
    EnvParams p;
    int rc = make_params(desc, &p);
    if (rc) return rc;
    MSAT_REQUIRE(state && state->clause_sat && state->clause_ntrue && clause_features,
                 "clause_features needs clause_sat, clause_ntrue and an output");
    const int BC = p.B * p.C;
    if (BC == 0) return MSAT_OK;
    hipLaunchKernelGGL(clause_features_kernel, dim3((BC + 255) / 256), dim3(256), 0, (hipStream_t)stream, BC,
                       state->clause_sat, state->clause_ntrue, clause_features);
    return check_launch("clause_features_kernel");
}

extern "C" int msat_clause_sat_features(const msat_env_desc *desc, const msat_env_state *state,
                                        float *clause_features, void *stream) {
    EnvParams p;
    int rc = make_params(desc, &p);
    if (rc) return rc;
    MSAT_REQUIRE(state && state->clause_sat && clause_features, "NULL pointer");
    const int BC = p.B * p.C;
    if (BC == 0) return MSAT_OK;
    hipLaunchKernelGGL(clause_sat_features_kernel, dim3((BC + 255) / 256), dim3(256), 0, (hipStream_t)stream, BC,
                       state->clause_sat, clause_features);
    return check_launch("clause_sat_features_kernel");
}

extern "C" int msat_static_var_features(const uint16_t *pool, int32_t num_problems, int32_t num_vars,
                                        int32_t num_clauses, float *var_features, void *stream) {
    MSAT_REQUIRE(pool && var_features, "NULL pointer");
    MSAT_REQUIRE(num_vars >= 1 && num_vars <= 32000 && num_clauses >= 1, "bad dims");
    const size_t lds = (size_t)num_vars * 8;
    MSAT_REQUIRE(lds <= 160 * 1024, "static_var_features: num_vars %d needs %zu B of LDS (> 160 KiB)", num_vars, lds);
    if (num_problems == 0) return MSAT_OK;
    hipLaunchKernelGGL(static_var_features_kernel, dim3(num_problems), dim3(kThreads), lds, (hipStream_t)stream, pool,
                       num_vars, num_clauses, var_features);
    return check_launch("static_var_features_kernel");
}
