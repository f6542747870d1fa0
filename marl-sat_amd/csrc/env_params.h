// What every translation unit of the batched SAT environment shares: the launch parameters derived from an
// msat_env_desc, the variable -> agent split, and the host-side argument checks of the env entry points
// (env_kernels.hip: the step / reset / obs kernels; env_tables.hip: pool packing, agent tables, masks and
// features; bc_data.hip: behavioural-cloning labels and corrupted experts).
#pragma once
#include <stdlib.h>

#include "common.h"

namespace msat {

struct EnvParams {
    int B, V, C, K, A, M, D;
    int WV, WC;     // uint32 words per agent row of the nbr / rel tables (even: whole 64-bit ballots)
    int base, rem;  // agent i owns [i*base + min(i,rem), +base+(i<rem))
    int max_steps, action_mode, reward_mode, N;
    float r_clause, r_sat, gamma;
    int ablate;  // diagnostics only (MARLSAT_ABLATE): bits 0-1: 0 full, 1 constant obs, 2 no obs write;
                 // bit 2: disable the XCD-major env order
    // debug builds (MSAT_DCHECK): elements from each caller buffer's pointer to the end of its allocation
    // (dbg_extent); 0 in product builds
    long long dbg_obs, dbg_assign, dbg_sat, dbg_ntrue, dbg_actions;
    // reset queue (msat_env_state.reset_queue): 0 none; 1 this autoreset launch consumes the list the previous
    // one made and makes the next one's (launch B + rq_cap workgroups); 2 the launch clears the entries of the
    // envs it modifies (the other state-modifying calls)
    int rq_mode, rq_cap;
    uint32_t rq_serial;
};

__host__ __device__ __forceinline__ int agent_lo(const EnvParams &p, int i) { return i * p.base + (i < p.rem ? i : p.rem); }
__host__ __device__ __forceinline__ int agent_size(const EnvParams &p, int i) { return p.base + (i < p.rem ? 1 : 0); }

__device__ __forceinline__ int agent_of_var(const EnvParams &p, int v) {
    const int split = p.rem * (p.base + 1);
    if (v < split) return v / (p.base + 1);
    return p.rem + (v - split) / p.base;  // base > 0 whenever v >= split
}

__device__ __forceinline__ uint32_t bit(const uint32_t *w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }

inline int make_params(const msat_env_desc *d, EnvParams *p) {
    MSAT_REQUIRE(d != nullptr, "desc is NULL");
    MSAT_REQUIRE(d->num_envs >= 0, "num_envs < 0");
    MSAT_REQUIRE(d->num_vars >= 1 && d->num_vars <= 32000, "num_vars %d out of [1,32000]", d->num_vars);
    MSAT_REQUIRE(d->num_clauses >= 1, "num_clauses %d < 1", d->num_clauses);
    MSAT_REQUIRE(d->clause_width >= 1 && d->clause_width <= 3, "clause_width %d out of [1,3]", d->clause_width);
    MSAT_REQUIRE(d->num_agents >= 1 && d->num_agents <= 1000, "num_agents %d out of [1,1000]", d->num_agents);
    MSAT_REQUIRE(d->action_mode == 0 || d->action_mode == 1, "action_mode %d", d->action_mode);
    MSAT_REQUIRE(d->reward_mode >= 0 && d->reward_mode <= 2, "reward_mode %d", d->reward_mode);
    MSAT_REQUIRE(d->obs_dtype == MSAT_OBS_I32 || d->obs_dtype == MSAT_OBS_I8, "obs_dtype %d", d->obs_dtype);
    MSAT_REQUIRE(d->num_problems >= 1, "num_problems %d < 1", d->num_problems);
    p->B = d->num_envs;
    p->V = d->num_vars;
    p->C = d->num_clauses;
    p->K = d->clause_width;
    p->A = d->num_agents;
    p->base = p->V / p->A;
    p->rem = p->V % p->A;
    p->M = p->base + (p->rem > 0 ? 1 : 0);
    MSAT_REQUIRE(d->max_vars_per_agent == p->M, "max_vars_per_agent %d != ceil(V/A)=%d",
                 d->max_vars_per_agent, p->M);
    p->WV = 2 * ((p->V + 63) / 64);
    p->WC = 2 * ((p->C + 63) / 64);
    p->D = 2 * p->V + p->C;
    p->max_steps = d->max_steps;
    p->action_mode = d->action_mode;
    p->reward_mode = d->reward_mode;
    p->N = d->num_problems;
    p->r_clause = d->r_clause;
    p->r_sat = d->r_sat;
    p->gamma = d->gamma;
    const char *ab = getenv("MARLSAT_ABLATE");
    p->ablate = ab ? atoi(ab) : 0;
    p->dbg_obs = p->dbg_assign = p->dbg_sat = p->dbg_ntrue = p->dbg_actions = 0;
    p->rq_mode = p->rq_cap = 0;  // the env launches: set_reset_queue (env_kernels.hip)
    p->rq_serial = 0;
    return MSAT_OK;
}

inline int check_state(const msat_env_state *st) {
    MSAT_REQUIRE(st != nullptr, "state is NULL");
    MSAT_REQUIRE(st->assign && st->clause_sat && st->num_unsat && st->step && st->done && st->problem_idx,
                 "a required state pointer is NULL");
    return MSAT_OK;
}

inline int check_pool(const msat_pool *pool) {
    MSAT_REQUIRE(pool != nullptr && pool->lits && pool->rel && pool->nbr, "pool (lits/rel/nbr) is NULL");
    return MSAT_OK;
}

// The preamble of an entry point that takes a desc, a state and a pool: the desc's parameters, then the state's and
// the pool's pointers.  An empty batch may pass NULL for both: its pointers are checked only with check_empty, and
// the caller returns MSAT_OK for p->B == 0 behind this.
inline int env_entry(const msat_env_desc *d, const msat_env_state *st, const msat_pool *pool, EnvParams *p,
                     bool check_empty = false) {
    if (int rc = make_params(d, p)) return rc;
    if (p->B == 0 && !check_empty) return MSAT_OK;
    if (int rc = check_state(st)) return rc;
    return check_pool(pool);
}

}  // namespace msat
