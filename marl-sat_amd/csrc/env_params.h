// What every translation unit of the batched SAT environment shares: the launch parameters derived from an
// msat_env_desc, the variable -> agent split, and the host-side argument checks of the env entry points
// (env_kernels.hip: the step / reset / obs kernels; env_tables.hip: pool packing, agent tables, masks and
// features; bc_data.hip: behavioural-cloning labels and corrupted experts).
#pragma once
#include <stdlib.h>

#include <type_traits>

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

// What follows from (V, C, A) alone: the one place make_params and StaticShape derive it.
struct EnvGeom {
    int base, rem, M, D, WV, WC;
};

__host__ __device__ constexpr EnvGeom env_geom(int V, int C, int A) {
    return EnvGeom{V / A, V % A, V / A + (V % A > 0 ? 1 : 0), 2 * V + C, 2 * ((V + 63) / 64), 2 * ((C + 63) / 64)};
}

// The Shape parameter of shadow::env_kernel (env_kernels.hip).  DynShape: every geometry field is the run-time
// argument it always was.  StaticShape<V, C, A>: a kernel compiled for that one geometry (3-literal clauses) --
// pin_shape overwrites the fields at kernel entry, every helper is inlined, and the divisions, clamps, tail loops
// and argument registers that served other shapes fold away.  The host takes such a kernel only for a launch whose
// EnvParams equal the constants field by field (shape_matches).
struct DynShape {};

template <int V_, int C_, int A_>
struct StaticShape {
    static_assert(V_ >= 1 && C_ >= 1 && A_ >= 1 && A_ <= V_, "StaticShape: not a geometry make_params accepts");
    static constexpr int V = V_, C = C_, A = A_, K = 3;
    static constexpr int base = env_geom(V_, C_, A_).base, rem = env_geom(V_, C_, A_).rem;
    static constexpr int M = env_geom(V_, C_, A_).M, D = env_geom(V_, C_, A_).D;
    static constexpr int WV = env_geom(V_, C_, A_).WV, WC = env_geom(V_, C_, A_).WC;
};

template <class Shape>
__device__ __forceinline__ void pin_shape(EnvParams &p) {
    if constexpr (!std::is_same<Shape, DynShape>::value) {
        p.V = Shape::V, p.C = Shape::C, p.A = Shape::A, p.K = Shape::K;
        p.base = Shape::base, p.rem = Shape::rem, p.M = Shape::M, p.D = Shape::D;
        p.WV = Shape::WV, p.WC = Shape::WC;
    }
}

template <class Shape>
inline bool shape_matches(const EnvParams &p) {
    return p.V == Shape::V && p.C == Shape::C && p.A == Shape::A && p.K == Shape::K && p.base == Shape::base &&
           p.rem == Shape::rem && p.M == Shape::M && p.D == Shape::D && p.WV == Shape::WV &&
           p.WC == Shape::WC;
}

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
    const EnvGeom g = env_geom(p->V, p->C, p->A);
    p->base = g.base;
    p->rem = g.rem;
    p->M = g.M;
    MSAT_REQUIRE(d->max_vars_per_agent == p->M, "max_vars_per_agent %d != ceil(V/A)=%d",
                 d->max_vars_per_agent, p->M);
    p->WV = g.WV;
    p->WC = g.WC;
    p->D = g.D;
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
