/*
 * marlsat.h — C-ABI of libmarlsat.so, the MI355X (gfx950) implementation of the
 * marl-sat data-parallel hot path: the batched multi-agent SAT environment
 * (reset / step / auto-reset / local observations) and the MAPPO rollout math
 * around it (GAE + advantage normalisation).
 *
 * Every pointer is a DEVICE pointer owned by the caller (torch tensors on the
 * Python side); dims are passed explicitly; the stream is the last argument and
 * every call only enqueues work on it (no implicit device synchronisation, no
 * allocation on the hot path).  Return value: 0 on success, negative on error
 * (MSAT_EBADARG / MSAT_EHIP); msat_last_error() returns a thread-local message.
 *
 * Reference interfaces replaced (paths relative to kongqg/marl-sat):
 *   msat_pool_pack           <- jnp.abs(clauses)-1 literal decoding shared by
 *                               src/envs/multi_agent_sat_env.py:135-144 and :100
 *   msat_pool_agent_tables   <- _compute_observation_maps  src/envs/multi_agent_sat_env.py:99-128
 *                               (hoisted from every reset to once per pool instance)
 *   msat_pool_generate       <- generate_sat_cnf           src/utils/generate_cnf_dataset.py:5-42
 *                               (planted k-SAT; Philox draws on the device instead of the host Mersenne Twister)
 *   msat_env_reset           <- SATEnv.reset               src/envs/multi_agent_sat_env.py:158-181
 *                               (+ _compute_observation_maps :99-128, get_obs :345-398)
 *   msat_env_step            <- SATEnv.step_env            src/envs/multi_agent_sat_env.py:225-284
 *                               (flip decode :230-250, _calculate_satisfaction_explicit
 *                               :130-156, _calculate_rewards :183-198 / PBRS :201-223)
 *                               autoreset=1 additionally replaces the rollout's
 *                               reset-all-then-where-select  src/learners/mappo_gnn_sat_learner.py:422-464
 *   msat_env_obs             <- SATEnv.get_obs              src/envs/multi_agent_sat_env.py:345-398
 *   msat_env_masks           <- SATState.agent_clause_masks / agent_neighbor_masks /
 *                               literal_to_agent_idx        src/envs/multi_agent_sat_env.py:160-161
 *   msat_clause_features     <- SATDataWrapper._calculate_dynamic_clause_features
 *                               src/learners/mappo_gnn_sat_learner.py:176-195
 *   msat_static_var_features <- SATDataWrapper._state_to_gnn_input degrees
 *                               src/learners/mappo_gnn_sat_learner.py:150-164
 *   msat_walksat             <- solve_one (pysat Glucose3 -> one .sol per .cnf)  src/utils/sat_solver.py:5-29;
 *                               here a batched WalkSAT/SKC local search
 *   msat_dpll                <- the same tool's completeness (Glucose3 decides every file): a batched DPLL
 *                               that returns a model or the verdict UNSAT
 *   msat_solve_track / _pick <- the first-solve bookkeeping of evaluate_policy  src/runners/mappo_runner.py:30-73
 *                               (+ best-so-far assignment, flip count and the choice among restarts)
 *   msat_gae                 <- _calculate_gae + global normalisation
 *                               src/learners/mappo_gnn_sat_learner.py:504-532
 */
#ifndef MARLSAT_H
#define MARLSAT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSAT_OK 0
#define MSAT_EBADARG (-1)
#define MSAT_EHIP (-2)
#define MSAT_ECOMM (-3)

/* packed literal codes (uint16 per literal slot, clause rows padded to 4 slots) */
#define MSAT_LIT_NULL 0xFFFFu   /* literal value 0 in the int32 input: always false,  */
                                /* and (reference quirk) "matches" padded agent slots */
#define MSAT_LIT_ABSENT 0xFFFEu /* padding slot beyond the clause width: inert        */
#define MSAT_LIT_SLOTS 4

/* obs element type */
#define MSAT_OBS_I32 0 /* reference dtype (jnp.int32)                */
#define MSAT_OBS_I8 1  /* same values {-1,0,1}, 4x fewer bytes        */

/* reward modes */
#define MSAT_REWARD_SPARSE 0 /* active reference reward: 1.0 on solve else 0 (env:183-198) */
#define MSAT_REWARD_PBRS 1   /* commented reference variant (env:201-223)                  */
#define MSAT_REWARD_SINGLE_DELTA 2 /* single-agent SatEnv (src/envs/sat_env.py:77-118): f32     */
                                   /* ((u_prev - u_new) * 10 + r_sat * solved) - 0.005, u =      */
                                   /* unsat/C; done = solved || step >= max_steps (pre-increment) */

/* Static description of one batch of environments (all envs share V, C, K, A). */
typedef struct msat_env_desc {
    int32_t num_envs;           /* B */
    int32_t num_vars;           /* V  (<= 32000) */
    int32_t num_clauses;        /* C */
    int32_t clause_width;       /* K  (1..3) */
    int32_t num_agents;         /* A  (<= 1000); contiguous partition, first V%A agents get V/A+1 vars */
    int32_t max_vars_per_agent; /* M = ceil(V/A) */
    int32_t max_steps;          /* MAX_STEPS */
    int32_t action_mode;        /* 0 single-flip Discrete(M+1), 1 multi-flip MultiDiscrete([2]*M) */
    int32_t reward_mode;        /* MSAT_REWARD_* */
    int32_t obs_dtype;          /* MSAT_OBS_* */
    int32_t num_problems;       /* N instances in the device problem pool */
    float r_clause;             /* PBRS only */
    float r_sat;                /* PBRS only */
    float gamma;                /* PBRS only */
} msat_env_desc;

/* Device problem pool: packed literals + per-instance agent tables.  The tables
 * depend only on the instance and the agent partition (the reference recomputes
 * them on every reset, env:99-128), so they are built once per pool. */
typedef struct msat_pool {
    const uint16_t *lits; /* (N,C,4)  packed literal codes                          */
    const uint32_t *rel;  /* (N,A,WC) agent-clause relation bits, WC = 2*ceil(C/64) */
    const uint32_t *nbr;  /* (N,A,WV) agent neighbour-var bits,  WV = 2*ceil(V/64)  */
} msat_pool;

/* Device-resident batch state (structure of arrays, leading dim B). */
typedef struct msat_env_state {
    uint8_t *assign;      /* (B,V)   variable_assignments in {0,1}           */
    uint8_t *clause_sat;  /* (B,C)   clauses_satisfied_status                */
    uint8_t *clause_ntrue;/* (B,C)   #true literals per clause (nullable)    */
    int32_t *num_unsat;   /* (B,)    num_unsatisfied                         */
    int32_t *step;        /* (B,)    step                                    */
    uint8_t *done;        /* (B,)    done (every agent shares it)            */
    int32_t *problem_idx; /* (B,)    row of the problem pool this env solves */
    /* Reset queue (nullable; msat_reset_queue_words(B) zeroed uint32 words, 16-byte aligned, owned by the state like
     * the arrays above): each msat_env_step(autoreset=1) launch marks the envs whose NEXT step times out (their step
     * counter reaches max_steps - 1; the reference's timed_out, env:256-260), and the next launch resets the first
     * B/256 + 8 of them (rounded up to a multiple of 8; in index order) in workgroups of their own, beside the step workgroups, instead of serially
     * behind their step (their step workgroup then writes only the transition outputs, the assignment, step, done
     * and problem_idx).  Results are identical with or without it.  Used by the sparse reward mode with mode-0
     * actions and fewer than 64 agents (B a multiple of 4); the other state-modifying calls clear the entries of the
     * envs they touch.  A caller that writes the state arrays directly must zero the queue (or pass NULL).
     * reset_serial: the launch's serial, +1 per msat_env_step(autoreset=1) call on this state; a launch uses the
     * marks only if the previous launch on the state had serial reset_serial - 1. */
    uint32_t *reset_queue;
    uint32_t reset_serial;
} msat_env_state;

/* uint32 words of a msat_env_state.reset_queue for B envs. */
size_t msat_reset_queue_words(int32_t num_envs);

/* Step outputs that are NOT state (they describe the transition that was taken). */
typedef struct msat_step_out {
    float *reward;          /* (B,)  team reward (identical for every agent)        */
    uint8_t *done;          /* (B,)  dones["__all__"] of the step (pre-reset)        */
    uint8_t *solved;        /* (B,)  infos["solved"]                                 */
    int32_t *num_unsat;     /* (B,)  infos["num_unsatisfied"]  (nullable)            */
    int32_t *episode_step;  /* (B,)  infos["episode_step"]     (nullable)            */
    /* Diagnostics, not reference state (nullable; NULL in every product call): per env 8 words from
     * its workgroup's wave 0 -- [0] shader-clock counter delta (s_memtime) and [1] 100 MHz real-time
     * counter delta over the workgroup's run (clock MHz = 100 * [0] / [1]); [2] real time at its
     * start, [3..6] at the end of four phases (assignment in LDS, clause scan, agent tables staged,
     * obs bit images built; 0 where a phase does not run), [7] at its end after its stores drained.
     * bench.py reads it for the clock and the phase breakdown of its env steps. */
    uint64_t *clock_stamps; /* (B,8) */
} msat_step_out;

const char *msat_last_error(void);
int msat_version(void); /* 3: msat_env_state carries reset_queue / reset_serial (version 2 had neither), 2:
                         * msat_step_out carries clock_stamps (version 1 had no such field) */

/* Pack an int32 literal tensor (N,C,K) (signed, 1-based, 0 = null literal) into
 * the device pool layout uint16 (N,C,4).  Literals with |l| > V (INT32_MIN among
 * them) set *err_flag (device int32, caller zeroes it) to 1. */
int msat_pool_pack(const int32_t *lits, int32_t num_problems, int32_t num_clauses,
                   int32_t clause_width, int32_t num_vars, uint16_t *pool,
                   int32_t *err_flag, void *stream);

/* Build the per-instance agent tables of a packed pool for desc's partition
 * (desc->num_problems rows): rel (N,A,WC) and nbr (N,A,WV) uint32 bit words.
 * Reproduces _compute_observation_maps (env:99-128) incl. the literal-0 quirk. */
int msat_pool_agent_tables(const msat_env_desc *desc, const uint16_t *lits,
                           uint32_t *rel, uint32_t *nbr, void *stream);

/* A pool of planted random k-SAT instances drawn on the device: clauses (N,C,K) int32, signed and 1-based, ready
 * for msat_pool_pack; planted (N,V) u8, an assignment that satisfies every clause of its instance; attempts (N,)
 * int32.  The semantics are the reference generator's (src/utils/generate_cnf_dataset.py:5-42): a hidden
 * assignment; per clause K distinct variables, one uniformly chosen slot forced to agree with the hidden
 * assignment, a coin for the sign of every other slot.  The draws are Philox4x32-10 words, not the reference's
 * Mersenne Twister: the same family of instances, not the same bytes.  Instance n depends only on (seed, counter,
 * n) and the shape, so the first 64 instances of a 128-instance call are the 64-instance call's, and a host replay
 * reproduces every word (csrc/pool_gen.h holds the arithmetic the kernel runs):
 *   q(a, b) = philox4x32_10((counter lo, counter hi, n, (a << 24) | b), seed lo, seed hi), attempt a, block b.
 *   Hidden bits: blocks 0 .. HB-1, HB = ceil(V/128); variable v (0-based) is bit v % 32 of word (v % 128) / 32 of
 *   block v / 128 (the layout of the reset stream's assignment blocks).
 *   Clause c: block HB + c, words q0..q3.  Variables: Floyd's sample of K of V as in msat_bc_corrupt: for
 *   i = 0..K-1, j = V-K+i, t = (q_i * (j+1)) >> 32; slot i takes t unless an earlier slot holds t, then j.  Slots
 *   stay in pick order.  Anchor slot = ((q3 & 0xFFFF) * K) >> 16: its literal is positive iff its variable's
 *   hidden bit is 1.  Every other slot i is positive iff bit 16 + i of q3 is 1.  Variable v is literal +-(v + 1).
 * reject_isolated != 0: an attempt is accepted only if every variable occurs in some clause (an isolated variable
 * makes the first Adam step non-finite, in the reference and here alike); otherwise the instance's workgroup draws
 * attempt a + 1, up to max_attempts attempts.  attempts[n] = the accepted attempt, or -1 when none was accepted;
 * clauses and planted then hold the last attempt.  reject_isolated == 0: every instance is attempt 0.
 * Enqueues only.  num_problems == 0: MSAT_OK without a launch.  MSAT_EBADARG: num_problems < 0, num_vars outside
 * [1, 32000], num_clauses < 1, clause_width outside [1, 3] or above num_vars, HB + num_clauses >= 2^24,
 * max_attempts outside [1, 255], reject_isolated with clause_width * num_clauses < num_vars, a NULL pointer with
 * num_problems > 0.
 * (Additive entry point: msat_version() stays 3, no struct changed.) */
int msat_pool_generate(int32_t num_problems, int32_t num_vars, int32_t num_clauses, int32_t clause_width,
                       uint64_t seed, uint64_t counter, int32_t reject_isolated, int32_t max_attempts,
                       int32_t *clauses, uint8_t *planted, int32_t *attempts, void *stream);

/* Reset the envs with reset_mask[b] != 0 (NULL: all envs).
 * new_problem_idx (B,) and new_assign (B,V) are explicit inputs for exact-parity
 * runs; when NULL they are drawn from the counter-based RNG (Philox4x32-10 keyed
 * by seed, counter=(rng_counter, env)).  Writes every state field of the reset
 * envs (step=0, done=0) and their observations obs (B,A,D), D = 2V+C. */
int msat_env_reset(const msat_env_desc *desc, const msat_pool *pool,
                   const msat_env_state *state, const uint8_t *reset_mask,
                   const int32_t *new_problem_idx, const uint8_t *new_assign,
                   uint64_t seed, uint64_t rng_counter, void *obs, void *stream);

/* One batched SATEnv.step_env.  actions: (B,A) int32 (mode 0) or (B,A,M) int32
 * (mode 1, values 0/1: MultiDiscrete([2]*m); the state keeps one bit per variable, so bit 0
 * is applied — the reference's integer XOR with other values (env:246-250) leaves non-binary
 * assignments, and the Python facade rejects such actions before the call).  autoreset=0: pure step_env (state/obs are the stepped ones).
 * autoreset=1: the rollout's auto-reset — envs whose step is done are reset
 * (problem index / assignment from the explicit arrays or the RNG, exactly as
 * msat_env_reset) and state/obs hold the post-reset values, while `out` holds
 * the pre-reset reward/done/info of the step, as in the reference rollout. */
int msat_env_step(const msat_env_desc *desc, const msat_pool *pool,
                  const msat_env_state *state, const int32_t *actions,
                  int32_t autoreset, const int32_t *new_problem_idx,
                  const uint8_t *new_assign, uint64_t seed, uint64_t rng_counter,
                  const msat_step_out *out, void *obs, void *stream);

/* msat_env_step for a caller whose obs buffer persists from step to step: it writes only the observation
 * elements that changed.  obs_shadow (device, msat_obs_shadow_words(desc) uint32 words, 4-byte aligned) is the
 * library's record of what `obs` holds: per env [problem_idx or -1 | assignment bits | clause-satisfied bits].
 * Fill it with 0xFFFFFFFF words before the first call, and again whenever anything but this entry point (with
 * this pool and this desc) wrote into `obs`.  An env whose row names its current instance gets only the aligned
 * groups of delta_group_bytes (16, 64 or 128) bytes in which the observation changed; every other env, every
 * reset and a step that flips more than a quarter of the env's variable + clause bits write the whole block.
 * Every env's row is rewritten.  The state arrays may be written by the caller between calls (the new
 * observation is computed from them, the difference from the shadow).  State, outputs and observation are those
 * of msat_env_step.  obs_shadow NULL: msat_env_step.  delta_group_bytes 0: whole blocks, rows kept up to date.
 * obs_shadow with NULL obs, or another delta_group_bytes: MSAT_EBADARG.
 * (Additive entry points: msat_version() stays 3, no struct changed.) */
int msat_env_step_delta(const msat_env_desc *desc, const msat_pool *pool,
                        const msat_env_state *state, const int32_t *actions,
                        int32_t autoreset, const int32_t *new_problem_idx,
                        const uint8_t *new_assign, uint64_t seed, uint64_t rng_counter,
                        const msat_step_out *out, void *obs, uint32_t *obs_shadow,
                        int32_t delta_group_bytes, void *stream);

/* uint32 words of the obs shadow of desc's batch (0 for an invalid desc). */
size_t msat_obs_shadow_words(const msat_env_desc *desc);

/* Ragged batches (BASELINE config 5: mixed uf50/uf100/uf200): up to MSAT_MAX_GROUPS size
 * classes, each a homogeneous batch with its own desc / pool / state / obs / actions / outs,
 * advanced by ONE kernel launch (no padding to the largest instance; the reference cannot
 * mix sizes at all, runner:118 jnp.stack).  Resets draw from the counter RNG only, class g
 * keyed by seed ^ (g * 0x9E3779B97F4A7C15) -- bit-identical to msat_env_reset / msat_env_step
 * of that class alone with that seed.  All classes share obs_dtype. */
#define MSAT_MAX_GROUPS 8
int msat_env_reset_grouped(int32_t num_groups, const msat_env_desc *descs, const msat_pool *pools,
                           const msat_env_state *states, uint64_t seed, uint64_t rng_counter,
                           void *const *obs, void *stream);
int msat_env_step_grouped(int32_t num_groups, const msat_env_desc *descs, const msat_pool *pools,
                          const msat_env_state *states, const int32_t *const *actions, int32_t autoreset,
                          uint64_t seed, uint64_t rng_counter, const msat_step_out *outs, void *const *obs,
                          void *stream);

/* Workgroup size (lanes per env) that msat_env_reset / msat_env_step / msat_env_obs launch with for desc (chosen
 * from num_agents * (2 num_vars + num_clauses) and num_envs), and the one msat_env_*_grouped launch with for
 * total_envs envs over all classes: exactly what the launches use, the MARLSAT_ENV_THREADS /
 * MARLSAT_ENV_GROUP_THREADS overrides (read once per process) included.  Host-only: no GPU call.  A bad desc or
 * total_envs < 0: MSAT_EBADARG.  For tests and benchmark labels that name the kernel instantiation that ran.
 * (Additive entry points: msat_version() stays 3, no struct changed.) */
int msat_env_launch_threads(const msat_env_desc *desc);
int msat_env_group_launch_threads(int32_t total_envs);
/* The same for msat_env_step_delta, whose launches (the step kernel with the obs shadow compiled in) follow a width
 * rule of their own: for num_agents * (2 num_vars + num_clauses) >= 16384 with int32 observations, the shapes the
 * delta write is the default of, chosen for that kernel; for every other desc msat_env_launch_threads' value.
 * MARLSAT_ENV_THREADS forces both.  (Additive as well: msat_version() stays 3.) */
int msat_env_delta_launch_threads(const msat_env_desc *desc);
/* 1 if an msat_env_step_delta launch of desc with an obs shadow takes a step kernel compiled for desc's own
 * geometry (num_vars, num_clauses, num_agents; clause_width 3) instead of the kernel of any shape, else 0 (a bad
 * desc included).  Such a kernel exists for uf200-860 with 25 agents, int32 observations, at the delta rule's 256
 * lanes; it computes what the kernel of any shape computes.  MARLSAT_ENV_STATIC=0 (read once per process) turns
 * every such kernel off.  Host-only: no GPU call.  (Additive as well: msat_version() stays 3.) */
int msat_env_static_shape(const msat_env_desc *desc);

/* obs may be NULL in msat_env_reset / msat_env_step: state-only update, no observation write
 * (the single-agent SatEnv observes the GNN input instead, src/envs/sat_env.py:120-166). */

/* Behavioural-cloning joint labels: compute_joint_labels_parallel_greedy
 * (src/runners/behavioral_cloning.py:54-100) for B envs (desc->num_envs) given explicit
 * problem_idx (B,) into the packed pool lits and assignments (B,V) u8: per agent, the first
 * local var index whose single flip lowers the unsatisfied-clause count the most, if that
 * delta < tau, else the no-op index M.  labels (B,A) int32; deltas (B,V) int32 (nullable) =
 * unsat(x with v flipped) - unsat(x). */
int msat_bc_greedy_labels(const msat_env_desc *desc, const uint16_t *lits, const int32_t *problem_idx,
                          const uint8_t *assign, float tau, int32_t *labels, int32_t *deltas, void *stream);

/* Behavioural-cloning corrupted experts (src/runners/behavioral_cloning.py:121-130) on the device:
 * dst (S,V) u8, dst[s] = src[clamp(src_row[s], 0, n_src-1)] (src (n_src,V) u8) with n = min(level, V)
 * DISTINCT variables flipped.  The variables are Floyd's sample, reproducible on the host: for
 * i = 0..n-1, j = V-n+i, t = (philox4x32_10((counter lo, counter hi, s, i), seed lo, seed hi).x * (j+1)) >> 32;
 * flip t unless t is already flipped, then flip j.  level = 0 is a plain copy.
 * S < 0, V < 1, level < 0, n_src < 1, or a NULL pointer with S > 0: MSAT_EBADARG.
 * (Additive entry point: msat_version() stays 3, no struct changed.) */
int msat_bc_corrupt(const uint8_t *src, int32_t n_src, const int32_t *src_row, int32_t S, int32_t V,
                    int32_t level, uint64_t seed, uint64_t counter, uint8_t *dst, void *stream);

/* Batched WalkSAT/SKC on the device: the expert solutions of behavioural cloning for any CNF set (replaces
 * src/utils/sat_solver.py, which runs pysat's Glucose3 over a directory), and the classical local-search
 * baseline beside the learned policy.  Sample s of S runs instance clamp(problem_idx[s], 0, N-1) of the packed
 * pool lits (N,C,4).  Every decision depends only on the current assignment and the Philox stream, so a host
 * replay reproduces the outputs bit for bit.
 *   Clause truth is the env's: a code c < MSAT_LIT_ABSENT is true iff (x[c >> 1] ^ c) & 1; MSAT_LIT_NULL is
 *   always false; MSAT_LIT_ABSENT slots are inert.  The real slots of a clause are those with a code below
 *   MSAT_LIT_ABSENT, in slot order 0, 1, 2.
 *   Start: init_assign NULL: x is the assignment msat_env_reset draws for env s at (seed, counter) (block
 *   1 + v/128 of the reset stream, word (v%128)/32, bit v%32); otherwise x = init_assign[s] & 1 ((S,V) u8).
 *   Step t = 0, 1, ...:
 *    1. U = the unsatisfied clauses in ascending clause index, n = |U|.  n == 0: stop, solved = 1, flips = t.
 *       t == max_flips: stop, solved = 0, flips = t.
 *    2. q = philox4x32_10((counter lo, counter hi, s, 0x80000000 + t), seed lo, seed hi), words q0, q1, q2
 *       (the reset blocks use c3 = 0 .. 1 + V/128, so the two ranges never meet).
 *    3. The clause U[(q0 * n) >> 32]; its candidates are its real slots j = 0..m-1 with variable v_j.  m == 0
 *       (null literals only): nothing flips, t advances.
 *    4. break_j = the number of clauses satisfied now and unsatisfied after flipping v_j alone (a clause breaks
 *       iff its set of true slots is non-empty and equals its set of slots on v_j).
 *    5. b = min_j break_j.  b == 0 or q1 >= noise_p32: flip the first slot with break_j == b; otherwise flip
 *       slot (q2 * m) >> 32.
 *   Outputs per sample: assign_out (S,V) u8 the final x, solved (S,) u8, flips (S,) i32, num_unsat (S,) i32 the
 *   final n.
 * form: 0 picks the kernel form (registers up to 256 clauses, then form 6 where it fits, else 3, 4 or 5);
 * 1..msat_walksat_forms() force one.  Forms 1..4 keep 2 / 4 / 8 / 16 clauses per lane in registers
 * (num_clauses <= 128 / 256 / 512 / 1023); form 5 walks the LDS copy of the instance and takes any num_clauses;
 * form 6 keeps per-variable clause lists, break counts and an unsatisfied-clause bitmap in LDS, so that a flip
 * touches only the clauses of its variable.  All forms give the same outputs.  Every form needs
 * 8 * num_clauses + num_vars (rounded up to 16) <= 65536 bytes of LDS per sample; form 6 needs
 * 14 * num_clauses + 8 * ceil(num_clauses / 64) + 9 * num_vars + 4 (rounded up to 16) <= 65536 and is refused
 * when forced on a larger shape (form 0 then takes another form).
 * Enqueues only.  num_samples == 0: MSAT_OK without a launch.  MSAT_EBADARG: a NULL pointer (init_assign
 * excepted) with num_samples > 0, num_vars outside [1, 32000], num_clauses < 1, num_problems < 1, max_flips < 0,
 * num_samples < 0, form outside 0..msat_walksat_forms(), a forced form that cannot hold num_clauses, a shape
 * past the LDS bound.
 * (Additive entry points: msat_version() stays 3, no struct changed.) */
int msat_walksat(const uint16_t *lits, int32_t num_problems, int32_t num_vars, int32_t num_clauses,
                 const int32_t *problem_idx, int32_t num_samples, const uint8_t *init_assign,
                 int32_t max_flips, uint32_t noise_p32, uint64_t seed, uint64_t counter, int32_t form,
                 uint8_t *assign_out, uint8_t *solved, int32_t *flips, int32_t *num_unsat, void *stream);
int msat_walksat_forms(void); /* number of kernel forms; form 0 = automatic, 1..n force one */

/* Batched DPLL on the device: the complete search beside msat_walksat's local search.  It decides an instance
 * (a model, or the verdict that none exists) where the reference's expert tool runs pysat's Glucose3
 * (src/utils/sat_solver.py).  Sample s of S searches instance clamp(problem_idx[s], 0, N-1) of the packed pool
 * lits (N,C,4) under the cube cube[s] (cube NULL: cube 0 for every sample).  No decision depends on lane order,
 * so a host replay of the text below reproduces every output bit for bit.
 *   Clause truth and real slots are msat_walksat's: a code c < MSAT_LIT_ABSENT is the literal of variable c >> 1
 *   and is true iff (x[c >> 1] ^ c) & 1 (and only where that variable is assigned); MSAT_LIT_NULL is always false;
 *   MSAT_LIT_ABSENT slots are inert.  The real slots of a clause are those with a code below MSAT_LIT_ABSENT.
 *   Per sample: every variable starts unassigned, L = 0, nodes = conflicts = propagations = 0.  The decision
 *   stack holds one (variable, phase, closed) entry per level 1..L; every assigned variable carries the level
 *   at which it was assigned.  Repeat:
 *    1. Propagate to a fixpoint in synchronous passes (at most V + 1).  A pass judges every clause against the
 *       assignment as it stood at the start of the pass.  A clause with no true slot and no unassigned real slot
 *       is a conflict.  A clause with no true slot, at least one unassigned real slot and the same code in all
 *       its unassigned real slots is a unit for that code.  Any conflict: go to 2.  No unit: the fixpoint, go
 *       to 3.  Two units of the pass on one variable with opposite signs: a conflict, go to 2 (the pass assigns
 *       nothing that counts).  Otherwise every unit's variable is assigned at level L so that the unit's code is
 *       true, propagations += the number of distinct variables assigned, and the next pass runs.
 *    2. Conflict: conflicts += 1.  Pop levels while L > 0 and the top entry is closed.  L == 0: status UNSAT,
 *       stop.  Otherwise every variable whose level is >= L becomes unassigned.  nodes == max_nodes: status
 *       UNKNOWN, stop.  Otherwise nodes += 1, the top entry (v, phase, open) becomes (v, phase ^ 1, closed), v is
 *       assigned phase ^ 1 at level L, go to 1.
 *    3. Model check: no clause is without a true slot: status SAT, assign_out = the assignment with unassigned
 *       variables written as 0, stop.
 *    4. Decide.  nodes == max_nodes: status UNKNOWN, stop.  cnt[.] = 0; for every open clause (one with no true
 *       slot), with k its number of unassigned real slots and w = 4 if k == 2, else 1: cnt[code] += w for each
 *       of its unassigned real slots (per slot, duplicates included).  v = the unassigned variable that
 *       maximises cnt[2v] + cnt[2v+1], the lowest index on ties; phase = 1 if cnt[2v] >= cnt[2v+1], else 0.
 *       L += 1, nodes += 1.  L <= cube_bits: phase = bit L-1 of cube[s] and the entry is pushed closed;
 *       otherwise it is pushed open.  v is assigned phase at level L, go to 1.
 *   A cube so fixes the phases of the first cube_bits decisions along its own path and never tries their other
 *   branch: over the 2^cube_bits cubes of an instance the searches partition the tree.  The instance is SAT iff
 *   some cube is SAT, UNSAT iff every cube is UNSAT, undecided otherwise (no cube SAT, some cube UNKNOWN).  A
 *   cube whose path ends above depth cube_bits ignores its unused bits (its siblings report the same result).
 *   Outputs per sample: status (S,) u8 MSAT_DPLL_SAT / MSAT_DPLL_UNSAT / MSAT_DPLL_UNKNOWN; assign_out (S,V) u8 a
 *   model when status is SAT, zeros otherwise; nodes, conflicts, propagations (S,) i32.
 * One wave per sample.  LDS per sample: 8 * num_clauses (the instance row) + 8 * num_vars (the two count arrays,
 * u32) + 4 * num_vars (the decision stack) + 2 * num_vars (16-bit levels) + num_vars rounded up to 16 (value
 * bytes) = 8 C + 14 V + ceil16(V) <= 65536 bytes.
 * Enqueues only.  num_samples == 0: MSAT_OK without a launch.  MSAT_EBADARG: a NULL pointer (cube excepted) with
 * num_samples > 0, num_vars outside [1, 32000], num_clauses < 1, num_problems < 1, num_samples < 0,
 * max_nodes < 0, cube_bits outside [0, 30], a shape past the LDS bound.
 * (Additive entry point: msat_version() stays 3, no struct changed.) */
#define MSAT_DPLL_UNKNOWN 0
#define MSAT_DPLL_SAT 1
#define MSAT_DPLL_UNSAT 2
int msat_dpll(const uint16_t *lits, int32_t num_problems, int32_t num_vars, int32_t num_clauses,
              const int32_t *problem_idx, const int32_t *cube, int32_t num_samples, int32_t cube_bits,
              int32_t max_nodes, uint8_t *status, uint8_t *assign_out, int32_t *nodes, int32_t *conflicts,
              int32_t *propagations, void *stream);

/* The policy solver's search record (marlsat/solvers/policy.py): what a policy search remembers per env row
 * while it steps B envs of V variables.  It replaces the three jnp.where selects per step with which the
 * reference's evaluation loop remembers the first solve (src/runners/mappo_runner.py, runner:30-73), and adds
 * what that loop drops: the best assignment of a row that never solves, and the number of variables flipped.
 * All arrays are caller-allocated device memory; the entry points only enqueue. */
typedef struct msat_solve_state {
    uint8_t *prev_x;      /* (B,V) the assignment after the last tracked step                       */
    uint8_t *best_x;      /* (B,V) the assignment of the record below (the solution once solved)    */
    int32_t *best_unsat;  /* (B,)  least number of unsatisfied clauses seen (0 once solved)         */
    int32_t *best_step;   /* (B,)  the step that record was set at (0 = the reset assignment)       */
    int32_t *first_solve; /* (B,)  step of the first solve, -1 = not solved                         */
    int32_t *flips;       /* (B,)  variables flipped up to the first solve (or up to the last step) */
    int32_t *unsolved;    /* (1,)  number of rows with first_solve < 0 after the call               */
} msat_solve_state;

/* msat_solve_track_init: the record of the reset assignment.  assign (B,V) u8, num_unsat (B,) i32 (the env
 * state's arrays after a reset).  Per row: prev_x = best_x = assign, best_unsat = num_unsat, best_step = 0,
 * flips = 0, first_solve = 0 where num_unsat == 0, else -1.
 * msat_solve_track: call after env step number `step` (1-based) with the state's assignment and the step's
 * outputs solved (B,) u8 and num_unsat (B,) i32.  For a row with first_solve < 0:
 *   flips += popcount(prev_x ^ assign) over the row, then prev_x = assign;
 *   solved != 0:                  first_solve = step, best_step = step, best_unsat = 0, best_x = assign;
 *   else num_unsat < best_unsat:  best_unsat = num_unsat, best_step = step, best_x = assign (strictly fewer: a
 *                                 tie keeps the earlier record).
 * A row with first_solve >= 0 is frozen: no field of it changes, whatever the env does afterwards.
 * After either call unsolved[0] is the number of rows with first_solve < 0, recomputed from first_solve by a
 * single-workgroup launch behind the row kernel (the caller never zeroes it; every word has one writer, so two
 * identical runs leave identical words).
 * B == 0: unsolved[0] = 0, nothing else.  MSAT_EBADARG: B < 0, V < 1, step < 1, a NULL state or unsolved word,
 * any other NULL pointer with B > 0.
 * (Additive entry points: msat_version() stays 3, no struct changed.) */
int msat_solve_track_init(int32_t B, int32_t V, const uint8_t *assign, const int32_t *num_unsat,
                          const msat_solve_state *state, void *stream);
int msat_solve_track(int32_t B, int32_t V, int32_t step, const uint8_t *assign, const uint8_t *solved,
                     const int32_t *num_unsat, const msat_solve_state *state, void *stream);

/* One winner per instance among its tries: instance p of P owns the rows p * tries .. p * tries + tries - 1 of
 * state (P * tries rows of V variables; prev_x and unsolved are not read).  Order (csrc/solve_pick.h):
 *   1. a solved row (first_solve >= 0) beats an unsolved one;
 *   2. among solved rows: fewest first_solve, then fewest flips, then lowest try;
 *   3. among unsolved rows: least best_unsat, then least best_step, then lowest try.
 * Outputs of the winner, (P,) each: solved u8, try_out (its index within the instance), steps = first_solve
 * (-1 where unsolved), flips, best_unsat, best_step; x (P,V) u8 = its best_x.
 * P == 0: MSAT_OK without a launch.  MSAT_EBADARG: P < 0, tries < 1, V < 1, P * tries > INT32_MAX, a NULL
 * pointer with P > 0.
 * (Additive entry point: msat_version() stays 3, no struct changed.) */
int msat_solve_pick(int32_t P, int32_t tries, int32_t V, const msat_solve_state *state, uint8_t *solved,
                    int32_t *try_out, int32_t *steps, int32_t *flips, int32_t *best_unsat, int32_t *best_step,
                    uint8_t *x, void *stream);

/* Single-agent SatEnv clause features [is_sat, is_unsat, 1] (B,C,3) (src/envs/sat_env.py:143-160). */
int msat_clause_sat_features(const msat_env_desc *desc, const msat_env_state *state,
                             float *clause_features, void *stream);

/* SATEnv.get_obs (env:345-398) of the current state, without changing it. */
int msat_env_obs(const msat_env_desc *desc, const msat_pool *pool,
                 const msat_env_state *state, void *obs, void *stream);

/* Materialise the reference's per-env static mask tensors (cold path):
 * agent_clause_masks (B,A,C) int32 +-1, agent_neighbor_masks (B,A,V) int32 +-1,
 * literal_to_agent_idx (B,C,K) int32.  Any output pointer may be NULL. */
int msat_env_masks(const msat_env_desc *desc, const msat_pool *pool,
                   const msat_env_state *state, int32_t *agent_clause_masks,
                   int32_t *agent_neighbor_masks, int32_t *literal_to_agent_idx,
                   void *stream);

/* Dynamic clause features (B,C,3) float32 = [is_sat, ntrue/3, 1]. */
int msat_clause_features(const msat_env_desc *desc, const msat_env_state *state,
                         float *clause_features, void *stream);

/* Static variable features (N,V,3) float32 = [deg+/C, deg-/C, 0] per pool row.
 * 8 bytes of LDS per variable: num_vars > 20480 (more than 160 KiB) is MSAT_EBADARG. */
int msat_static_var_features(const uint16_t *pool, int32_t num_problems,
                             int32_t num_vars, int32_t num_clauses,
                             float *var_features, void *stream);

/* GAE over a (T,B) rollout + global normalisation over all T*B entries.
 * reward: team reward with row stride reward_stride (elements) per (t,b)
 * (reward[...,0] of the reference's (T,B,A) reward; stride 1 for a (T,B) tensor).
 * done: (T,B) uint8.  value: (T,B).  last_val: (B,).
 * gamma_lambda is GAMMA*GAE_LAMBDA rounded once to float32 (the reference
 * multiplies the two Python floats before the fp32 arithmetic).
 * advantages/targets: (T,B) outputs (advantages normalised when normalize!=0,
 * targets = raw advantages + value).  workspace: >= msat_gae_workspace_bytes(T,B)
 * bytes; after the call workspace holds (double) the mean and the std+1e-8 used. */
size_t msat_gae_workspace_bytes(int32_t T, int32_t B);
int msat_gae(int32_t T, int32_t B, const float *reward, int32_t reward_stride,
             const uint8_t *done, const float *value, const float *last_val,
             float gamma, float gamma_lambda, int32_t normalize, float *advantages,
             float *targets, void *workspace, void *stream);

/* Global-normalisation pieces for multi-GPU GAE (the reference normalises over ALL
 * T*B advantages, learner:529-532): per-rank moments (fp64 sum, sum of squares;
 * workspace >= 2*1024 doubles), all-reduced by the caller, then x = (x - mean)/std. */
int msat_moments(const float *x, size_t n, double *out2, void *workspace, void *stream);
int msat_standardize(float *x, size_t n, float mean, float stdv, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MARLSAT_H */
