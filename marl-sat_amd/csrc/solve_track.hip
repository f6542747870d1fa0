// The policy solver's search record on the device (gfx950): msat_solve_track_init / msat_solve_track keep, per env
// row, the best assignment seen, the first solving step and the number of variables flipped; msat_solve_pick
// chooses one winner among an instance's tries (solve_pick.h) and gathers its record.
//
// The loop these serve is marlsat/solvers/policy.py policy_search, which stands in for the reference's
// evaluation loop (src/runners/mappo_runner.py, runner:30-73): reset, then max_steps joint actions through
// step_env while remembering the first solve.  There the memory is three jnp.where selects per step inside the
// jitted scan; here it is one row kernel per step behind the env step, and the number of rows still unsolved is
// one word the host reads every 16 steps.
//
// Layout: one wave per row, lanes striding the row's bytes; four rows per workgroup.  Every row's words are
// written by lane 0 of its own wave only.  The unsolved count is a single-workgroup reduction launched behind
// the row kernel: it recomputes the word from first_solve in a fixed order (no atomics, nothing to zero).
#include "common.h"
#include "solve_pick.h"

namespace msat {

// Debug builds (MSAT_DCHECK): elements from each buffer's pointer to the end of its allocation (dbg_extent).
struct TrackDbg {
    long long assign, solved, num_unsat, prev_x, best_x, best_unsat, best_step, first_solve, flips;
};

static TrackDbg track_dbg(const uint8_t *assign, const uint8_t *solved, const int32_t *num_unsat,
                          const msat_solve_state &s) {
    return TrackDbg{dbg_extent(assign, 1),      dbg_extent(solved, 1),     dbg_extent(num_unsat, 4),
                    dbg_extent(s.prev_x, 1),    dbg_extent(s.best_x, 1),   dbg_extent(s.best_unsat, 4),
                    dbg_extent(s.best_step, 4), dbg_extent(s.first_solve, 4), dbg_extent(s.flips, 4)};
}

__global__ void __launch_bounds__(256)
solve_track_init_kernel(int B, int V, const uint8_t *__restrict__ assign, const int32_t *__restrict__ num_unsat,
                        msat_solve_state s, TrackDbg dbg) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B) return;  // wave-uniform
    const size_t o = (size_t)r * V;
    for (int j = lane; j < V; j += 64) {
        MSAT_DCHECK(o + j, dbg.assign);
        MSAT_DCHECK(o + j, dbg.prev_x);
        MSAT_DCHECK(o + j, dbg.best_x);
        const uint8_t a = assign[o + j];
        s.prev_x[o + j] = a;
        s.best_x[o + j] = a;
    }
    if (lane == 0) {
        MSAT_DCHECK(r, dbg.num_unsat);
        MSAT_DCHECK(r, dbg.best_unsat);
        MSAT_DCHECK(r, dbg.best_step);
        MSAT_DCHECK(r, dbg.first_solve);
        MSAT_DCHECK(r, dbg.flips);
        const int nu = num_unsat[r];
        s.best_unsat[r] = nu;
        s.best_step[r] = 0;
        s.flips[r] = 0;
        s.first_solve[r] = nu == 0 ? 0 : -1;
    }
}

__global__ void __launch_bounds__(256)
solve_track_kernel(int B, int V, int step, const uint8_t *__restrict__ assign, const uint8_t *__restrict__ solved,
                   const int32_t *__restrict__ num_unsat, msat_solve_state s, TrackDbg dbg) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B) return;  // wave-uniform
    MSAT_DCHECK(r, dbg.first_solve);
    if (s.first_solve[r] >= 0) return;  // frozen: a solved row changes no field (wave-uniform)
    MSAT_DCHECK(r, dbg.solved);
    MSAT_DCHECK(r, dbg.num_unsat);
    MSAT_DCHECK(r, dbg.best_unsat);
    const bool sv = solved[r] != 0;
    const int nu = num_unsat[r];
    const bool better = sv || nu < s.best_unsat[r];  // strictly fewer: a tie keeps the earlier record
    const size_t o = (size_t)r * V;
    int d = 0;
    for (int j = lane; j < V; j += 64) {
        MSAT_DCHECK(o + j, dbg.assign);
        MSAT_DCHECK(o + j, dbg.prev_x);
        const uint8_t a = assign[o + j];
        d += __popc((unsigned)(uint8_t)(a ^ s.prev_x[o + j]));
        s.prev_x[o + j] = a;
        if (better) {
            MSAT_DCHECK(o + j, dbg.best_x);
            s.best_x[o + j] = a;
        }
    }
    d = wave_sum_i32(d);
    if (lane == 0) {
        MSAT_DCHECK(r, dbg.flips);
        MSAT_DCHECK(r, dbg.best_step);
        s.flips[r] += d;
        if (better) {
            s.best_unsat[r] = sv ? 0 : nu;
            s.best_step[r] = step;
        }
        if (sv) s.first_solve[r] = step;
    }
}

// unsolved[0] = #{r : first_solve[r] < 0}: one workgroup, integer sums (any order gives the same word).
__global__ void __launch_bounds__(256)
solve_count_unsolved_kernel(int B, const int32_t *__restrict__ first_solve, int32_t *__restrict__ unsolved,
                            long long ext_first) {
    __shared__ int red[4];
    int n = 0;
    for (int r = threadIdx.x; r < B; r += 256) {
        MSAT_DCHECK(r, ext_first);
        n += first_solve[r] < 0 ? 1 : 0;
    }
    n = wave_sum_i32(n);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) unsolved[0] = red[0] + red[1] + red[2] + red[3];
}

struct PickDbg {
    long long best_x, best_unsat, best_step, first_solve, flips;
    long long o_solved, o_try, o_steps, o_flips, o_best_unsat, o_best_step, o_x;
};

// One wave per instance: lanes stride its tries, a butterfly of pick_before leaves the winner in every lane,
// then the lanes stride the winner's best_x.
__global__ void __launch_bounds__(256)
solve_pick_kernel(int P, int tries, int V, msat_solve_state s, uint8_t *__restrict__ o_solved,
                  int32_t *__restrict__ o_try, int32_t *__restrict__ o_steps, int32_t *__restrict__ o_flips,
                  int32_t *__restrict__ o_best_unsat, int32_t *__restrict__ o_best_step, uint8_t *__restrict__ o_x,
                  PickDbg dbg) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;  // wave-uniform
    const size_t row0 = (size_t)p * tries;
    PickRec best{-1, INT_MAX, INT_MAX, INT_MAX, INT_MAX};  // after every real record (idx < tries <= INT_MAX)
    for (int t = lane; t < tries; t += 64) {
        MSAT_DCHECK(row0 + t, dbg.first_solve);
        MSAT_DCHECK(row0 + t, dbg.flips);
        MSAT_DCHECK(row0 + t, dbg.best_unsat);
        MSAT_DCHECK(row0 + t, dbg.best_step);
        const PickRec c{s.first_solve[row0 + t], s.flips[row0 + t], s.best_unsat[row0 + t], s.best_step[row0 + t], t};
        if (pick_before(c, best)) best = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const PickRec c{__shfl_xor(best.first_solve, o, 64), __shfl_xor(best.flips, o, 64),
                        __shfl_xor(best.best_unsat, o, 64), __shfl_xor(best.best_step, o, 64),
                        __shfl_xor(best.idx, o, 64)};
        if (pick_before(c, best)) best = c;
    }
    const size_t src = (row0 + best.idx) * V, dst = (size_t)p * V;
    for (int j = lane; j < V; j += 64) {
        MSAT_DCHECK(src + j, dbg.best_x);
        MSAT_DCHECK(dst + j, dbg.o_x);
        o_x[dst + j] = s.best_x[src + j];
    }
    if (lane == 0) {
        MSAT_DCHECK(p, dbg.o_solved);
        MSAT_DCHECK(p, dbg.o_try);
        MSAT_DCHECK(p, dbg.o_steps);
        MSAT_DCHECK(p, dbg.o_flips);
        MSAT_DCHECK(p, dbg.o_best_unsat);
        MSAT_DCHECK(p, dbg.o_best_step);
        o_solved[p] = best.first_solve >= 0 ? 1 : 0;
        o_try[p] = best.idx;
        o_steps[p] = best.first_solve;
        o_flips[p] = best.flips;
        o_best_unsat[p] = best.best_unsat;
        o_best_step[p] = best.best_step;
    }
}

}  // namespace msat

using namespace msat;

static int require_state(const char *who, const msat_solve_state *s, bool need_unsolved) {
    MSAT_REQUIRE(s, "%s: NULL state", who);
    MSAT_REQUIRE(s->prev_x && s->best_x && s->best_unsat && s->best_step && s->first_solve && s->flips,
                 "%s: NULL pointer in the state", who);
    MSAT_REQUIRE(!need_unsolved || s->unsolved, "%s: NULL unsolved word", who);
    return MSAT_OK;
}

static int count_unsolved(int B, const msat_solve_state *s, hipStream_t st) {
    hipLaunchKernelGGL(solve_count_unsolved_kernel, dim3(1), dim3(256), 0, st, B, s->first_solve, s->unsolved,
                       dbg_extent(s->first_solve, 4));
    return check_launch("solve_count_unsolved_kernel");
}

extern "C" int msat_solve_track_init(int32_t B, int32_t V, const uint8_t *assign, const int32_t *num_unsat,
                                     const msat_solve_state *state, void *stream) {
    MSAT_REQUIRE(B >= 0, "solve_track_init: B %d < 0", B);
    MSAT_REQUIRE(V >= 1, "solve_track_init: V %d < 1", V);
    MSAT_REQUIRE(state && state->unsolved, "solve_track_init: NULL unsolved word");
    if (B) {
        int rc = require_state("solve_track_init", state, true);
        if (rc) return rc;
        MSAT_REQUIRE(assign && num_unsat, "solve_track_init: NULL pointer");
        hipLaunchKernelGGL(solve_track_init_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, V, assign,
                           num_unsat, *state, track_dbg(assign, nullptr, num_unsat, *state));
        rc = check_launch("solve_track_init_kernel");
        if (rc) return rc;
    }
    return count_unsolved(B, state, (hipStream_t)stream);
}

extern "C" int msat_solve_track(int32_t B, int32_t V, int32_t step, const uint8_t *assign, const uint8_t *solved,
                                const int32_t *num_unsat, const msat_solve_state *state, void *stream) {
    MSAT_REQUIRE(B >= 0, "solve_track: B %d < 0", B);
    MSAT_REQUIRE(V >= 1, "solve_track: V %d < 1", V);
    MSAT_REQUIRE(step >= 1, "solve_track: step %d < 1 (steps count from 1; 0 is the reset assignment)", step);
    MSAT_REQUIRE(state && state->unsolved, "solve_track: NULL unsolved word");
    if (B) {
        int rc = require_state("solve_track", state, true);
        if (rc) return rc;
        MSAT_REQUIRE(assign && solved && num_unsat, "solve_track: NULL pointer");
        hipLaunchKernelGGL(solve_track_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, V, step, assign,
                           solved, num_unsat, *state, track_dbg(assign, solved, num_unsat, *state));
        rc = check_launch("solve_track_kernel");
        if (rc) return rc;
    }
    return count_unsolved(B, state, (hipStream_t)stream);
}

extern "C" int msat_solve_pick(int32_t P, int32_t tries, int32_t V, const msat_solve_state *state, uint8_t *solved,
                               int32_t *try_out, int32_t *steps, int32_t *flips, int32_t *best_unsat,
                               int32_t *best_step, uint8_t *x, void *stream) {
    MSAT_REQUIRE(P >= 0, "solve_pick: P %d < 0", P);
    MSAT_REQUIRE(tries >= 1, "solve_pick: tries %d < 1", tries);
    MSAT_REQUIRE(V >= 1, "solve_pick: V %d < 1", V);
    MSAT_REQUIRE((long long)P * tries <= INT_MAX, "solve_pick: P * tries = %lld rows exceed int32",
                 (long long)P * tries);
    if (!P) return MSAT_OK;
    int rc = require_state("solve_pick", state, false);
    if (rc) return rc;
    MSAT_REQUIRE(solved && try_out && steps && flips && best_unsat && best_step && x, "solve_pick: NULL pointer");
    const PickDbg dbg{dbg_extent(state->best_x, 1), dbg_extent(state->best_unsat, 4), dbg_extent(state->best_step, 4),
                      dbg_extent(state->first_solve, 4), dbg_extent(state->flips, 4), dbg_extent(solved, 1),
                      dbg_extent(try_out, 4), dbg_extent(steps, 4), dbg_extent(flips, 4), dbg_extent(best_unsat, 4),
                      dbg_extent(best_step, 4), dbg_extent(x, 1)};
    hipLaunchKernelGGL(solve_pick_kernel, dim3((P + 3) / 4), dim3(256), 0, (hipStream_t)stream, P, tries, V, *state,
                       solved, try_out, steps, flips, best_unsat, best_step, x, dbg);
    return check_launch("solve_pick_kernel");
}
