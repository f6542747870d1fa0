// The policy solver's order on search records (include/marlsat.h, msat_solve_pick): which of two tries of one
// instance is the better one.  A record is what msat_solve_track keeps per env row plus the row's try index.
//
// Plain C++ (host and device): solve_pick_kernel (solve_track.hip) reduces an instance's tries with
// pick_before, tests/solve_pick_check.cpp sweeps the same function on the host against a brute-force sort and
// checks that it is a strict total order.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MSAT_SP_HD __host__ __device__ __forceinline__
#else
#define MSAT_SP_HD inline
#endif

namespace msat {

struct PickRec {
    int32_t first_solve;  // step of the first solve (0 = the reset assignment), -1 = not solved
    int32_t flips;        // variables flipped up to the first solve (or the end of the search)
    int32_t best_unsat;   // least number of unsatisfied clauses seen (0 iff solved)
    int32_t best_step;    // the step that record was set at
    int32_t idx;          // try index within the instance: the last tie-break, so two tries never tie
};

// True iff a comes strictly before b:
//   1. a solved record before an unsolved one;
//   2. solved: fewest steps to the solve, then fewest flips, then lowest try;
//   3. unsolved: least best_unsat, then least best_step, then lowest try.
MSAT_SP_HD bool pick_before(const PickRec &a, const PickRec &b) {
    const bool sa = a.first_solve >= 0, sb = b.first_solve >= 0;
    if (sa != sb) return sa;
    if (sa) {
        if (a.first_solve != b.first_solve) return a.first_solve < b.first_solve;
        if (a.flips != b.flips) return a.flips < b.flips;
    } else {
        if (a.best_unsat != b.best_unsat) return a.best_unsat < b.best_unsat;
        if (a.best_step != b.best_step) return a.best_step < b.best_step;
    }
    return a.idx < b.idx;
}

}  // namespace msat
