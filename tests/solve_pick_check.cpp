// Host check of the policy solver's order on search records (marl-sat_amd/csrc/solve_pick.h, the function
// solve_pick_kernel reduces an instance's tries with).  Built under ASan + UBSan by the Makefile target
// solve_pick_check and run by tests/test_solve_pick_cpu.py.
//
// Over every record of a small domain (first_solve in {-1, 0, 1, 2}, flips, best_unsat, best_step in {0, 1, 2},
// idx in {0, 1, 2}; a solved record has best_unsat 0 and best_step = first_solve as msat_solve_track leaves it, and
// also arbitrary values, which the order must ignore):
//   * pick_before is irreflexive, antisymmetric, total on records with distinct idx, and transitive;
//   * it agrees with the order stated in include/marlsat.h, restated here as a lexicographic key;
//   * the winner of every multiset of up to three tries (distinct idx) found by the kernel's fold -- a sentinel,
//     then "replace if before" in any visiting order -- is the first element of a brute-force sort by that key.
#include <algorithm>
#include <array>
#include <climits>
#include <cstdio>
#include <vector>

#include "solve_pick.h"

using msat::PickRec;
using msat::pick_before;

// include/marlsat.h, msat_solve_pick: solved first; solved: (first_solve, flips, idx); unsolved: (best_unsat,
// best_step, idx).
static std::array<long, 4> key_of(const PickRec &r) {
    if (r.first_solve >= 0) return {0, r.first_solve, r.flips, r.idx};
    return {1, r.best_unsat, r.best_step, r.idx};
}

static int fails = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            if (fails++ < 20) {               \
                std::printf("FAIL %s: ", #c); \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

int main() {
    std::vector<PickRec> dom;
    for (int fs = -1; fs <= 2; ++fs)
        for (int fl = 0; fl <= 2; ++fl)
            for (int bu = 0; bu <= 2; ++bu)
                for (int bs = 0; bs <= 2; ++bs)
                    for (int idx = 0; idx <= 2; ++idx) dom.push_back(PickRec{fs, fl, bu, bs, idx});
    const size_t n = dom.size();
    long pairs = 0, triples = 0;
    for (size_t i = 0; i < n; ++i) {
        const PickRec &a = dom[i];
        CHECK(!pick_before(a, a), "reflexive at %zu", i);
        for (size_t j = 0; j < n; ++j) {
            const PickRec &b = dom[j];
            const bool ab = pick_before(a, b), ba = pick_before(b, a);
            CHECK(!(ab && ba), "antisymmetry %zu %zu", i, j);
            if (a.idx != b.idx) CHECK(ab || ba, "totality %zu %zu", i, j);
            CHECK(ab == (key_of(a) < key_of(b)), "stated order %zu %zu", i, j);
            ++pairs;
        }
    }
    // transitivity over a thinned triple sweep (every 5th record: 65^3 triples)
    for (size_t i = 0; i < n; i += 5)
        for (size_t j = 0; j < n; j += 5)
            for (size_t k = 0; k < n; k += 5) {
                if (pick_before(dom[i], dom[j]) && pick_before(dom[j], dom[k]))
                    CHECK(pick_before(dom[i], dom[k]), "transitivity %zu %zu %zu", i, j, k);
                ++triples;
            }
    // the kernel's fold against a brute-force sort: tries 0, 1, 2 with every combination of the other fields of
    // a thinned domain, visited in every order
    std::vector<PickRec> base;
    for (size_t i = 0; i < n; i += 6)
        if (dom[i].idx == 0) base.push_back(dom[i]);
    long folds = 0;
    const PickRec sentinel{-1, INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    for (const PickRec &r0 : base)
        for (const PickRec &r1 : base)
            for (const PickRec &r2 : base) {
                std::array<PickRec, 3> t{r0, r1, r2};
                for (int q = 0; q < 3; ++q) t[q].idx = q;
                std::array<PickRec, 3> sorted = t;
                std::sort(sorted.begin(), sorted.end(),
                          [](const PickRec &a, const PickRec &b) { return key_of(a) < key_of(b); });
                std::array<int, 3> perm{0, 1, 2};
                do {
                    PickRec best = sentinel;
                    for (int q : perm)
                        if (pick_before(t[q], best)) best = t[q];
                    CHECK(best.idx == sorted[0].idx, "fold winner %d, sort winner %d", best.idx, sorted[0].idx);
                    ++folds;
                } while (std::next_permutation(perm.begin(), perm.end()));
            }
    if (fails) {
        std::printf("solve_pick_check: %d failure(s)\n", fails);
        return 1;
    }
    std::printf("solve_pick_check: ok (%zu records, %ld pairs, %ld triples, %ld folds)\n", n, pairs, triples, folds);
    return 0;
}
