// Host sweep of the direct full observation write (marl-sat_amd/csrc/obs_sparse.h: direct_task, direct_store_quad -- the
// functions write_obs_direct in env_kernels.hip runs per (agent, source word) task and lane) against obs_elem, the brute-force
// get_obs of the same header.  Stand-alone, built with the host compiler under ASan + UBSan (Makefile target
// obs_direct_check); tests/test_env_obs_direct_cpu.py builds and runs it.
//
// Over grids of (V, C, A, offset): random assignment, clause and table words (the bits past V and C set at random
// too: the writer must mask them by the task's length), the env's block placed `offset` elements past a 16-byte
// boundary inside a sentinel-filled buffer.  Checked per shape:
//   * the tasks' element ranges tile [0, A D) exactly once (every element written by one task);
//   * every element equals obs_elem; the sentinels on both sides of the block are untouched;
//   * every 16-byte store is 16-byte aligned (UBSan's alignment check on the ObsQuad store).
// The sweep must have met V and C that are no multiple of 32, rem > 0 and rem == 0, A == 1, A == V, a task shorter
// than four elements, and all four block misalignments.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "obs_sparse.h"

using namespace msat;

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

int main() {
    constexpr int kPad = 8, kSent = 7;
    long elems = 0, shapes = 0;
    bool odd_v = false, odd_c = false, rem_pos = false, rem_zero = false, one_agent = false, full_agents = false,
         short_task = false;
    const int Vs[] = {1, 5, 20, 31, 32, 33, 50, 64, 70, 100};
    const int Cs[] = {1, 3, 33, 64, 91, 130, 218};
    for (int V : Vs)
        for (int C : Cs)
            for (int A = 1; A <= V; A += (A < 8 ? 1 : 7))
                for (int offset = 0; offset < 4; ++offset) {
                    ObsGeom g{V, C, A, 2 * V + C, 2 * ((V + 63) / 64), 2 * ((C + 63) / 64), V / A, V % A};
                    const int total = A * g.D, nwV = (V + 31) >> 5, nwC = (C + 31) >> 5, U = 2 * nwV + nwC;
                    std::vector<uint32_t> x(g.WV), sat(g.WC), rel((size_t)A * g.WC), nbr((size_t)A * g.WV);
                    for (auto &w : x) w = rnd();
                    for (auto &w : sat) w = rnd();
                    for (auto &w : rel) w = rnd();
                    for (auto &w : nbr) w = rnd();
                    const size_t n = (size_t)((kPad + offset + total + kPad + 3) & ~3);
                    int32_t *buf = static_cast<int32_t *>(aligned_alloc(16, n * sizeof(int32_t)));
                    for (size_t e = 0; e < n; ++e) buf[e] = kSent;
                    int32_t *o = buf + kPad + offset;
                    std::vector<int> seen(total, 0);
                    for (int t = 0; t < A * U; ++t) {
                        const int i = t / U;
                        const DirectTask k = direct_task(g, i, t - i * U);
                        if (k.len < 1 || k.len > 32 || k.e0 < 0 || k.e0 + k.len > total) {
                            printf("V %d C %d A %d task %d: e0 %d len %d outside [0, %d)\n", V, C, A, t, k.e0, k.len,
                                   total);
                            return 1;
                        }
                        short_task |= k.len < 4;
                        for (int u = 0; u < k.len; ++u) ++seen[k.e0 + u];
                        const uint32_t m = k.region == 0   ? k.own_m
                                           : k.region == 1 ? rel[(size_t)i * g.WC + k.r]
                                                           : nbr[(size_t)i * g.WV + k.r];
                        for (int sub = 0; sub < kDirectSubs; ++sub)  // the task's eight lanes
                            direct_store_quad(o + k.e0, k.len, sub, m, k.region == 1 ? sat[k.r] : x[k.r]);
                    }
                    for (int e = 0; e < total; ++e) {
                        const int want = obs_elem(g, x.data(), sat.data(), rel.data(), nbr.data(), e);
                        if (seen[e] != 1 || o[e] != want) {
                            printf("V %d C %d A %d offset %d element %d (row %d, k %d): written %d times, holds %d, "
                                   "want %d\n", V, C, A, offset, e, e / g.D, e % g.D, seen[e], o[e], want);
                            return 1;
                        }
                    }
                    for (size_t e = 0; e < n; ++e)
                        if ((e < (size_t)(kPad + offset) || e >= (size_t)(kPad + offset + total)) && buf[e] != kSent) {
                            printf("V %d C %d A %d offset %d: a store outside the block at %ld\n", V, C, A, offset,
                                   (long)e - kPad - offset);
                            return 1;
                        }
                    free(buf);
                    elems += total;
                    ++shapes;
                    odd_v |= V % 32 != 0;
                    odd_c |= C % 32 != 0;
                    rem_pos |= g.rem > 0;
                    rem_zero |= g.rem == 0;
                    one_agent |= A == 1;
                    full_agents |= A == V;
                }
    if (!(odd_v && odd_c && rem_pos && rem_zero && one_agent && full_agents && short_task)) {
        printf("sweep missed a case: %d %d %d %d %d %d %d\n", odd_v, odd_c, rem_pos, rem_zero, one_agent, full_agents,
               short_task);
        return 1;
    }
    printf("obs_direct_check: ok (%ld shapes, %ld elements)\n", shapes, elems);
    return 0;
}
