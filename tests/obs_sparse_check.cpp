// Host check of the sparse delta observation write's index arithmetic (marl-sat_amd/csrc/obs_sparse.h): the same
// functions the kernel runs, swept exhaustively over small shapes against a brute-force get_obs.
//
// For every shape, element offset and (old, new) state pair:
//   * obs_elem(e) equals the brute-force observation element for every e (old and new state);
//   * the set of dirty chunks listed by sparse_task / sparse_entry over all (agent, source word) tasks equals the set
//     obtained by differencing the two brute-force images chunk by chunk;
//   * every listed entry decodes to the brute-force image's values (a chunk listed twice: both times).
// Build (marl-sat_amd/Makefile, target obs_sparse_check): host compiler, -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "obs_sparse.h"

using namespace msat;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Shape {
    ObsGeom g;
    std::vector<int> owner;        // [V] the agent owning each var
    std::vector<uint8_t> rel, nbr;  // [A][C], [A][V] byte tables
    std::vector<uint32_t> relw, nbrw;
};

static Shape make_shape(int V, int C, int vpa) {
    Shape s;
    const int A = (V + vpa - 1) / vpa;
    s.g = ObsGeom{V, C, A, 2 * V + C, 2 * ((V + 63) / 64), 2 * ((C + 63) / 64), V / A, V % A};
    s.owner.resize(V);
    int v = 0;
    for (int i = 0; i < A; ++i)  // the first rem agents own base + 1 vars, the others base
        for (int k = 0; k < s.g.base + (i < s.g.rem ? 1 : 0); ++k) s.owner[v++] = i;
    if (v != V) abort();
    s.rel.resize((size_t)A * C);
    s.nbr.resize((size_t)A * V);
    s.relw.assign((size_t)A * s.g.WC, 0u);
    s.nbrw.assign((size_t)A * s.g.WV, 0u);
    for (int i = 0; i < A; ++i) {
        const uint32_t dens = rnd() % 3;  // sparse, half, dense rows
        for (int c = 0; c < C; ++c) {
            const bool b = dens == 0 ? rnd() % 8 == 0 : dens == 1 ? rnd() % 2 : rnd() % 8 != 0;
            s.rel[(size_t)i * C + c] = b;
            if (b) s.relw[(size_t)i * s.g.WC + (c >> 5)] |= 1u << (c & 31);
        }
        for (int u = 0; u < V; ++u) {
            const bool b = dens == 0 ? rnd() % 8 == 0 : dens == 1 ? rnd() % 2 : rnd() % 8 != 0;
            s.nbr[(size_t)i * V + u] = b;
            if (b) s.nbrw[(size_t)i * s.g.WV + (u >> 5)] |= 1u << (u & 31);
        }
    }
    return s;
}

// the observation by its definition: row i = [own vars | related clauses | neighbour vars], -1 where masked
static std::vector<int> brute_obs(const Shape &s, const std::vector<uint8_t> &x, const std::vector<uint8_t> &sat) {
    const ObsGeom &g = s.g;
    std::vector<int> o((size_t)g.A * g.D);
    for (int i = 0; i < g.A; ++i) {
        int *row = &o[(size_t)i * g.D];
        for (int v = 0; v < g.V; ++v) row[v] = s.owner[v] == i ? x[v] : -1;
        for (int c = 0; c < g.C; ++c) row[g.V + c] = s.rel[(size_t)i * g.C + c] ? sat[c] : -1;
        for (int v = 0; v < g.V; ++v) row[g.V + g.C + v] = s.nbr[(size_t)i * g.V + v] ? x[v] : -1;
    }
    return o;
}

static std::vector<uint32_t> pack(const std::vector<uint8_t> &b, int words) {
    std::vector<uint32_t> w(words, 0u);
    for (size_t k = 0; k < b.size(); ++k)
        if (b[k]) w[k >> 5] |= 1u << (k & 31);
    return w;
}

static long n_cases = 0, n_chunks = 0, n_fast = 0, n_dup = 0;

#define FAIL(...)                                                              \
    do {                                                                       \
        fprintf(stderr, "obs_sparse_check: FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                                          \
        fprintf(stderr, "\n");                                                 \
        exit(1);                                                               \
    } while (0)

template <int VEC>
static void check_pair(const Shape &s, int sh, const std::vector<uint8_t> &x0, const std::vector<uint8_t> &sat0,
                       const std::vector<uint8_t> &x1, const std::vector<uint8_t> &sat1) {
    const ObsGeom &g = s.g;
    const int total = g.A * g.D;
    const std::vector<int> img0 = brute_obs(s, x0, sat0), img1 = brute_obs(s, x1, sat1);
    const std::vector<uint32_t> sx = pack(x0, g.WV), ssat = pack(sat0, g.WC), x = pack(x1, g.WV),
                                sat = pack(sat1, g.WC);
    for (int e = 0; e < total; ++e) {
        if (obs_elem(g, x.data(), sat.data(), s.relw.data(), s.nbrw.data(), e) != img1[e])
            FAIL("obs_elem(new) V=%d C=%d A=%d e=%d", g.V, g.C, g.A, e);
        if (obs_elem(g, sx.data(), ssat.data(), s.relw.data(), s.nbrw.data(), e) != img0[e])
            FAIL("obs_elem(old) V=%d C=%d A=%d e=%d", g.V, g.C, g.A, e);
    }
    std::set<int> want;  // shifted first index of every chunk with a changed element
    for (int e = 0; e < total; ++e)
        if (img0[e] != img1[e]) want.insert((e + sh) / VEC * VEC);
    std::set<int> got;
    const int U = 2 * ((g.V + 31) >> 5) + ((g.C + 31) >> 5);
    for (int t = 0; t < g.A * U; ++t) {
        SparseTask k;
        if (!sparse_task<VEC>(g, t / U, t % U, x.data(), sat.data(), sx.data(), ssat.data(), s.relw.data(),
                              s.nbrw.data(), sh, k))
            continue;
        if (k.dirty == 0) FAIL("task %d returned true with no chunk", t);
        for (uint64_t d = k.dirty; d; d &= d - 1) {
            const uint32_t entry = sparse_entry<VEC>(k, __builtin_ctzll(d));
            int ec, vals[16];
            if (VEC == 4 && (entry & kSparseFast)) {
                ec = (int)((entry >> 8) & 0x7FFFFFu) * 4;
                if (ec - sh < 0 || ec - sh + VEC > total) FAIL("fast entry leaves the block, t=%d ec=%d", t, ec);
                for (int u = 0; u < VEC; ++u) vals[u] = ((entry >> (4 + u)) & 1u) ? (int)((entry >> u) & 1u) : -1;
                ++n_fast;
            } else {
                ec = (int)entry;
                for (int u = 0; u < VEC; ++u) {
                    const int e = ec - sh + u;
                    vals[u] = e >= 0 && e < total
                                  ? obs_elem(g, x.data(), sat.data(), s.relw.data(), s.nbrw.data(), e) : -2;
                }
            }
            if (ec % VEC != 0) FAIL("entry not chunk-aligned, t=%d ec=%d", t, ec);
            for (int u = 0; u < VEC; ++u) {
                const int e = ec - sh + u;
                if (e >= 0 && e < total && vals[u] != img1[e])
                    FAIL("chunk value V=%d C=%d A=%d sh=%d t=%d e=%d: %d != %d", g.V, g.C, g.A, sh, t, e, vals[u],
                         img1[e]);
            }
            if (!got.insert(ec).second) ++n_dup;
            ++n_chunks;
        }
    }
    if (got != want)
        FAIL("dirty chunk sets differ V=%d C=%d A=%d VEC=%d sh=%d: %zu listed, %zu by differencing", g.V, g.C, g.A,
             VEC, sh, got.size(), want.size());
    ++n_cases;
}

// a new state `flips` source bits away from the old one
static void flip(std::vector<uint8_t> &x, std::vector<uint8_t> &sat, int flips) {
    const int n = (int)(x.size() + sat.size());
    std::vector<int> idx(n);
    for (int k = 0; k < n; ++k) idx[k] = k;
    for (int k = 0; k < flips; ++k) {
        const int j = k + (int)(rnd() % (uint32_t)(n - k));
        const int t = idx[k];
        idx[k] = idx[j];
        idx[j] = t;
        if (idx[k] < (int)x.size())
            x[idx[k]] ^= 1;
        else
            sat[idx[k] - x.size()] ^= 1;
    }
}

int main() {
    const int Vs[] = {1, 3, 31, 32, 33, 64}, Cs[] = {1, 31, 32, 33, 70};
    for (int V : Vs)
        for (int C : Cs) {
            const int vpas[] = {1, 3, 8, V};
            for (int vi = 0; vi < 4; ++vi) {
                const int vpa = vpas[vi] > V ? V : vpas[vi];
                const Shape s = make_shape(V, C, vpa);
                const int quarter = (V + C) / 4;  // the most source bits the quarter rule leaves to the delta write
                const int flips[] = {0, quarter, 1, 2, quarter / 2, (int)(rnd() % (uint32_t)(quarter + 1))};
                for (int f : flips) {
                    if (f > quarter) continue;
                    std::vector<uint8_t> x0(V), sat0(C);
                    for (auto &b : x0) b = rnd() & 1;
                    for (auto &b : sat0) b = rnd() & 1;
                    std::vector<uint8_t> x1 = x0, sat1 = sat0;
                    flip(x1, sat1, f);
                    for (int sh = 0; sh < 4; ++sh) check_pair<4>(s, sh, x0, sat0, x1, sat1);
                    for (int sh = 0; sh < 16; ++sh) check_pair<16>(s, sh, x0, sat0, x1, sat1);
                }
            }
        }
    printf("obs_sparse_check: ok (%ld cases, %ld chunk entries, %ld fast, %ld listed twice)\n", n_cases, n_chunks,
           n_fast, n_dup);
    return 0;
}
