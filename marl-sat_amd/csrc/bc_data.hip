// Behavioural-cloning data on the device: the greedy joint labels of a batch of states and the corrupted copies of
// expert solutions (behavioral_cloning.py).  Cold: run once per dataset, never in the env step.
#include <algorithm>

#include "env_params.h"

namespace msat {

constexpr int kThreads = 256;

// ------------------------------------------------------- BC joint labels ----
// behavioral_cloning.py:54-100 (compute_joint_labels_parallel_greedy) for a batch: per env,
// delta[v] = unsat(x with v flipped) - unsat(x) for every var (one pass over the clauses: a clause
// changes status under the flip of v iff re-evaluating it with v flipped differs; duplicate vars in
// a clause are counted once, literal 0 stays false), then per agent the first local index with the
// smallest delta among strictly improving flips; label = that index if best < tau, else M (no-op).
__global__ void __launch_bounds__(kThreads)
bc_labels_kernel(EnvParams p, const uint16_t *__restrict__ lits, const int32_t *__restrict__ pidx,
                 const uint8_t *__restrict__ assign, float tau, int32_t *__restrict__ labels,
                 int32_t *__restrict__ deltas) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t *xb = smem;                               // [WV] assignment bits
    int *dl = reinterpret_cast<int *>(smem + p.WV);    // [V]
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t *xg = assign + (size_t)b * p.V;
    for (int t = tid; t < p.WV; t += kThreads) {
        uint32_t w = 0;
        for (int k = 0; k < 32; ++k) {
            const int v = 32 * t + k;
            if (v < p.V && (xg[v] & 1u)) w |= 1u << k;
        }
        xb[t] = w;
    }
    for (int v = tid; v < p.V; v += kThreads) dl[v] = 0;
    __syncthreads();
    const uint64_t *prow = reinterpret_cast<const uint64_t *>(lits) + (size_t)pidx[b] * p.C;
    for (int c = tid; c < p.C; c += kThreads) {
        const uint64_t w = prow[c];
        int var[MSAT_LIT_SLOTS];
        bool val[MSAT_LIT_SLOTS];
        bool old = false;
#pragma unroll
        for (int j = 0; j < MSAT_LIT_SLOTS; ++j) {
            const uint32_t code = (uint32_t)(w >> (16 * j)) & 0xFFFFu;
            var[j] = code >= MSAT_LIT_ABSENT ? -1 : (int)(code >> 1);  // NULL / ABSENT: no variable, false
            val[j] = var[j] >= 0 && ((((xb[var[j] >> 5] >> (var[j] & 31)) & 1u) ^ (code & 1u)) != 0u);
            old = old || val[j];
        }
#pragma unroll
        for (int j = 0; j < MSAT_LIT_SLOTS; ++j) {
            const int v = var[j];
            if (v < 0) continue;
            bool dup = false;
#pragma unroll
            for (int k = 0; k < j; ++k) dup = dup || (var[k] == v);
            if (dup) continue;
            bool nw = false;
#pragma unroll
            for (int k = 0; k < MSAT_LIT_SLOTS; ++k) nw = nw || (var[k] >= 0 && (val[k] != (var[k] == v)));
            if (nw != old) atomicAdd(&dl[v], old ? 1 : -1);
        }
    }
    __syncthreads();
    if (deltas)
        for (int v = tid; v < p.V; v += kThreads) deltas[(size_t)b * p.V + v] = dl[v];
    for (int i = tid; i < p.A; i += kThreads) {
        int best = 0, bi = p.M;
        const int lo = agent_lo(p, i), n = agent_size(p, i);
        for (int j = 0; j < n; ++j) {
            const int d = dl[lo + j];
            if (d < best) {
                best = d;
                bi = j;
            }
        }
        labels[(size_t)b * p.A + i] = ((float)best < tau) ? bi : p.M;
    }
}

// ------------------------------------------------- BC corrupted experts ----
// behavioral_cloning.py:121-130 for a batch: sample s is expert row src_row[s] (clamped into the table)
// with n = min(level, V) distinct variables flipped.  The n variables are Floyd's sample of [0, V): for
// i = 0..n-1, j = V - n + i, t = mulhi32(philox(counter, s, i).x, j + 1) in [0, j]; take t unless it is
// already taken, then j (never taken before: earlier picks are <= j - 1).  Every pick flips once, so
// "taken" is dst != src at that position and the sample needs no scratch.  One thread per sample: the
// draws of a sample are sequential and each thread reads back only bytes it stored itself (a one-off
// preprocessing pass over N x NUM_SAMPLES_PER_EXPERT rows of V bytes).
__global__ void __launch_bounds__(256)
bc_corrupt_kernel(const uint8_t *__restrict__ src, int n_src, const int32_t *__restrict__ src_row, int S, int V,
                  int n, uint64_t seed, uint64_t ctr, uint8_t *__restrict__ dst) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const uint8_t *x = src + (size_t)min(max(src_row[s], 0), n_src - 1) * V;
    uint8_t *y = dst + (size_t)s * V;
    for (int v = 0; v < V; ++v) y[v] = x[v];
    for (int i = 0; i < n; ++i) {
        const int j = V - n + i;
        const uint4 q = philox4x32_10(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)s, (uint32_t)i),
                                      (uint32_t)seed, (uint32_t)(seed >> 32));
        const int t = (int)mulhi32(q.x, (uint32_t)j + 1u);
        const int pick = y[t] != x[t] ? j : t;
        MSAT_DCHECK(pick, V);
        y[pick] = x[pick] ^ 1u;
    }
}

}  // namespace msat

using namespace msat;

extern "C" int msat_bc_greedy_labels(const msat_env_desc *desc, const uint16_t *lits, const int32_t *problem_idx,
                                     const uint8_t *assign, float tau, int32_t *labels, int32_t *deltas,
                                     void *stream) {
    EnvParams p;
    int rc = make_params(desc, &p);
    if (rc) return rc;
    if (p.B == 0) return MSAT_OK;
    MSAT_REQUIRE(lits && problem_idx && assign && labels, "NULL pointer");
    const size_t lds = ((size_t)p.WV + p.V) * 4;
    MSAT_REQUIRE(lds <= 160 * 1024, "bc labels need %zu B of LDS", lds);
    hipLaunchKernelGGL(bc_labels_kernel, dim3(p.B), dim3(kThreads), lds, (hipStream_t)stream, p, lits, problem_idx,
                       assign, tau, labels, deltas);
    return check_launch("bc_labels_kernel");
}

extern "C" int msat_bc_corrupt(const uint8_t *src, int32_t n_src, const int32_t *src_row, int32_t S, int32_t V,
                               int32_t level, uint64_t seed, uint64_t counter, uint8_t *dst, void *stream) {
    MSAT_REQUIRE(S >= 0, "bc_corrupt: S %d < 0", S);
    MSAT_REQUIRE(V >= 1, "bc_corrupt: V %d < 1", V);
    MSAT_REQUIRE(level >= 0, "bc_corrupt: level %d < 0", level);
    MSAT_REQUIRE(n_src >= 1, "bc_corrupt: n_src %d < 1", n_src);
    if (S == 0) return MSAT_OK;
    MSAT_REQUIRE(src && src_row && dst, "bc_corrupt: NULL pointer");
    hipLaunchKernelGGL(bc_corrupt_kernel, dim3((S + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, n_src,
                       src_row, S, V, std::min(level, V), seed, counter, dst);
    return check_launch("bc_corrupt_kernel");
}
