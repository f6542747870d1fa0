// msat_pool_generate: a pool of planted random k-SAT instances drawn on the device (include/marlsat.h).  Cold:
// once per pool (a training run that refreshes its pool calls it every few updates), never in the env step.
// The arithmetic of every stored word is csrc/pool_gen.h, shared with the host check.
#include "common.h"
#include "pool_gen.h"

namespace msat {

constexpr int kPgThreads = 256;

// One workgroup per instance.  LDS: the hidden words (HB * 4) and one occurrence bit per variable (WV words;
// a bit, not a count: the rule only asks whether a variable occurs).  An attempt writes its hidden bytes and
// its clauses straight to the outputs with plain vector stores, every word by the same lane in every attempt,
// so a rejected attempt is simply overwritten by the next and the last attempt is what stays.
__global__ void __launch_bounds__(kPgThreads)
pool_generate_kernel(int V, int C, int K, uint64_t seed, uint64_t ctr, int reject, int max_attempts,
                     int32_t *__restrict__ clauses, uint8_t *__restrict__ planted, int32_t *__restrict__ attempts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pg_smem[];
    const int HB = pg_hidden_blocks(V), WV = (V + 31) / 32;
    uint32_t *hidden = pg_smem;        // [HB * 4]
    uint32_t *occ = pg_smem + HB * 4;  // [WV]
    const int n = blockIdx.x, tid = threadIdx.x;
    int32_t *cl = clauses + (size_t)n * C * K;
    uint8_t *pl = planted + (size_t)n * V;
    const int tries = reject ? max_attempts : 1;
    int accepted = -1;
    for (int a = 0; a < tries; ++a) {
        for (int b = tid; b < HB; b += kPgThreads) {
            const PgWords w = pg_block(seed, ctr, (uint32_t)n, (uint32_t)a, (uint32_t)b);
            for (int k = 0; k < 4; ++k) hidden[4 * b + k] = w.q[k];
        }
        for (int w = tid; w < WV; w += kPgThreads) occ[w] = 0u;
        __syncthreads();
        for (int v = tid; v < V; v += kPgThreads) pl[v] = (uint8_t)((hidden[v >> 5] >> (v & 31)) & 1u);
        for (int c = tid; c < C; c += kPgThreads) {
            const PgWords w = pg_block(seed, ctr, (uint32_t)n, (uint32_t)a, (uint32_t)(HB + c));
            int32_t lits[kPgMaxWidth];
            pg_clause(w, hidden, V, K, lits);
            for (int k = 0; k < K; ++k) {
                const int v = (lits[k] < 0 ? -lits[k] : lits[k]) - 1;
                MSAT_DCHECK(v, V);
                atomicOr(&occ[v >> 5], 1u << (v & 31));
                cl[(size_t)c * K + k] = lits[k];
            }
        }
        __syncthreads();
        int missing = 0;
        if (reject)
            for (int w = tid; w < WV; w += kPgThreads) {
                const int bits = min(32, V - 32 * w);
                const uint32_t full = bits == 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
                missing |= (occ[w] != full);
            }
        // a barrier as well: every lane has read occ and hidden before the next attempt rewrites them
        if (!__syncthreads_or(missing)) {
            accepted = a;
            break;
        }
    }
    if (tid == 0) attempts[n] = accepted;
}

}  // namespace msat

using namespace msat;

extern "C" int msat_pool_generate(int32_t num_problems, int32_t num_vars, int32_t num_clauses, int32_t clause_width,
                                  uint64_t seed, uint64_t counter, int32_t reject_isolated, int32_t max_attempts,
                                  int32_t *clauses, uint8_t *planted, int32_t *attempts, void *stream) {
    MSAT_REQUIRE(num_problems >= 0, "pool_generate: num_problems %d < 0", num_problems);
    MSAT_REQUIRE(num_vars >= 1 && num_vars <= 32000, "pool_generate: num_vars %d outside [1, 32000]", num_vars);
    MSAT_REQUIRE(num_clauses >= 1, "pool_generate: num_clauses %d < 1", num_clauses);
    MSAT_REQUIRE(clause_width >= 1 && clause_width <= kPgMaxWidth, "pool_generate: clause_width %d outside [1, %d]",
                 clause_width, kPgMaxWidth);
    MSAT_REQUIRE(clause_width <= num_vars, "pool_generate: clause_width %d > num_vars %d (distinct variables)",
                 clause_width, num_vars);
    MSAT_REQUIRE((uint64_t)pg_hidden_blocks(num_vars) + (uint64_t)num_clauses < (uint64_t)kPgMaxBlocks,
                 "pool_generate: %d hidden blocks + %d clauses do not fit the 24-bit block index",
                 pg_hidden_blocks(num_vars), num_clauses);
    MSAT_REQUIRE(max_attempts >= 1 && max_attempts <= kPgMaxAttempts, "pool_generate: max_attempts %d outside [1, %d]",
                 max_attempts, kPgMaxAttempts);
    MSAT_REQUIRE(!reject_isolated || (int64_t)clause_width * num_clauses >= num_vars,
                 "pool_generate: reject_isolated with %d x %d literal slots < %d variables can never be accepted",
                 num_clauses, clause_width, num_vars);
    if (num_problems == 0) return MSAT_OK;
    MSAT_REQUIRE(clauses && planted && attempts, "pool_generate: NULL pointer");
    const size_t lds = ((size_t)pg_hidden_blocks(num_vars) * 4 + (size_t)(num_vars + 31) / 32) * 4;
    hipLaunchKernelGGL(pool_generate_kernel, dim3(num_problems), dim3(kPgThreads), lds, (hipStream_t)stream, num_vars,
                       num_clauses, clause_width, seed, counter, reject_isolated != 0, max_attempts, clauses, planted,
                       attempts);
    return check_launch("pool_generate_kernel");
}
