// Assignment predictor (src/learners/bc_learner.py, src/runners/bc_runner.py): the per-variable two-class
// cross-entropy over a (S*V, 2) logit matrix, its gradient, the arg-max assignment and whether that assignment
// satisfies the sample's formula, in one pass.  Enqueue-only; the sums are fp64 in a fixed order (bitwise
// reproducible), no floating-point atomics, one writer per output word.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "marlsat_net.h"

namespace msat {

constexpr int kAlWaves = 4;        // samples per workgroup pass, one wave each
constexpr int kAlWords = 512;      // ballot words per wave: 32768 bits, so every code below MSAT_LIT_ABSENT indexes
                                   // inside the wave's own slice whatever the pool holds (V <= 32000 needs 500)
constexpr int kAlSumT = 1024;      // the sums kernel's one workgroup

struct AssignArgs {
    const float *logits;
    int S, V;
    const uint8_t *labels;  // NULL: predict only
    double denom;           // minibatch * V
    const uint16_t *lits;
    int N, C;
    const int32_t *problem_idx;
    float *dlogits;
    uint8_t *pred;
    float *sample_nll;
    int32_t *sample_correct;
    int32_t *sample_unsat;
    uint8_t *sample_solved;
};

// -log p[label] of a two-class softmax from d = l[label] - l[1 - label]: softplus(-d), the form that neither
// overflows nor cancels.  Both kernels below call it, so the sums are sums of the very values the rows report.
__device__ __forceinline__ double two_class_nll(double d) { return fmax(-d, 0.0) + log1p(exp(-fabs(d))); }

// p[1 - label] = 1 / (1 + exp(d)) with the exponential taken of -|d|
__device__ __forceinline__ double two_class_p_other(double d) {
    const double e = exp(-fabs(d));
    return d >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
}

__device__ __forceinline__ bool row_valid(unsigned lab, float l0, float l1) {
    return lab <= 1u && isfinite(l0) && isfinite(l1);
}

// One wave per sample.  Pass 1, lanes stride the V rows: prediction (stored, and kept as ballot words in the wave's
// LDS slice), nll, gradient, correct count.  Pass 2, lanes stride the C clauses of the sample's instance: one
// 8-byte load of the four codes, truth from the ballot words, the wave adds the false clauses.  The trip count of
// the outer loop is the same for the four waves of a workgroup (the barriers are workgroup-wide).
__global__ void __launch_bounds__(64 * kAlWaves)
assign_loss_kernel(AssignArgs a) {
    __shared__ unsigned long long s_bits[kAlWaves][kAlWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *bits = s_bits[wave];
    const int V = a.V, C = a.C;
    for (int s0 = blockIdx.x * kAlWaves; s0 < a.S; s0 += gridDim.x * kAlWaves) {
        const int s = s0 + wave;
        const bool live = s < a.S;  // wave-uniform
        if (live) {
            const size_t row0 = (size_t)s * V;
            double nll = 0.0;
            int correct = 0;
            for (int j0 = 0; j0 < V; j0 += 64) {
                const int j = j0 + lane;
                const bool in = j < V;
                float l0 = 0.f, l1 = 0.f;
                if (in) {
                    l0 = a.logits[2 * (row0 + j)];
                    l1 = a.logits[2 * (row0 + j) + 1];
                }
                const bool p = in && l1 > l0;  // a tie and a NaN give 0
                const unsigned long long word = __ballot(p);
                if (lane == 0) bits[j0 >> 6] = word;
                if (!in) continue;
                a.pred[row0 + j] = p ? 1 : 0;
                if (!a.labels) continue;
                const unsigned lab = a.labels[row0 + j];
                float g = 0.f;
                const bool valid = row_valid(lab, l0, l1);
                if (valid) {
                    const double d = lab ? (double)l1 - (double)l0 : (double)l0 - (double)l1;
                    nll += two_class_nll(d);
                    g = (float)(two_class_p_other(d) / a.denom);
                    correct += (p ? 1u : 0u) == lab;
                }
                // the same magnitude with opposite signs: the row sums to exactly 0
                a.dlogits[2 * (row0 + j) + lab % 2u] = valid ? -g : 0.f;
                a.dlogits[2 * (row0 + j) + 1 - lab % 2u] = g;
            }
            if (a.labels) {
                nll = wave_sum_f64(nll);
                correct = wave_sum_i32(correct);
                if (lane == 0) {
                    a.sample_nll[s] = (float)nll;
                    a.sample_correct[s] = correct;
                }
            }
        }
        __syncthreads();  // the ballot words are in LDS
        if (live) {
            const int p = std::min(std::max(a.problem_idx[s], 0), a.N - 1);
            const uint2 *row = reinterpret_cast<const uint2 *>(a.lits + (size_t)p * C * MSAT_LIT_SLOTS);
            int unsat = 0;
            for (int c = lane; c < C; c += 64) {
                const uint2 w = row[c];
                const unsigned code[MSAT_LIT_SLOTS] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16};
                bool sat = false;
#pragma unroll
                for (int k = 0; k < MSAT_LIT_SLOTS; ++k) {
                    const unsigned cd = code[k];
                    if (cd >= MSAT_LIT_ABSENT) continue;  // ABSENT is inert, NULL is false
                    const unsigned v = cd >> 1;           // < 32768 = 64 * kAlWords
                    const unsigned x = (unsigned)(bits[v >> 6] >> (v & 63u)) & 1u;
                    sat |= ((x ^ cd) & 1u) != 0;
                }
                unsat += sat ? 0 : 1;
            }
            unsat = wave_sum_i32(unsat);
            if (lane == 0) {
                a.sample_unsat[s] = unsat;
                a.sample_solved[s] = unsat == 0 ? 1 : 0;
            }
        }
        __syncthreads();  // before the next sample's words replace these
    }
}

// sums[0..4] += (sum nll, sum correct, valid rows, invalid rows, solved samples): one workgroup, wave w takes the
// samples w, w + 16, ..., its lanes stride their rows in order, then the wave butterfly and the sixteen wave sums
// in order.  The nll terms are evaluated again from the logits (the per-sample outputs are fp32, the sum is of the
// fp64 terms); the four counts are whole numbers below 2^53, exact in any order.  labels NULL: sums[4] only.
__global__ void __launch_bounds__(kAlSumT)
assign_sums_kernel(AssignArgs a, double *__restrict__ sums) {
    __shared__ double red[5][kAlSumT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.labels) {
        for (int s = wave; s < a.S; s += kAlSumT / 64) {
            const size_t row0 = (size_t)s * a.V;
            for (int j = lane; j < a.V; j += 64) {
                const float l0 = a.logits[2 * (row0 + j)], l1 = a.logits[2 * (row0 + j) + 1];
                const unsigned lab = a.labels[row0 + j];
                if (row_valid(lab, l0, l1)) {
                    acc[0] += two_class_nll(lab ? (double)l1 - (double)l0 : (double)l0 - (double)l1);
                    acc[2] += 1.0;
                } else {
                    acc[3] += 1.0;
                }
            }
        }
    }
    for (int s = threadIdx.x; s < a.S; s += kAlSumT) {
        if (a.labels) acc[1] += (double)a.sample_correct[s];
        acc[4] += a.sample_solved[s] ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double t = wave_sum_f64(acc[k]);
        if (lane == 0) red[k][wave] = t;
    }
    __syncthreads();
    if (threadIdx.x < 5 && (a.labels || threadIdx.x == 4)) {
        double t = 0.0;
        for (int w = 0; w < kAlSumT / 64; ++w) t += red[threadIdx.x][w];
        sums[threadIdx.x] += t;
    }
}

}  // namespace msat

using namespace msat;

extern "C" int msat_assign_loss(const float *logits, int32_t S, int32_t V, const uint8_t *labels, int32_t minibatch,
                                const uint16_t *lits, int32_t num_problems, int32_t num_clauses,
                                const int32_t *problem_idx, float *dlogits, uint8_t *pred, float *sample_nll,
                                int32_t *sample_correct, int32_t *sample_unsat, uint8_t *sample_solved, double *sums,
                                void *stream) {
    MSAT_REQUIRE(S >= 0, "assign_loss: S %d < 0", S);
    MSAT_REQUIRE(V >= 1 && V <= 32000, "assign_loss: V %d outside [1, 32000]", V);
    MSAT_REQUIRE(num_clauses >= 1, "assign_loss: num_clauses %d < 1", num_clauses);
    MSAT_REQUIRE(num_problems >= 1, "assign_loss: num_problems %d < 1", num_problems);
    MSAT_REQUIRE(minibatch >= 1, "assign_loss: minibatch %d < 1", minibatch);
    MSAT_REQUIRE((labels != nullptr) == (dlogits != nullptr),
                 "assign_loss: labels and dlogits go together (both set, or both NULL to predict only)");
    if (!S) return MSAT_OK;
    MSAT_REQUIRE(logits && lits && problem_idx && pred && sample_unsat && sample_solved, "assign_loss: NULL pointer");
    MSAT_REQUIRE(!labels || (sample_nll && sample_correct && sums),
                 "assign_loss: NULL sample_nll, sample_correct or sums with labels set");
    AssignArgs a;
    a.logits = logits;
    a.S = S;
    a.V = V;
    a.labels = labels;
    a.denom = (double)minibatch * (double)V;
    a.lits = lits;
    a.N = num_problems;
    a.C = num_clauses;
    a.problem_idx = problem_idx;
    a.dlogits = dlogits;
    a.pred = pred;
    a.sample_nll = sample_nll;
    a.sample_correct = sample_correct;
    a.sample_unsat = sample_unsat;
    a.sample_solved = sample_solved;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(assign_loss_kernel, dim3(std::min(8192, (S + kAlWaves - 1) / kAlWaves)), dim3(64 * kAlWaves), 0,
                       st, a);
    int rc = check_launch("assign_loss_kernel");
    if (rc || !sums) return rc;
    hipLaunchKernelGGL(assign_sums_kernel, dim3(1), dim3(kAlSumT), 0, st, a, sums);
    return check_launch("assign_sums_kernel");
}
