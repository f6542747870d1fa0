// Single-agent PPO baseline on the device (src/learners/single_rl_learner.py, src/runners/single_rl_runner.py):
// the loss over a (S, V) logit batch, the per-minibatch population standardisation of the advantages, the
// optimiser chain's clip_by_global_norm and the bookkeeping of a greedy evaluation episode.  Everything here is
// enqueue-only; the sums are fp64 in a fixed order (bitwise reproducible), no floating-point atomics.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "marlsat_net.h"

namespace msat {

// ------------------------------------------------------------------- loss ----
struct SingleCfg {
    double lo, hi;      // 1 - clip_eps, 1 + clip_eps (the fp32 clip_eps widened)
    double ent_coef, vf_coef;
    double inv_n;       // 1 / minibatch
};

// d/dr jnp.clip(r, lo, hi) = min(max(r, lo), hi) with balanced ties (heads_kernels.hip clip_grad, in fp64)
__device__ __forceinline__ double clip_grad_f64(double r, double lo, double hi) {
    const double a = r > lo ? 1.0 : (r == lo ? 0.5 : 0.0);
    return r < hi ? a : (r == hi ? 0.5 * a : 0.0);
}

// One wave per row of width V (single_rl_learner.py:118-158).  The row's softmax, entropy and ratio in fp64, each
// output rounded to fp32 once (as bc_loss_kernel).  The sum of exponentials leaves the row maximum's own 1 out
// (log1p of the rest): a dominant logit keeps its small entropy and its 1 - p to fp64 rounding.
// A row whose action is outside [0, V) gets zeros throughout and reads nothing but its action.
__global__ void __launch_bounds__(256)
single_loss_kernel(const float *__restrict__ logits, int S, int V, const int32_t *__restrict__ action,
                   const float *__restrict__ old_logp, const float *__restrict__ adv, const float *__restrict__ value,
                   const float *__restrict__ targets, SingleCfg cfg, float *__restrict__ dlogits,
                   float *__restrict__ dvalue, float *__restrict__ row_terms) {
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < S; r += gridDim.x * 4) {
        const float *lg = logits + (size_t)r * V;
        float *dl = dlogits + (size_t)r * V;
        float *rt = row_terms + 3 * (size_t)r;
        const int a = action[r];
        if (a < 0 || a >= V) {  // wave-uniform
            for (int j = lane; j < V; j += 64) dl[j] = 0.f;
            if (lane == 0) {
                dvalue[r] = 0.f;
                rt[0] = rt[1] = rt[2] = 0.f;
            }
            continue;
        }
        // the row maximum and its lowest index
        float best = -INFINITY;
        int bi = 0x7FFFFFFF;
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            if (v > best || (v == best && j < bi)) {
                best = v;
                bi = j;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) {
                best = ob;
                bi = oi;
            }
        }
        const double m = (double)best;
        double rest = 0.0;  // sum of exp(l - m) over every slot but the maximum's
        for (int j = lane; j < V; j += 64) rest += j == bi ? 0.0 : exp((double)lg[j] - m);
        rest = wave_sum_f64(rest);
        const double sum = 1.0 + rest, lse = log1p(rest);
        double h = 0.0, others = 0.0;  // -sum p log p; sum of p over every slot but the action's
        for (int j = lane; j < V; j += 64) {
            const double z = (double)lg[j] - m;
            const double p = (j == bi ? 1.0 : exp(z)) / sum;
            h -= p * (z - lse);  // p = 0 (underflow) times a finite log-prob: 0
            others += j == a ? 0.0 : p;
        }
        h = wave_sum_f64(h);
        others = wave_sum_f64(others);
        const double lpa = ((double)lg[a] - m) - lse;
        const double ratio = exp(lpa - (double)old_logp[r]);
        const double g = (double)adv[r];
        const double c = fmin(fmax(ratio, cfg.lo), cfg.hi);
        const double u = ratio * g, v = c * g;
        const double du = g, dv = g * clip_grad_f64(ratio, cfg.lo, cfg.hi);
        const double dmin = u < v ? du : (v < u ? dv : 0.5 * (du + dv));  // jnp.minimum: ties 0.5 / 0.5
        const double dlpa = -dmin * ratio * cfg.inv_n;
        const double dh = cfg.ent_coef * cfg.inv_n;  // d total / d (-H) per row
        for (int j = lane; j < V; j += 64) {
            const double z = (double)lg[j] - m;
            const double p = (j == bi ? 1.0 : exp(z)) / sum;
            const double onehot_minus_p = j == a ? others : -p;
            dl[j] = (float)(dlpa * onehot_minus_p + dh * (p * ((z - lse) + h)));
        }
        if (lane == 0) {
            const double d = (double)value[r] - (double)targets[r];
            dvalue[r] = (float)(cfg.vf_coef * 2.0 * d * cfg.inv_n);
            rt[0] = (float)(-fmin(u, v));
            rt[1] = (float)(d * d);
            rt[2] = (float)h;
        }
    }
}

// sums[0..3] += (sum actor, sum vl, sum ent, invalid rows) over the fp32 row terms, fp64, fixed order
__global__ void __launch_bounds__(256)
single_sums_kernel(const float *__restrict__ row_terms, int S, int V, const int32_t *__restrict__ action,
                   double *__restrict__ sums) {
    __shared__ double red[4][256];
    double a = 0, v = 0, e = 0, ni = 0;
    for (int r = threadIdx.x; r < S; r += 256) {
        a += row_terms[3 * (size_t)r];
        v += row_terms[3 * (size_t)r + 1];
        e += row_terms[3 * (size_t)r + 2];
        const int ac = action[r];
        ni += (ac < 0 || ac >= V) ? 1.0 : 0.0;
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = v;
    red[2][threadIdx.x] = e;
    red[3][threadIdx.x] = ni;
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = 0;
        for (int k = 0; k < 256; ++k) t += red[threadIdx.x][k];
        sums[threadIdx.x] += t;
    }
}

// ------------------------------------------------ population standardisation ----
// x = (x - mean) / (std + 1e-8), mean = m[0] / n, std = sqrt(max(m[1] / n - mean^2, 0)) from msat_moments'
// device sums; fp64 per element, rounded once.  (A constant fp32 vector sums exactly in fp64, so its mean is the
// constant and every element becomes 0 whatever the variance's rounding leaves.)
constexpr int kEwT = 256;

__global__ void __launch_bounds__(kEwT)
standardize_pop_kernel(float *__restrict__ x, size_t n, const double *__restrict__ moments2) {
    const double mean = moments2[0] / (double)n;
    const double var = fmax(moments2[1] / (double)n - mean * mean, 0.0);
    const double den = sqrt(var) + 1e-8;
    for (size_t i = (size_t)blockIdx.x * kEwT + threadIdx.x; i < n; i += (size_t)gridDim.x * kEwT)
        x[i] = (float)(((double)x[i] - mean) / den);
}

// ------------------------------------------------------- clip_by_global_norm ----
// Stage 1: part[block] = sum of g^2 over the block's grid-stride elements, fp64: lane sums, wave butterfly, the
// four wave sums in order.
__global__ void __launch_bounds__(kEwT)
sumsq_kernel(const float *__restrict__ g, size_t n, double *__restrict__ part) {
    __shared__ double ws[kEwT / 64];
    double a = 0.0;
    for (size_t i = (size_t)blockIdx.x * kEwT + threadIdx.x; i < n; i += (size_t)gridDim.x * kEwT) {
        const double v = (double)g[i];
        a += v * v;
    }
    a = wave_sum_f64(a);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// Stage 2: every workgroup adds the nb partials in the same order (its first wave: lane-strided sums, butterfly),
// so all of them hold the same norm; norm < max_norm leaves the gradient untouched, otherwise
// g *= (float)(max_norm / norm).  A NaN norm compares false and scales every element to NaN.
__global__ void __launch_bounds__(kEwT)
clip_scale_kernel(float *__restrict__ g, size_t n, float max_norm, const double *__restrict__ part, int nb,
                  float *__restrict__ norm_out) {
    __shared__ double s_norm;
    if (threadIdx.x < 64) {
        double a = 0.0;
        for (int k = threadIdx.x; k < nb; k += 64) a += part[k];
        a = wave_sum_f64(a);
        if (threadIdx.x == 0) s_norm = sqrt(a);
    }
    __syncthreads();
    const double norm = s_norm;
    if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)norm;
    if (norm < (double)max_norm) return;
    const float scale = (float)((double)max_norm / norm);
    for (size_t i = (size_t)blockIdx.x * kEwT + threadIdx.x; i < n; i += (size_t)gridDim.x * kEwT) g[i] = g[i] * scale;
}

// ------------------------------------------------------------ episode track ----
// single_rl_runner.py:218-229 without auto-reset: until an env's first done its return accumulates (fp32, step
// order); the first done fixes its length, its solved flag and finished = 1.
__global__ void episode_track_kernel(int B, int t, const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                     const uint8_t *__restrict__ solved, float *__restrict__ ret,
                                     int32_t *__restrict__ len, uint8_t *__restrict__ ep_solved,
                                     uint8_t *__restrict__ finished) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || finished[b]) return;
    ret[b] = ret[b] + reward[b];
    if (done[b]) {
        len[b] = t + 1;
        ep_solved[b] = solved[b] ? 1 : 0;
        finished[b] = 1;
    }
}

static int ew_blocks(size_t n) { return (int)std::min<size_t>((n + kEwT - 1) / kEwT, 1024); }

}  // namespace msat

using namespace msat;

extern "C" int msat_ppo_single_loss(const float *logits, int32_t S, int32_t V, const int32_t *action,
                                    const float *old_logp, const float *adv_n, const float *value,
                                    const float *targets, float clip_eps, float ent_coef, float vf_coef,
                                    int32_t minibatch, float *dlogits, float *dvalue, float *row_terms, double *sums,
                                    void *stream) {
    MSAT_REQUIRE(S >= 0, "ppo_single_loss: S %d < 0", S);
    MSAT_REQUIRE(V >= 1, "ppo_single_loss: V %d < 1", V);
    MSAT_REQUIRE(minibatch >= 1, "ppo_single_loss: minibatch %d < 1", minibatch);
    MSAT_REQUIRE(std::isfinite(clip_eps) && clip_eps > 0.f, "ppo_single_loss: clip_eps %g must be finite and > 0",
                 (double)clip_eps);
    if (!S) return MSAT_OK;
    MSAT_REQUIRE(logits && action && old_logp && adv_n && value && targets && dlogits && dvalue && row_terms && sums,
                 "ppo_single_loss: NULL pointer");
    SingleCfg c;
    c.lo = 1.0 - (double)clip_eps;
    c.hi = 1.0 + (double)clip_eps;
    c.ent_coef = (double)ent_coef;
    c.vf_coef = (double)vf_coef;
    c.inv_n = 1.0 / (double)minibatch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(single_loss_kernel, dim3(std::min(8192, (S + 3) / 4)), dim3(256), 0, s, logits, S, V, action,
                       old_logp, adv_n, value, targets, c, dlogits, dvalue, row_terms);
    int rc = check_launch("single_loss_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(single_sums_kernel, dim3(1), dim3(256), 0, s, row_terms, S, V, action, sums);
    return check_launch("single_sums_kernel");
}

extern "C" int msat_standardize_pop(float *x, size_t n, const double *moments2, void *stream) {
    if (!n) return MSAT_OK;
    MSAT_REQUIRE(x && moments2, "standardize_pop: NULL pointer");
    hipLaunchKernelGGL(standardize_pop_kernel, dim3(ew_blocks(n)), dim3(kEwT), 0, (hipStream_t)stream, x, n, moments2);
    return check_launch("standardize_pop_kernel");
}

extern "C" size_t msat_clip_global_norm_workspace_doubles(size_t n) { return (size_t)std::max(1, ew_blocks(n)); }

extern "C" int msat_clip_global_norm(float *grads, size_t n, float max_norm, double *workspace, float *norm_out,
                                     void *stream) {
    MSAT_REQUIRE(std::isfinite(max_norm) && max_norm > 0.f, "clip_global_norm: max_norm %g must be finite and > 0",
                 (double)max_norm);
    MSAT_REQUIRE(workspace && norm_out, "clip_global_norm: NULL workspace or norm_out");
    if (!n) return MSAT_OK;
    MSAT_REQUIRE(grads, "clip_global_norm: NULL gradient");
    const int nb = ew_blocks(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(kEwT), 0, s, grads, n, workspace);
    int rc = check_launch("sumsq_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(clip_scale_kernel, dim3(nb), dim3(kEwT), 0, s, grads, n, max_norm, workspace, nb, norm_out);
    return check_launch("clip_scale_kernel");
}

extern "C" int msat_episode_track(int32_t B, int32_t t, const float *reward, const uint8_t *done,
                                  const uint8_t *solved, float *ret, int32_t *len, uint8_t *ep_solved,
                                  uint8_t *finished, void *stream) {
    MSAT_REQUIRE(B >= 0, "episode_track: B %d < 0", B);
    MSAT_REQUIRE(t >= 0 && t < INT_MAX, "episode_track: step index %d outside [0, INT_MAX)", t);
    if (!B) return MSAT_OK;
    MSAT_REQUIRE(reward && done && solved && ret && len && ep_solved && finished, "episode_track: NULL pointer");
    hipLaunchKernelGGL(episode_track_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, t, reward,
                       done, solved, ret, len, ep_solved, finished);
    return check_launch("episode_track_kernel");
}
