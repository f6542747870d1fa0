// Batched multi-agent SAT environment on gfx950.
//
// One workgroup (64 .. 512 lanes by instance and batch size: env_threads, env_delta_threads for a launch with an obs
// shadow) owns one environment for the whole call:
//   1. assignment -> LDS bit words (one ballot per 64 vars), agents' flips as
//      LDS atomic XORs;
//   2. every clause evaluated once from the L2/MALL-resident packed pool
//      (8 B/clause), clause status -> LDS bit words by wave ballot, the
//      unsatisfied count by popcount of the same ballots;
//   3. done / reward / info, and (auto-reset) an in-place reset of done envs;
//   4. the instance's agent tables (relation + neighbour bits, built once per
//      pool instance) staged into LDS;
//   5. the env's (A, 2V+C) observation block streamed to HBM with 16 B stores,
//      every 4-element chunk assembled from two LDS words by bit extraction.
// The observation write is >90 % of a step's algorithmic bytes (SURVEY.md
// §8(d)); everything before it is sized to keep the obs pass a pure
// LDS-read -> 16 B store stream.
//
// Reference semantics (kongqg/marl-sat, src/envs/multi_agent_sat_env.py):
//   flip decode             :230-250
//   clause evaluation       :130-156   (literal l true iff l>0&&x=1 or l<0&&x=0)
//   done / reward / info    :256-284, :183-198 (sparse) / :201-223 (PBRS)
//   reset + masks           :158-181, :99-128
//   get_obs                 :345-398
//   rollout auto-reset      src/learners/mappo_gnn_sat_learner.py:422-464
//
// This file holds the step / reset / obs kernel family, its launchers and its entry points, and nothing else: the
// cold kernels around the env live in env_tables.hip and bc_data.hip and share env_params.h with it.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "env_params.h"
#include "obs_sparse.h"

namespace msat {

// Obs shadow (msat_env_step_delta), an argument of shadow::env_kernel alone: per env, what the obs buffer holds --
// [problem_idx or -1 | x bit words | clause-sat bit words] (shadow_row_words).  With it a step stores only the obs
// groups (g aligned bytes: 16 / 64 / 128; 0: whole blocks) in which the image of the shadow row and the image of the
// new state differ.  EnvParams, and with it every kernel of a launch without a shadow, is what it was without it.
struct ObsShadowArg {
    uint32_t *rows;
    int g;
};

enum : int { kModeReset = 0, kModeStep = 1, kModeStepAutoReset = 2, kModeObs = 3 };

// Reset queue (msat_env_state.reset_queue): pend[2][B] uint32 tokens.  The launch with serial s reads parity s & 1 --
// env b timed out now iff pend[s & 1][b] == rq_token(s), written by the previous launch -- and writes every entry of
// parity (s + 1) & 1 (rq_token(s + 1) for an env whose next step times out, else 0): never the same words within a
// launch.  The reset workgroups of launch s take the pending envs in index order: workgroup j the one of rank j,
// the env of rank r is covered iff r < cap (the others reset in their step workgroup).  Ranks come from a scan of
// the pending words (one round trip), so no counter, list or atomic is involved: a launch in which every env times
// out (a batch reset together, every max_steps launches) costs each env one scan of B words from L2.  Tokens have
// bit 31 set, so a zeroed queue lists nothing.
__host__ __device__ __forceinline__ uint32_t rq_token(uint32_t serial) { return 0x80000000u | (serial & 0x7FFFFFFFu); }
// ~B/512 envs time out per launch; a multiple of 8, so the reset workgroups (launched first) leave the step workgroups
// XCD placement as without them
__host__ __device__ __forceinline__ int rq_capacity(int B) { return (B / 256 + 8 + 7) & ~7; }
__host__ __device__ __forceinline__ size_t rq_words(int B) { return 2 * (size_t)B; }

__device__ __forceinline__ uint32_t *rq_pend(uint32_t *q, int B, int par) { return q + (size_t)par * B; }

// Wave 0 (all 64 lanes, uniform arguments) scans pend[0 .. B): lane l owns the contiguous words [W l, W l + W),
// W = ceil(B / 64) rounded up to 4 (16-byte loads).  Returns, in every lane, the number of entries equal to tok
// with index < lim; with want >= 0 also the index of the entry of rank want (-1 if fewer), in *sel.  Each lane keeps
// its matches as a bit mask (W <= 64, i.e. B <= 4096), so the selection needs no second read; larger batches
// re-read the owning lane's range.
__device__ __forceinline__ int rq_scan(const uint32_t *__restrict__ pend, int B, uint32_t tok, int lim, int want,
                                       int *sel) {
    const int lane = threadIdx.x & 63;
    const int W = ((B + 63) / 64 + 3) & ~3;
    const int lo = lane * W;
    int below = 0, mine = 0;
    uint64_t bits = 0;
    for (int i = 0; i < W; i += 4) {
        const int k = lo + i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (k < B) v = *reinterpret_cast<const uint4 *>(pend + k);  // B % 4 == 0 (host-checked)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool m = k + u < B && w[u] == tok;
            mine += m;
            below += m && k + u < lim;
            if (m && i + u < 64) bits |= 1ull << (i + u);
        }
    }
    int total_below = below;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) total_below += __shfl_xor(total_below, d, 64);
    if (want >= 0) {
        int incl = mine;  // inclusive prefix of mine over the lanes (index order), Hillis-Steele by shuffles
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const int excl = incl - mine;
        int found = -1;
        if (want >= excl && want < incl) {  // the rank-want entry is in this lane's range
            int r = want - excl;            // its rank among this lane's matches
            if (W <= 64) {
                uint64_t m = bits;
                for (; r > 0; --r) m &= m - 1;
                found = lo + __ffsll((unsigned long long)m) - 1;
            } else {
                for (int i = 0; i < W && found < 0; i += 4) {
                    const int k = lo + i;
                    if (k >= B) break;
                    const uint4 v = *reinterpret_cast<const uint4 *>(pend + k);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    for (int u = 0; u < 4 && found < 0; ++u)
                        if (k + u < B && w[u] == tok && r-- == 0) found = k + u;
                }
            }
        }
        const uint64_t has = __ballot(found >= 0);
        *sel = has ? __shfl(found, __ffsll((unsigned long long)has) - 1, 64) : -1;
    }
    return total_below;
}

// LDS image of one environment (all uint32 words).
struct EnvLds {
    uint32_t *x;    // [WV]    assignment bits
    uint32_t *sat;  // [WC]    clause-satisfied bits
    uint32_t *rel;  // [A*WC]  agent-clause relation bits of the env's instance
    uint32_t *nbr;  // [A*WV]  agent neighbour bits of the env's instance
    uint32_t *fm;   // [NW]    obs image: element is not -1   (NW = A*D/32 + 2)
    uint32_t *fx;   // [NW]    obs image: element value bit
    int *red;       // [16]    reduction / broadcast scratch
    // only in a launch with an obs shadow (carve<true>):
    uint32_t *fd;    // [NW+1] obs image: element differs from what the obs buffer holds (follows fx; G = 64 / 128).
                     //        A G = 16 delta step builds no images and leaves fm, fx, fd alone
    uint32_t *sx;    // [WV]   the shadow row's assignment bits
    uint32_t *ssat;  // [WC]   the shadow row's clause-satisfied bits
    uint16_t *own;   // [V]    agent_of_var (follows red): whose rows a changed element lies in (scatter_obs)
};

__host__ __device__ __forceinline__ int obs_image_words(const EnvParams &p) { return (p.A * p.D) / 32 + 2; }

// uint32 words of an env's obs shadow row: problem_idx, ceil(V/32) assignment words, ceil(C/32) clause words
__host__ __device__ __forceinline__ int shadow_row_words(const EnvParams &p) {
    return 1 + ((p.V + 31) >> 5) + ((p.C + 31) >> 5);
}

// a launch with a shadow (sh) carries the third obs image (fd), the shadow row's bit words (sx, ssat) and the
// variables' owners (own: V 16-bit entries) as well
__host__ __device__ __forceinline__ size_t env_lds_words(const EnvParams &p, bool sh = false) {
    return (size_t)p.WV + p.WC + (size_t)p.A * (p.WC + p.WV) + 2 * (size_t)obs_image_words(p) + 16 +
           (sh ? (size_t)obs_image_words(p) + 1 + p.WV + p.WC + (p.V + 1) / 2 : 0);
}

template <bool SH = false>
__device__ __forceinline__ EnvLds carve(uint32_t *smem, const EnvParams &p) {
    EnvLds l;
    l.x = smem;
    l.sat = l.x + p.WV;
    l.rel = l.sat + p.WC;
    l.nbr = l.rel + (size_t)p.A * p.WC;
    l.fm = l.nbr + (size_t)p.A * p.WV;
    l.fx = l.fm + obs_image_words(p);
    l.fd = l.fx + obs_image_words(p);
    l.sx = l.fd + (SH ? obs_image_words(p) + 1 : 0);
    l.ssat = l.sx + (SH ? p.WV : 0);
    l.red = reinterpret_cast<int *>(l.ssat + (SH ? p.WC : 0));
    l.own = reinterpret_cast<uint16_t *>(l.red + 16);
    return l;
}

// Assignment bytes -> LDS bit words, one ballot per 64 vars.  x0: this lane's byte of the first pass
// (var threadIdx.x, loaded early by the caller; any value where threadIdx.x >= V).
template <int T>
__device__ __forceinline__ void load_x_bits(const EnvParams &p, const EnvLds &l, const uint8_t *__restrict__ xg,
                                            uint32_t x0) {
    const int lane = threadIdx.x & 63;
    for (int v0 = threadIdx.x & ~63; v0 < p.WV * 32; v0 += T) {
        const int v = v0 + lane;
        const uint32_t xv = v0 == (int)(threadIdx.x & ~63) ? x0 : (v < p.V ? xg[v] : 0u);
        const uint64_t m = __ballot(v < p.V && (xv & 1u));
        if (lane < 2) l.x[(v0 >> 5) + lane] = (uint32_t)(m >> (32 * lane));
    }
}
template <int T>
__device__ __forceinline__ void load_x_bits(const EnvParams &p, const EnvLds &l, const uint8_t *__restrict__ xg) {
    load_x_bits<T>(p, l, xg, (int)threadIdx.x < p.V ? xg[threadIdx.x] : 0u);
}

// Prefetch depth (per lane) of the step path: pool-row words (covers C <= kPfClause*T
// clauses) and agent-table words, all issued right after problem_idx is known so the
// preamble costs ~2 dependent memory round trips instead of ~4.
constexpr int kPfClause = 4;
constexpr int kPfRel = 4;
constexpr int kPfNbr = 2;
// The depths of one instantiation.  The kernels of a launch with an obs shadow and int32 observations (SCATTER)
// prefetch no rel word: their running step scatters its changed elements and reads none, and their full writes load
// the table where they stage it (four loads per lane less on the step's chain).  Every other kernel keeps the depths
// above.  (Depths by width -- the whole uf200 row in registers at 64 and 128 lanes, 14 + 4 and 7 + 2 words -- did not
// make a narrow width win: DESIGN.md section 10, round 15.)
template <bool SCATTER>
struct PfDepth {
    static constexpr int clause = kPfClause;
    static constexpr int nbr = kPfNbr;
    static constexpr int rel = SCATTER ? 1 : kPfRel;  // (SCATTER: one unused word, not loaded)
    static constexpr bool load_rel = !SCATTER;
};

// Every global load this wave has issued has landed behind this point, and the compiler's wait-count bookkeeping knows
// it (an s_waitcnt in inline asm is opaque to it).  gfx950 counts loads and stores in the one vmcnt, so a register
// the bookkeeping believes some load under an earlier branch may still be writing (the cold tail loops of the
// actions, the shadow row and the assignment bytes, the reset-queue rank scan: a wait on one branch does not clear
// the state on the path that skipped it) gets a vmcnt(0) at its next definition -- and behind the clause scan's first
// byte stores that wait is a store round trip, once per slice and once per scattered store (DESIGN.md section 4,
// round 12).  The gfx9 encoding: vmcnt = imm[15:14]:imm[3:0] = 0; expcnt imm[6:4] and lgkmcnt imm[11:8] at their
// maxima (not waited for).
__device__ __forceinline__ void retire_loads() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// One 64-clause wave slice of the clause scan: c0 wave-uniform, w = this lane's pool word.
template <bool kPbrs>
__device__ __forceinline__ void clause_slice(const EnvParams &p, const EnvLds &l, int c0, uint64_t w,
                                             uint8_t *__restrict__ sat_g, uint8_t *__restrict__ ntrue_g, int &unsat,
                                             int &newly) {
    const int lane = threadIdx.x & 63;
    const int c = c0 + lane;
    uint32_t sat = 0, ntrue = 0, old = 0;
    const bool live = c < p.C;
    if (live) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t lit = (uint32_t)(w >> (16 * j)) & 0xFFFFu;
            if (lit < MSAT_LIT_ABSENT) ntrue += (bit(l.x, (int)(lit >> 1)) ^ lit) & 1u;
        }
        sat = ntrue ? 1u : 0u;
        if (kPbrs) old = sat_g[c];
        if (sat_g) sat_g[c] = (uint8_t)sat;  // NULL: a step whose reset another workgroup does (reset queue)
        if (ntrue_g) ntrue_g[c] = (uint8_t)ntrue;
    }
    const uint64_t ms = __ballot(sat);
    if (lane < 2) l.sat[(c0 >> 5) + lane] = (uint32_t)(ms >> (32 * lane));
    unsat += __popcll(__ballot(live && !sat));
    if (kPbrs) newly += __popcll(__ballot(sat && !old));
}

// Evaluate every clause of pool row `pidx` against l.x: clause bits -> l.sat,
// bytes -> sat_g / ntrue_g, unsat count (and PBRS newly-satisfied) -> red[0] / red[1].
// The first NPF slices (all NC of the prefetch, or none) use the lane's prefetched pool words pw[].
template <int T, bool kPbrs, bool kPf, int NC>
__device__ __forceinline__ void eval_clauses(const EnvParams &p, const EnvLds &l, const uint16_t *__restrict__ lits,
                                             int pidx, uint8_t *__restrict__ sat_g, uint8_t *__restrict__ ntrue_g,
                                             const uint64_t (&pw)[NC]) {
    constexpr int NPF = kPf ? NC : 0;
    const uint64_t *prow = reinterpret_cast<const uint64_t *>(lits) + (size_t)pidx * p.C;
    const int lane = threadIdx.x & 63;
    int unsat = 0, newly = 0;  // wave-uniform
    const int cend = p.WC * 32;
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
        const int c0 = (threadIdx.x & ~63) + j * T;
        if (c0 < cend) clause_slice<kPbrs>(p, l, c0, pw[j], sat_g, ntrue_g, unsat, newly);
    }
    for (int c0 = (threadIdx.x & ~63) + NPF * T; c0 < cend; c0 += T) {
        const int c = c0 + lane;
        const uint64_t w = c < p.C ? prow[c] : 0ull;  // pool rows are shared by many envs: keep them cached
        retire_loads();
        clause_slice<kPbrs>(p, l, c0, w, sat_g, ntrue_g, unsat, newly);
    }
    if (lane == 0) {
        atomicAdd(&l.red[0], unsat);
        if (kPbrs) atomicAdd(&l.red[1], newly);
    }
}

// ---------------------------------------------------------------- obs pass --
// The env's (A, D) observation block as two flat bit images over its A*D
// elements: FM (element != -1) and FX (its 0/1 value).  Row i, element k
// (env:345-398): k < V own vars (FM = owned, FX = x), V <= k < V+C clause
// status (FM = rel_i, FX = sat), k >= V+C neighbour vars (FM = nbr_i, FX = x).
// Built once per env from the LDS bit words (OR of shifted source words), then
// every 16 B store is a funnel-shifted extraction at its flat bit offset: no
// row/region logic and no divergence in the store loop, for any (V, C, A).

__device__ __forceinline__ uint32_t low_mask(int n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }

__device__ __forceinline__ void or_bits(uint32_t *img, int dst, uint32_t bits) {
    if (!bits) return;
    const int w = dst >> 5, s = dst & 31;
    atomicOr(&img[w], bits << s);
    if (s) {
        const uint32_t hi = bits >> (32 - s);
        if (hi) atomicOr(&img[w + 1], hi);
    }
}

// delta (G = 64 / 128; G = 16 builds no images, write_obs_sparse16): also FD, the elements whose value differs from the
// image of the shadow row (l.sx, l.ssat).  The masks are those of the same instance, so FD = (old ^ new) & FM per
// source word (mostly zero: or_bits returns at once).
template <int T, bool SH>
__device__ __forceinline__ void build_obs_images(const EnvParams &p, const EnvLds &l, bool delta) {
    const int nwV = (p.V + 31) >> 5, nwC = (p.C + 31) >> 5;
    const int U = 2 * nwV + nwC;  // source words per row
    for (int t = threadIdx.x; t < p.A * U; t += T) {
        const int i = t / U;
        int s = t - i * U;
        int len, off;
        uint32_t m, x, xo = 0;
        if (s < nwV) {  // own vars
            len = min(32, p.V - 32 * s);
            const int lo = agent_lo(p, i) - 32 * s, hi = lo + agent_size(p, i);
            const int a = max(lo, 0), z = min(hi, 32);
            m = z > a ? (low_mask(z) & ~low_mask(a)) : 0u;
            x = l.x[s];
            if (SH && delta) xo = l.sx[s];
            off = 32 * s;
        } else if ((s -= nwV) < nwC) {  // clause status
            len = min(32, p.C - 32 * s);
            m = l.rel[i * p.WC + s];
            x = l.sat[s];
            if (SH && delta) xo = l.ssat[s];
            off = p.V + 32 * s;
        } else {  // neighbour vars
            s -= nwC;
            len = min(32, p.V - 32 * s);
            m = l.nbr[i * p.WV + s];
            x = l.x[s];
            if (SH && delta) xo = l.sx[s];
            off = p.V + p.C + 32 * s;
        }
        const uint32_t keep = low_mask(len);
        const int dst = i * p.D + off;
        or_bits(l.fm, dst, m & keep);
        or_bits(l.fx, dst, x & m & keep);  // value bits only where the element is live
        if (SH && delta) or_bits(l.fd, dst, (x ^ xo) & m & keep);
    }
}

__device__ __forceinline__ uint32_t bits_at(const uint32_t *img, int e) {
    const int w = e >> 5, s = e & 31;
    return (uint32_t)((((uint64_t)img[w + 1] << 32) | img[w]) >> s);
}

__device__ __forceinline__ int elem_val(uint32_t m, uint32_t x, int u) {
    return ((m >> u) & 1u) ? (int)((x >> u) & 1u) : -1;
}

template <typename ObsT>
struct ObsVec;
template <>
struct ObsVec<int32_t> {
    static constexpr int N = 4;
    __device__ static void store(int32_t *dst, uint32_t m, uint32_t x) {
        typedef int v4i __attribute__((ext_vector_type(4)));
        const v4i q = {elem_val(m, x, 0), elem_val(m, x, 1), elem_val(m, x, 2), elem_val(m, x, 3)};
        *reinterpret_cast<v4i *>(dst) = q;
    }
};
template <>
struct ObsVec<int8_t> {
    static constexpr int N = 16;
    __device__ static void store(int8_t *dst, uint32_t m, uint32_t x) {
        // byte u = m_u ? x_u : 0xFF  (-1)
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        v4u q;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            uint32_t word = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) word |= ((uint32_t)elem_val(m, x, 4 * w + u) & 0xFFu) << (8 * u);
            q[w] = word;
        }
        *reinterpret_cast<v4u *>(dst) = q;
    }
};

// Stream the env's (A, D) observation block from the bit images: unaligned head, 16 B body, tail.
template <int T, typename ObsT>
__device__ __forceinline__ void write_obs(const EnvParams &p, const EnvLds &l, ObsT *__restrict__ o) {
    constexpr int VEC = ObsVec<ObsT>::N;
    const int total = p.A * p.D;
    int head = (int)((reinterpret_cast<uintptr_t>(o) / sizeof(ObsT)) % VEC);
    head = head ? VEC - head : 0;
    head = min(head, total);
    for (int e = threadIdx.x; e < head; e += T) o[e] = (ObsT)elem_val(bits_at(l.fm, e), bits_at(l.fx, e), 0);
    const int nchunks = (total - head) / VEC;
    for (int q = threadIdx.x; q < nchunks; q += T) {
        const int e = head + q * VEC;
        ObsVec<ObsT>::store(o + e, bits_at(l.fm, e), bits_at(l.fx, e));
    }
    for (int e = head + nchunks * VEC + threadIdx.x; e < total; e += T)
        o[e] = (ObsT)elem_val(bits_at(l.fm, e), bits_at(l.fx, e), 0);
}

// Debug builds: an obs chunk a delta step leaves alone must already hold the new image (a caller who wrote into the
// obs buffer without SATEnv.invalidate_obs shows up here).
template <typename ObsT>
__device__ __forceinline__ void dcheck_obs_kept(const EnvLds &l, const ObsT *o, int e, int n) {
#ifdef MSAT_DEBUG
    for (int u = 0; u < n; ++u)
        MSAT_DCHECK((int)o[e + u] == elem_val(bits_at(l.fm, e + u), bits_at(l.fx, e + u), 0) ? 0 : -1 - (e + u), 1);
#endif
}

// The delta form of write_obs: the same chunks, each stored only if its aligned group of G bytes (G = 16 / 64 / 128:
// a power of two >= the chunk, by absolute address, clipped to the env's block) holds an element whose FD bit is set;
// the unaligned head and tail elements each on their own bit.
template <int T, typename ObsT>
__device__ __forceinline__ void write_obs_delta(const EnvParams &p, const EnvLds &l, ObsT *__restrict__ o, int G) {
    constexpr int VEC = ObsVec<ObsT>::N;
    const int total = p.A * p.D;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(o) / sizeof(ObsT);  // o[0]'s absolute element index
    const int GE = G / (int)sizeof(ObsT);                                 // elements per group
    int head = (int)(a0 % VEC);
    head = head ? VEC - head : 0;
    head = min(head, total);
    for (int e = threadIdx.x; e < head; e += T) {
        if (bit(l.fd, e))
            o[e] = (ObsT)elem_val(bits_at(l.fm, e), bits_at(l.fx, e), 0);
        else
            dcheck_obs_kept(l, o, e, 1);
    }
    const int nchunks = (total - head) / VEC;
    for (int q = threadIdx.x; q < nchunks; q += T) {
        const int e = head + q * VEC;
        const int gs = e - (int)((a0 + (uintptr_t)e) & (uintptr_t)(GE - 1));  // the group's first element (< 0: clipped)
        const int lo = max(gs, 0), hi = min(gs + GE, total);
        uint32_t any = 0;
        for (int k = lo; k < hi; k += 32) any |= bits_at(l.fd, k) & low_mask(hi - k);
        if (any)
            ObsVec<ObsT>::store(o + e, bits_at(l.fm, e), bits_at(l.fx, e));
        else
            dcheck_obs_kept(l, o, e, VEC);
    }
    for (int e = head + nchunks * VEC + threadIdx.x; e < total; e += T) {
        if (bit(l.fd, e))
            o[e] = (ObsT)elem_val(bits_at(l.fm, e), bits_at(l.fx, e), 0);
        else
            dcheck_obs_kept(l, o, e, 1);
    }
}

// ---------------------------------------------------------------- kernel ----
// XCD-major env order: blocks b and b+8 share an XCD (round-robin dispatch, speed only),
// so consecutive envs -- adjacent obs blocks in HBM -- are written through one XCD's L2.
__device__ __forceinline__ int xcd_major(int blk, int n, bool off) {
    return (!off && (n & 7) == 0) ? (blk & 7) * (n >> 3) + (blk >> 3) : blk;
}

// Every workgroup barrier below is barrier_lds() (common.h), for LDS only: it waits for this wave's LDS operations,
// not for its global stores (a __syncthreads() fence drains every outstanding store).  env_run never reads back
// global memory written by another thread of its workgroup.  (A persistent variant that walks several envs per
// workgroup to overlap one env's store drain with the next env's scan measured slower at every
// occupancy, 114-188 us vs 112 us at uf200 x 4096: the 8 resident workgroups per CU already overlap.)

// Diagnostic stamps (msat_step_out.clock_stamps, NULL in product calls: a wave-uniform branch at each
// point).  Per env, 8 words written by lane 0 of wave 0 (vector stores):
//   [0] shader-clock counter delta over the workgroup's run (s_memtime), [1] the 100 MHz real-time counter
//   delta (s_memrealtime): clock MHz = 100 [0] / [1];
//   [2] real time at the workgroup's start, [3..6] at four phase ends (3: assignment bits + flips in LDS,
//   i.e. the first global loads landed; 4: clause scan done; 5: agent tables staged -- the span from 4 holds wave
//   0's own decision and transition outputs, the write-backs and the staging, no longer a barrier that waits for
//   lane 0; a sparse int32 step stages nothing and marks 5 right before its scatter; 6: obs bit images built, or the
//   sparse write's task loop or scatter done, its stores issued), [7] at the end, after wave 0's stores
//   have drained (vmcnt(0)).
// Same CU, same wave: the ratio is the clock that CU ran at while it stepped this env, and the phase times
// are wave 0's view of the env's dependent chain.
struct ClockStamp {
    uint64_t *buf = nullptr;
    uint64_t t0 = 0, r0 = 0;
    __device__ __forceinline__ ClockStamp(uint64_t *stamps, int b) {
        if (stamps != nullptr) {
            t0 = __builtin_amdgcn_s_memtime();
            r0 = __builtin_amdgcn_s_memrealtime();
            buf = stamps + 8 * (size_t)b;
        }
    }
    __device__ __forceinline__ void mark(int i) const {
        if (buf == nullptr) return;
        const uint64_t r = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) buf[2 + i] = i == 0 ? r0 : r;
    }
    __device__ __forceinline__ void finish() const {
        if (buf == nullptr) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x < 4) {
            const int i = threadIdx.x;
            buf[i == 3 ? 7 : i] = i == 0 ? t1 - t0 : i == 1 ? r1 - r0 : i == 2 ? r0 : r1;
        }
    }
};

__host__ __device__ __forceinline__ ObsGeom obs_geom(const EnvParams &p) {
    return ObsGeom{p.V, p.C, p.A, p.D, p.WV, p.WC, p.base, p.rem};
}

// One listed chunk of the sparse delta write (obs_sparse.h, sparse_entry): a fast entry carries its nibbles; a slow
// one (the chunk straddles a source word, a region, a row or an end of the block; every int8 chunk) is evaluated
// element by element from the bit words and the agent tables.
template <typename ObsT>
__device__ __forceinline__ void store_sparse_entry(const EnvParams &p, const EnvLds &l, ObsT *__restrict__ o,
                                                   uint32_t entry, int sh) {
    constexpr int VEC = ObsVec<ObsT>::N;
    if (VEC == 4 && (entry & kSparseFast)) {
        ObsVec<ObsT>::store(o + (int)(((entry >> 8) & 0x7FFFFFu) * 4u) - sh, (entry >> 4) & 15u, entry & 15u);
        return;
    }
    const ObsGeom g = obs_geom(p);
    const int total = p.A * p.D, e = (int)entry - sh;
    const int lo = max(e, 0), hi = min(e + VEC, total);
    uint32_t m = 0, x = 0;
    for (int u = lo; u < hi; ++u) {
        const int v = obs_elem(g, l.x, l.sat, l.rel, l.nbr, u);
        m |= (v >= 0 ? 1u : 0u) << (u - e);
        x |= (v > 0 ? 1u : 0u) << (u - e);
    }
    if (lo == e && hi == e + VEC) {
        ObsVec<ObsT>::store(o + e, m, x);
    } else {
        for (int u = lo; u < hi; ++u) o[u] = (ObsT)elem_val(m, x, u - e);
    }
}

// The sparse G = 16 delta write: no FM / FX / FD images.  Every (agent, source word) task reads its diff word
// (x ^ shadow x, sat ^ shadow sat) first and ends there when it is zero; the others mask it with the agent's table
// word and store their dirty chunks themselves, one sparse_entry at a time (sparse_task / sparse_entry) -- the agent
// tables stay live for the slow entries.  A chunk two tasks reach is stored by both: both stores carry the same
// bytes.  (Until round 10 the tasks listed their chunks in LDS and, behind a barrier, a second pass stored the list one
// chunk per lane: dense stores on 8 waves, but a prefix sum, an atomic, a barrier and a pass more per env; at 4 waves
// per workgroup storing in place is the faster form)
// Since round 11 this is the int8 form alone: int32 observations scatter their changed elements (scatter_obs).
template <int T, typename ObsT>
__device__ __forceinline__ void write_obs_sparse16(const EnvParams &p, const EnvLds &l, ObsT *__restrict__ o, int sh,
                                                   const ClockStamp *cs) {
    constexpr int VEC = ObsVec<ObsT>::N;
    const ObsGeom g = obs_geom(p);
    const int U = 2 * ((p.V + 31) >> 5) + ((p.C + 31) >> 5);  // source words per row
    // one division per lane and pass: the carried (agent, source word) pair of obs_sparse.h cost
    // shadow::env_kernel<2, int8, 256 / 512> a spilled VGPR (8 B of scratch per lane; profiles/r10/resource_usage.txt)
    for (int t0 = 0; t0 < p.A * U; t0 += T) {
        const int t = t0 + (int)threadIdx.x;
        const int i = t / U, s = t - i * U;
        const bool live = t < p.A * U;
        SparseTask k;
        uint64_t d = 0;
        if (live && sparse_task<VEC>(g, i, s, l.x, l.sat, l.sx, l.ssat, l.rel, l.nbr, sh, k)) d = k.dirty;
        // <= 16 chunks under one task (a dead task falls through with d = 0: skipping the loop with `continue`
        // compiled the int8 kernels at 256 / 512 lanes with a spilled VGPR)
        while (d) {
            store_sparse_entry<ObsT>(p, l, o, sparse_entry<VEC>(k, __ffsll((unsigned long long)d) - 1), sh);
            d &= d - 1;
        }
    }
    if (cs) cs->mark(4);
#ifdef MSAT_DEBUG
    // chunks in which no element differs from the shadow row's image are read back
    const int total = p.A * p.D;
    for (int q = threadIdx.x; q * VEC < total + sh; q += T) {
        const int lo = max(q * VEC - sh, 0), hi = min(q * VEC - sh + VEC, total);
        bool dirty = false;
        for (int e = lo; e < hi; ++e)
            dirty |= obs_elem(g, l.x, l.sat, l.rel, l.nbr, e) != obs_elem(g, l.sx, l.ssat, l.rel, l.nbr, e);
        if (dirty) continue;
        for (int e = lo; e < hi; ++e)
            MSAT_DCHECK((int)o[e] == obs_elem(g, l.x, l.sat, l.rel, l.nbr, e) ? 0 : -1 - e, 1);
    }
#endif
}

// Clause c of the scatter below: the lane that evaluated it (pool word w) stores its new status into the rows of the
// agents it is related to, if the status differs from the shadow row's.  rel[i][c] is "agent i owns a variable of
// clause c" (agent_tables_kernel), so the rows are the owners of the clause's real literals -- and, for a clause that
// holds a literal 0, every agent i >= rem when rem > 0 (the reference quirk).  Two literals of
// one owner store the same value twice.
__device__ __forceinline__ void scatter_clause(const EnvParams &p, const EnvLds &l, int c, uint64_t w,
                                               int32_t *__restrict__ o) {
    const uint32_t ns = l.sat[c >> 5];
    if ((((ns ^ l.ssat[c >> 5]) >> (c & 31)) & 1u) == 0) return;
    const int32_t val = (int32_t)((ns >> (c & 31)) & 1u);
    const int k = p.V + c;
    bool null_lit = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t code = (uint32_t)(w >> (16 * j)) & 0xFFFFu;
        if (code < MSAT_LIT_ABSENT) {
            const int e = (int)l.own[code >> 1] * p.D + k;
            MSAT_DCHECK(e, p.A * p.D);
            o[e] = val;
        }
        null_lit |= code == MSAT_LIT_NULL;
    }
    if (null_lit && p.rem > 0)  // rare: a plain loop
        for (int i = p.rem; i < p.A; ++i) o[i * p.D + k] = val;
}

// The sparse G = 16 delta write of int32 observations: every changed element stored on its own, 4 bytes, by a lane
// that already holds what decides it -- no agent table in LDS, no barrier behind the clause scan's, no chunks.
//   clause status   the lane that evaluated clause c in the scan (pool word pw[j], or reloaded past the prefetch);
//   own variables   lane v: element (own[v], v) if x_v differs from the shadow row's;
//   neighbours      task t = (agent t / WV, word t % WV): the set bits of (x ^ shadow x) & nbr word, the word from the
//                   prefetch (pnbr[j] is nbr word tid + j T of the instance) or, past it, from the pool's row.
// l.own (agent_of_var, 16 bits per variable) was filled before the first barrier of the step.  The bits of l.x, l.sx
// and the nbr words past V are zero or meet a zero nbr bit.
template <int T, int NC, int NN>
__device__ __forceinline__ void scatter_obs(const EnvParams &p, const EnvLds &l, const msat_pool &pool, int pidx,
                                            const uint64_t (&pw)[NC], const uint32_t (&pnbr)[NN],
                                            int32_t *__restrict__ o) {
    const int tid = threadIdx.x;
    const uint64_t *prow = reinterpret_cast<const uint64_t *>(pool.lits) + (size_t)pidx * p.C;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = tid + j * T;
        if (c < p.C) scatter_clause(p, l, c, pw[j], o);
    }
    for (int c = tid + NC * T; c < p.C; c += T) {
        const uint64_t w = prow[c];
        retire_loads();
        scatter_clause(p, l, c, w, o);
    }
    for (int v = tid; v < p.V; v += T) {
        const uint32_t xw = l.x[v >> 5];
        if (((xw ^ l.sx[v >> 5]) >> (v & 31)) & 1u) {
            const int e = (int)l.own[v] * p.D + v;
            MSAT_DCHECK(e, p.A * p.D);
            o[e] = (int32_t)((xw >> (v & 31)) & 1u);
        }
    }
    const uint32_t *nbr_g = pool.nbr + (size_t)pidx * p.A * p.WV;
    const int ntask = p.A * p.WV;
    const TaskIdx stride = task_stride(T, p.WV);
    TaskIdx ti = task_first(tid, p.WV);  // one division per lane; every further pass adds the stride (obs_sparse.h)
    auto task = [&](uint32_t m) {
        const uint32_t xw = l.x[ti.s];
        uint32_t fd = (xw ^ l.sx[ti.s]) & m;
        const int e0 = ti.i * p.D + p.V + p.C + 32 * ti.s;
        while (fd) {
            const int k = __ffs((int)fd) - 1;
            MSAT_DCHECK(e0 + k, p.A * p.D);
            o[e0 + k] = (int32_t)((xw >> k) & 1u);
            fd &= fd - 1;
        }
        task_advance(ti, stride, p.WV);
    };
#pragma unroll
    for (int j = 0; j < NN; ++j) task(pnbr[j]);  // (zero past the table's end)
    for (int t = tid + NN * T; t < ntask; t += T) {
        const uint32_t m = nbr_g[t];
        retire_loads();
        task(m);
    }
}

// The prefetch of an instance's pool row and agent tables into this lane's registers (one round trip).
template <int T, bool kRel, int NC, int NR, int NN>
__device__ __forceinline__ void prefetch_instance(const EnvParams &p, const msat_pool &pool, int n, uint64_t (&w)[NC],
                                                  uint32_t (&rl)[NR], uint32_t (&nb)[NN]) {
    // Branch-free: every lane loads a clamped (valid) address and zeroes what lies past the end.  Loads under a
    // branch leave the compiler's vmcnt bookkeeping unsure how many are in flight, so the first use of an
    // EARLIER load (the assignment byte) then waited for all of these (a whole round trip before the flips).
    const int tid = threadIdx.x;
    const uint64_t *prow = reinterpret_cast<const uint64_t *>(pool.lits) + (size_t)n * p.C;
    const uint32_t *rel_g = pool.rel + (size_t)n * p.A * p.WC;
    const uint32_t *nbr_g = pool.nbr + (size_t)n * p.A * p.WV;
    const int nrel = p.A * p.WC, nnbr = p.A * p.WV;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = tid + j * T;
        const uint64_t v = prow[min(c, p.C - 1)];
        w[j] = c < p.C ? v : 0ull;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (!kRel) {
            rl[j] = 0u;
            continue;
        }
        const int t = tid + j * T;
        const uint32_t v = rel_g[min(t, nrel - 1)];
        rl[j] = t < nrel ? v : 0u;
    }
#pragma unroll
    for (int j = 0; j < NN; ++j) {
        const int t = tid + j * T;
        const uint32_t v = nbr_g[min(t, nnbr - 1)];
        nb[j] = t < nnbr ? v : 0u;
    }
}

// The instance a reset of env b draws (env:158-162 via the rollout's reset, learner:426-436): the caller's index,
// or Philox word block 0 of (seed, ctr, env).
__device__ __forceinline__ int reset_instance(const EnvParams &p, const int32_t *__restrict__ new_pidx, uint64_t seed,
                                              uint64_t ctr, int b) {
    if (new_pidx != nullptr) return new_pidx[b];
    const uint4 r = reset_rng_block(seed, ctr, (uint32_t)b, 0u);
    return (int)(((uint64_t)r.x * (uint64_t)p.N) >> 32);
}

// The assignment a reset of env b draws into l.x: the caller's bytes, or word t = lane t % 4 of the Philox block
// 1 + t / 4 (128 vars per block).
template <int T>
__device__ __forceinline__ void reset_assignment(const EnvParams &p, const EnvLds &l,
                                                 const uint8_t *__restrict__ new_assign, uint64_t seed, uint64_t ctr,
                                                 int b) {
    if (new_assign != nullptr) {
        load_x_bits<T>(p, l, new_assign + (size_t)b * p.V);
        return;
    }
    for (int t = threadIdx.x; t < p.WV; t += T) {
        const uint4 r = reset_rng_block(seed, ctr, (uint32_t)b, 1u + (uint32_t)(t >> 2));
        const int lane = t & 3;
        uint32_t w = lane == 0 ? r.x : lane == 1 ? r.y : lane == 2 ? r.z : r.w;
        const int hi = p.V - 32 * t;
        if (hi < 32) w &= hi <= 0 ? 0u : ((1u << hi) - 1u);
        l.x[t] = w;
    }
}

// Stage instance pidx's agent tables in LDS (the first kPf* words from this lane's prefetch registers when pf),
// build the obs bit images and stream the env's (A, D) block -- or, on a delta step with 16-byte groups, store what
// changed straight from the source diff: int32 observations element by element with nothing staged (scatter_obs),
// int8 ones the dirty chunks behind the staging (write_obs_sparse16).
// SH: the launch has an obs shadow (shadow::env_kernel; without one the code is the plain full write).
template <typename ObsT, int T, bool SH, int NC, int NR, int NN>
__device__ __forceinline__ void stage_and_write_obs(const EnvParams &p, const EnvLds &l, const msat_pool &pool,
                                                    int pidx, bool pf, const uint64_t (&pw)[NC],
                                                    const uint32_t (&prel)[NR], const uint32_t (&pnbr)[NN],
                                                    ObsT *__restrict__ o, const ClockStamp *cs,
                                                    uint32_t *__restrict__ srow, bool delta, int delta_g, int ndiff) {
    // srow: the env's obs shadow row (NULL: none), rewritten to describe this write.  delta: l.sx / l.ssat hold the
    // row as it was, it named this instance, and the block holds its image: store only what differs.
    const int tid = threadIdx.x;
    const int nwV = (p.V + 31) >> 5, nwC = (p.C + 31) >> 5;
    // a step that flipped more than a quarter of the env's variable + clause bits (ndiff, counted by env_run right
    // after the clause scan; mode-1 actions can flip them all) touches most groups anyway: the plain full write,
    // decided before any image work
    if (!SH || (delta && 4 * ndiff > p.V + p.C)) delta = false;
    // G = 16: the sparse write from the source diff, no bit images (and none to zero)
    const bool sparse = SH && delta && delta_g == 16;  // (a launch with a shadow is never an ablated one)
    if (SH && srow != nullptr) {
        if (tid == 0) srow[0] = (uint32_t)pidx;
        for (int t = tid; t < nwV + nwC; t += T) srow[1 + t] = t < nwV ? l.x[t] : l.sat[t - nwV];
    }
    // int32: a sparse step scatters its changed elements from registers and the bit words (scatter_obs): no table is
    // staged and no barrier follows the clause scan's (l.x, l.sat, l.sx, l.ssat and l.own are final since then, and
    // nothing in LDS is written any more).  Marks 3 and 4 bracket the scatter.
    constexpr bool kScatter = SH && sizeof(ObsT) == 4;
    if constexpr (kScatter) {
        if (sparse) {
            if (cs) cs->mark(3);
            scatter_obs<T>(p, l, pool, pidx, pw, pnbr, reinterpret_cast<int32_t *>(o));
            if (cs) cs->mark(4);
#ifdef MSAT_DEBUG
            // every element whose value did not change is read back, the evaluator on the instance's table rows in
            // global memory (a sparse int32 step stages no table in LDS)
            const uint32_t *rel_g = pool.rel + (size_t)pidx * p.A * p.WC;
            const uint32_t *nbr_g = pool.nbr + (size_t)pidx * p.A * p.WV;
            const ObsGeom g = obs_geom(p);
            for (int e = tid; e < p.A * p.D; e += T) {
                const int nv = obs_elem(g, l.x, l.sat, rel_g, nbr_g, e);
                if (nv == obs_elem(g, l.sx, l.ssat, rel_g, nbr_g, e)) MSAT_DCHECK((int)o[e] == nv ? 0 : -1 - e, 1);
            }
#endif
            return;
        }
    }
    {
        const uint32_t *rel_g = pool.rel + (size_t)pidx * p.A * p.WC;
        const uint32_t *nbr_g = pool.nbr + (size_t)pidx * p.A * p.WV;
        int t0r = 0, t0n = 0;
        if (pf) {
            if (!kScatter) {  // (the kScatter kernels prefetch no rel word: PfDepth)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (tid + j * T < p.A * p.WC) l.rel[tid + j * T] = prel[j];
                t0r = NR * T;
            }
#pragma unroll
            for (int j = 0; j < NN; ++j)
                if (tid + j * T < p.A * p.WV) l.nbr[tid + j * T] = pnbr[j];
            t0n = NN * T;
        }
        for (int t = t0r + tid; t < p.A * p.WC; t += T) l.rel[t] = rel_g[t];
        for (int t = t0n + tid; t < p.A * p.WV; t += T) l.nbr[t] = nbr_g[t];
        if (!sparse)
            for (int t = tid; t < (SH && delta ? 3 * obs_image_words(p) + 1 : 2 * obs_image_words(p)); t += T)
                l.fm[t] = 0u;  // fm, fx, fd contiguous
    }
    barrier_lds();
    if (cs) cs->mark(3);
    if (SH && !kScatter && sparse) {  // int8
        write_obs_sparse16<T, ObsT>(p, l, o, (int)((reinterpret_cast<uintptr_t>(o) / sizeof(ObsT)) % ObsVec<ObsT>::N),
                                    cs);
    } else if ((p.ablate & 3) == 0) {
        build_obs_images<T, SH>(p, l, delta);
        barrier_lds();
        if (cs) cs->mark(4);
        if (SH && delta)
            write_obs_delta<T, ObsT>(p, l, o, delta_g);
        else
            write_obs<T, ObsT>(p, l, o);
    } else {
        constexpr int VEC = ObsVec<ObsT>::N;
        const int n = (p.A * p.D) / VEC;
        for (int q = tid; q < n; q += T) ObsVec<ObsT>::store(o + q * VEC, 0u, 0u);
    }
}

// One environment (index b of its batch) advanced / reset / observed by one workgroup.
//
// Workgroup barriers, by path (every wave of a workgroup takes the same path: each condition below is a function of
// launch parameters, uniformly loaded words and LDS words that are final since the previous barrier):
//   running step   B1 assignment bits | B2 flips | B3 clause scan | B5 tables staged | B6 images built (a sparse
//                  delta step has no B6: its tasks store their chunks themselves; with int32 observations it has no
//                  B5 either: it stages nothing and scatters its changed elements, scatter_obs)
//   covered        B1 | B2 | B3 | R0 before the reset rewrites l.x | R1 new assignment bits, then the write-back; no obs
//   in-workgroup   B1 | B2 | B3 | R0 before l.x is rewritten and red[0..1] zeroed | R2 new assignment bits |
//   reset                        R3 its clause scan | B5 | B6
//   reset mode     R2 | R3 | B5 | B6               (msat_env_reset: no step in front)
//   obs only       B1 | B2 | B3 | B5 | B6          (no flips between B1 and B2, no state written)
//   reset workgroup (env_side_reset)  the rank scan | assignment bits | clause scan | B5 | B6
// After B3 nothing is broadcast: every wave reads red[0] (unsat count) and red[3] (covered) and derives done, the
// reset decision and, with a shadow, the diff count itself, so no wave waits for lane 0's transition outputs.
template <int MODE, typename ObsT, int T, bool SH = false>
__device__ __forceinline__ void env_run(const EnvParams &p, const msat_pool &pool, const msat_env_state &st,
                                        const int32_t *__restrict__ actions, const uint8_t *__restrict__ reset_mask,
                                        const int32_t *__restrict__ new_pidx, const uint8_t *__restrict__ new_assign,
                                        uint64_t seed, uint64_t ctr, const msat_step_out &out, ObsT *__restrict__ obs,
                                        int b, uint32_t *smem, const ClockStamp &cs,
                                        const ObsShadowArg sa = ObsShadowArg{nullptr, 0}) {
    const EnvLds l = carve<SH>(smem, p);
    const int tid = threadIdx.x;
    if (MODE == kModeReset && reset_mask != nullptr && reset_mask[b] == 0) return;

    uint8_t *__restrict__ xg = st.assign + (size_t)b * p.V;
    uint8_t *__restrict__ sat_g = st.clause_sat + (size_t)b * p.C;
    uint8_t *__restrict__ ntrue_g = st.clause_ntrue ? st.clause_ntrue + (size_t)b * p.C : nullptr;
    if (tid < 16) l.red[tid] = 0;
    // reset queue: rq_fast = this autoreset launch consumes / produces it; rq_mode 2 = clear this env's entries
    const bool rq_fast = MODE == kModeStepAutoReset && p.rq_mode == 1;  // host: sparse reward, mode 0, A < 64
    if (MODE != kModeObs && p.rq_mode == 2 && tid == 0) {
        rq_pend(st.reset_queue, p.B, 0)[b] = 0u;
        rq_pend(st.reset_queue, p.B, 1)[b] = 0u;
    }

    bool do_reset = (MODE == kModeReset);
    int ndiff = 0;  // SH: source bits that differ from the shadow row (a stepped env that does not reset)
    // the per-lane loads that do not depend on problem_idx, issued together with it (one round trip): this
    // lane's action and its assignment byte of the first ballot pass (clamped indices, no branches), then
    // problem_idx, step and unsat.  (step / unsat are wave-uniform values the compiler moves to scalar registers
    // as soon as they are loaded, i.e. waits for them right there: issued behind problem_idx, that wait retires
    // the first round trip, which the prefetch needs anyway.  Issued behind the prefetch (round 5), it held the
    // assignment bits and the flips until the prefetch had landed too.)
    int step0 = 0, u_old = 0, a0 = 0;
    uint32_t x0 = 0;
    bool covered = false;
    // the reset-queue entry rides in the action load: lane A of wave 0 (mode 0, A < 64) reads it instead of a
    // duplicate action, so it costs no round trip of its own
    if (MODE != kModeReset) {
        if (MODE != kModeObs && p.action_mode == 0) {
            const int32_t *ap = actions + (size_t)b * p.A + min(tid, p.A - 1);
            if (rq_fast && tid == p.A)
                ap = reinterpret_cast<const int32_t *>(rq_pend(st.reset_queue, p.B, p.rq_serial & 1) + b);
            a0 = *ap;
        }
        x0 = xg[min(tid, p.V - 1)];
    }
    // the env's obs shadow row rides in the same round trip: word tid (the few rows longer than the workgroup
    // load the rest behind the assignment bits)
    const int srw = shadow_row_words(p);
    uint32_t *const srow = SH ? sa.rows + (size_t)b * srw : nullptr;
    uint32_t sh0 = 0;
    if (SH && MODE != kModeReset) sh0 = srow[min(tid, srw - 1)];  // (SH is a template argument: no branch)
    int pidx = st.problem_idx[b];
    if (MODE != kModeReset) {
        step0 = st.step[b];
        u_old = st.num_unsat[b];
    }
    // keep the first round trip's loads ahead of the prefetch (the scheduler sank the assignment byte below it,
    // and its first use then waited for the prefetch as well)
    __builtin_amdgcn_sched_barrier(0);
    if (MSAT_DEBUG_BUILD && tid == 0) {  // this env's rows of every caller buffer, and its pool row
        if (MODE != kModeReset) MSAT_DCHECK(pidx, p.N);
        MSAT_DCHECK((long long)(b + 1) * p.V - 1, p.dbg_assign);
        MSAT_DCHECK((long long)(b + 1) * p.C - 1, p.dbg_sat);
        if (ntrue_g) MSAT_DCHECK((long long)(b + 1) * p.C - 1, p.dbg_ntrue);
        if (obs) MSAT_DCHECK((long long)(b + 1) * p.A * p.D - 1, p.dbg_obs);
        if (MODE == kModeStep || MODE == kModeStepAutoReset)
            MSAT_DCHECK((long long)(b + 1) * p.A * (p.action_mode == 0 ? 1 : p.M) - 1, p.dbg_actions);
    }
    using Pf = PfDepth<SH && sizeof(ObsT) == 4>;
    uint64_t pw[Pf::clause];
    uint32_t prel[Pf::rel], pnbr[Pf::nbr];
    if (MODE != kModeReset) {
        // ---- then the loads that do: the instance's pool row and agent tables (second round trip) --------
        prefetch_instance<T, Pf::load_rel>(p, pool, pidx, pw, prel, pnbr);
        __builtin_amdgcn_sched_barrier(0);
        // a step that may scatter its changed elements (int32, 16-byte groups): the variables' owners, one division
        // per lane while the prefetch is in flight; read behind the clause scan's barrier
        if (SH && sizeof(ObsT) == 4 && sa.g == 16 && (MODE == kModeStep || MODE == kModeStepAutoReset))
            for (int v = tid; v < p.V; v += T) l.own[v] = (uint16_t)agent_of_var(p, v);
        // ---- assignment + the agents' flips (env:230-250) --------------------
        load_x_bits<T>(p, l, xg, x0);
        barrier_lds();
        cs.mark(1);
        if (SH) {  // the shadow row -> red[5] (the instance it names), l.sx, l.ssat
            const int nwV = (p.V + 31) >> 5;
            for (int t = tid; t < srw; t += T) {
                const uint32_t w = t == tid ? sh0 : srow[t];
                if (t == 0)
                    l.red[5] = (int)w;
                else if (t <= nwV)
                    l.sx[t - 1] = w;
                else
                    l.ssat[t - 1 - nwV] = w;
            }
        }
        if (MODE == kModeObs) {
            // get_obs only: no flips, no state update
        } else if (p.action_mode == 0) {
            if (rq_fast && tid < 64) {  // wave 0: is this env covered?  (read by every wave after the barrier)
                const uint32_t tok = rq_token(p.rq_serial);
                int cov = 0;
                if (__builtin_amdgcn_readlane(a0, p.A) == (int)tok) {  // pending: its rank among the pending envs
                    int unused;
                    cov = rq_scan(rq_pend(st.reset_queue, p.B, p.rq_serial & 1), p.B, tok, b, -1, &unused) < p.rq_cap;
                }
                if (tid == 0) l.red[3] = cov;
            }
            for (int i = tid; i < p.A; i += T) {
                const int a = i == tid ? a0 : actions[(size_t)b * p.A + i];
                const int n = agent_size(p, i);
                if (a >= n) continue;  // no-op index (and every action of a var-less agent)
                int s = a;
                if (s < 0) {
                    s += p.M;  // jnp negative-index normalisation
                    if (s < 0) {
                        if (p.reward_mode == MSAT_REWARD_SINGLE_DELTA) continue;  // x.at[a] scatter drops it
                        s = 0;                                                   // agent_vars gather clamps
                    }
                }
                if (s < n) {
                    const int v = agent_lo(p, i) + s;
                    atomicXor(&l.x[v >> 5], 1u << (v & 31));
                }
            }
        } else {
            for (int t = tid; t < p.A * p.M; t += T) {
                const int i = t / p.M, j = t - (t / p.M) * p.M;
                if (j < agent_size(p, i) && (actions[(size_t)b * p.A * p.M + t] & 1)) {
                    const int v = agent_lo(p, i) + j;
                    atomicXor(&l.x[v >> 5], 1u << (v & 31));
                }
            }
        }
        barrier_lds();
        // every load of the step so far -- the first round trip, the prefetch (issued two phases ago; the scan needs its
        // pool words here anyway), the cold tail loops -- is retired at this one point, which dominates the scan, the
        // decision, the write-backs and the scatter: behind it no register carries a pending load, so none of them
        // waits for the wave's own stores.  In the kernels with an obs shadow only: the launches without one stage the
        // rel / nbr prefetch behind the scan and measured 0.3-0.7 % slower with the wait here
        if (SH) retire_loads();
        // ---- clause scan of the stepped assignment (env:252-254); a covered env (a reset workgroup of this launch
        // resets it: it times out now, listed by the previous launch) leaves its clause state to that workgroup
        covered = rq_fast && l.red[3] != 0;
        uint8_t *const scan_sat = covered ? nullptr : sat_g;
        uint8_t *const scan_ntrue = covered ? nullptr : ntrue_g;
        if (MODE != kModeObs && p.reward_mode == MSAT_REWARD_PBRS)
            eval_clauses<T, true, true>(p, l, pool.lits, pidx, scan_sat, scan_ntrue, pw);
        else
            eval_clauses<T, false, true>(p, l, pool.lits, pidx, scan_sat, scan_ntrue, pw);
        barrier_lds();
        cs.mark(2);
        // ---- the decision, taken by every wave for itself from what the scan's barrier published (red[0], red[3])
        // and the uniformly loaded step0: nothing is broadcast, nobody waits for lane 0's transition outputs
        const int u_new = MODE != kModeObs ? __builtin_amdgcn_readfirstlane(l.red[0]) : 0;
        const bool solved = (u_new == 0);
        // single-agent SatEnv (sat_env.py:106) tests the pre-increment step
        const bool done = solved || (p.reward_mode == MSAT_REWARD_SINGLE_DELTA ? step0 >= p.max_steps
                                                                               : step0 + 1 >= p.max_steps);
        // a covered env times out now (the previous launch listed it at max_steps - 1): its reset happens in any
        // case, here and in its reset workgroup, so the state stays whole even for a misused queue
        const bool reset_now = (MODE == kModeStepAutoReset) && (done || covered);
        do_reset = reset_now;
        if (SH && !do_reset) {  // source bits that differ from the shadow row: the obs write's full-or-sparse decision
                                // needs nothing else.  Each wave sums the nwV + nwC diff words itself (shuffles)
            const int nwV = (p.V + 31) >> 5, nwC = (p.C + 31) >> 5;
            int n = 0;
            for (int t = tid & 63; t < nwV + nwC; t += 64)
                n += t < nwV ? __popc(l.x[t] ^ l.sx[t]) : __popc(l.sat[t - nwV] ^ l.ssat[t - nwV]);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
            ndiff = n;
        }
        if (MODE != kModeObs && tid == 0) {
            float r;
            if (p.reward_mode == MSAT_REWARD_SINGLE_DELTA) {
                // sat_env.py:86-101, f32 in the reference's order: ((u_prev - u_new) * 10 + bonus) + (-0.005)
                const float up = __fdiv_rn((float)u_old, (float)p.C), un = __fdiv_rn((float)u_new, (float)p.C);
                r = __fmul_rn(__fsub_rn(up, un), 10.0f);
                r = __fadd_rn(r, solved ? p.r_sat : 0.0f);
                r = __fadd_rn(r, -0.005f);
            } else if (p.reward_mode == MSAT_REWARD_PBRS) {
                const float pot_new = (float)(-u_new), pot_old = (float)(-u_old);
                const float r_pbrs = __fsub_rn(__fmul_rn(p.gamma, pot_new), pot_old);
                const float r_cl = __fmul_rn((float)l.red[1], p.r_clause);
                r = __fadd_rn(__fadd_rn(r_pbrs, r_cl), solved ? p.r_sat : 0.0f);
            } else {
                r = solved ? 1.0f : 0.0f;
            }
            out.reward[b] = r;
            out.done[b] = done ? 1 : 0;
            out.solved[b] = solved ? 1 : 0;
            if (out.num_unsat) out.num_unsat[b] = u_new;
            if (out.episode_step) out.episode_step[b] = step0 + 1;
            MSAT_DCHECK(covered && !done ? 1 : 0, 1);
            if (!reset_now) {
                st.num_unsat[b] = u_new;
                st.step[b] = step0 + 1;
                st.done[b] = done ? 1 : 0;
            }
            if (rq_fast) {  // list this env for the next launch if its next step times out
                const int next_step = reset_now ? 0 : step0 + 1;
                rq_pend(st.reset_queue, p.B, (p.rq_serial + 1) & 1)[b] =
                    next_step + 1 >= p.max_steps ? rq_token(p.rq_serial + 1u) : 0u;
            }
        }
    }

    if (do_reset) {
        // ---- reset (env:158-181): new problem, new assignment ---------------
        // A stepped env that resets here: slower waves may still be reading red[0] / red[3] (their decision) and l.x;
        // the reset rewrites l.x and zeroes red[0..1], so it waits for them first.  Uniform: do_reset is a function of
        // red[0], red[3] (both final since the scan's barrier, neither written before this one), step0 and the
        // launch's parameters, the same values in every wave.
        if (MODE != kModeReset) barrier_lds();
        pidx = reset_instance(p, new_pidx, seed, ctr, b);
        if (MSAT_DEBUG_BUILD && tid == 0) MSAT_DCHECK(pidx, p.N);  // the reset's pool row
        reset_assignment<T>(p, l, new_assign, seed, ctr, b);
        if (covered) {
            // the reset workgroup scans the new instance and writes its clause state, count and observation;
            // this one writes the fields it read: assignment, step, done, problem_idx
            barrier_lds();
            if (tid == 0) {
                st.step[b] = 0;
                st.done[b] = 0;
                st.problem_idx[b] = pidx;
            }
            for (int v = tid; v < p.V; v += T) xg[v] = (uint8_t)bit(l.x, v);
            return;
        }
        if (tid < 2) l.red[tid] = 0;  // (every wave has read them: the barrier above)
        barrier_lds();
        eval_clauses<T, false, false>(p, l, pool.lits, pidx, sat_g, ntrue_g, pw);
        barrier_lds();
        if (tid == 0) {
            st.num_unsat[b] = l.red[0];
            st.step[b] = 0;
            st.done[b] = 0;
            st.problem_idx[b] = pidx;
        }
    }
    if (MODE != kModeObs)
        for (int v = tid; v < p.V; v += T) xg[v] = (uint8_t)bit(l.x, v);
    if ((p.ablate & 3) == 2 || obs == nullptr) return;  // NULL obs: state-only step (single-agent SatEnv)
    // ---- the instance's agent tables (built once per pool instance), obs images, obs stores ----------------
    // delta: the block holds the image of its shadow row, and that row names this instance (same masks)
    const bool delta = SH && (MODE == kModeStep || MODE == kModeStepAutoReset) && sa.g != 0 && !do_reset &&
                       l.red[5] == pidx;
    stage_and_write_obs<ObsT, T, SH>(p, l, pool, pidx, (MODE != kModeReset) && !do_reset, pw, prel, pnbr,
                                     obs + (size_t)b * p.A * p.D, &cs, srow, delta, sa.g, ndiff);
}

// A reset workgroup of an autoreset launch with a reset queue (rq_mode 1): the pending env of rank j, i.e. an env that
// times out in this launch.  It draws the env's new instance and assignment (the same draw as its step workgroup's),
// scans the new instance, and writes the clause state, the unsatisfied count and the observation; its step workgroup
// writes the transition outputs, the assignment, step, done and problem_idx.  Two dependent round trips: the
// pending words (wave 0's scan), then the pool row and agent tables.
template <typename ObsT, int T, bool SH>
__device__ __forceinline__ void env_side_reset(const EnvParams &p, const msat_pool &pool, const msat_env_state &st,
                                               const int32_t *__restrict__ new_pidx,
                                               const uint8_t *__restrict__ new_assign, uint64_t seed, uint64_t ctr,
                                               ObsT *__restrict__ obs, int j, uint32_t *smem,
                                               const ObsShadowArg sa = ObsShadowArg{nullptr, 0}) {
    const EnvLds l = carve<SH>(smem, p);
    const int tid = threadIdx.x;
    if (tid < 64) {
        int b = -1;
        rq_scan(rq_pend(st.reset_queue, p.B, p.rq_serial & 1), p.B, rq_token(p.rq_serial), 0, j, &b);
        if (tid == 0) l.red[4] = b;
    }
    if (tid < 4) l.red[tid] = 0;
    barrier_lds();
    const int b = l.red[4];
    if (b < 0) return;  // fewer than j + 1 envs time out in this launch
    const int pidx = reset_instance(p, new_pidx, seed, ctr, b);
    if (MSAT_DEBUG_BUILD && tid == 0) MSAT_DCHECK(pidx, p.N);
    using Pf = PfDepth<SH && sizeof(ObsT) == 4>;
    uint64_t pw[Pf::clause];
    uint32_t prel[Pf::rel], pnbr[Pf::nbr];
    prefetch_instance<T, Pf::load_rel>(p, pool, pidx, pw, prel, pnbr);
    reset_assignment<T>(p, l, new_assign, seed, ctr, b);
    barrier_lds();
    uint8_t *__restrict__ sat_g = st.clause_sat + (size_t)b * p.C;
    uint8_t *__restrict__ ntrue_g = st.clause_ntrue ? st.clause_ntrue + (size_t)b * p.C : nullptr;
    eval_clauses<T, false, true>(p, l, pool.lits, pidx, sat_g, ntrue_g, pw);
    barrier_lds();
    if (tid == 0) st.num_unsat[b] = l.red[0];
    if ((p.ablate & 3) == 2 || obs == nullptr) return;
    // the whole block and a fresh shadow row (its step workgroup touches neither)
    stage_and_write_obs<ObsT, T, SH>(p, l, pool, pidx, true, pw, prel, pnbr, obs + (size_t)b * p.A * p.D, nullptr,
                                     SH ? sa.rows + (size_t)b * shadow_row_words(p) : nullptr, false, 0, 0);
}

template <int MODE, typename ObsT, int T>
__global__ void __launch_bounds__(T)
env_kernel(EnvParams p, msat_pool pool, msat_env_state st, const int32_t *__restrict__ actions,
           const uint8_t *__restrict__ reset_mask, const int32_t *__restrict__ new_pidx,
           const uint8_t *__restrict__ new_assign, uint64_t seed, uint64_t ctr, msat_step_out out,
           ObsT *__restrict__ obs) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    // the reset workgroups first (block ids 0 .. cap - 1: their chain starts with a scan of the pending marks, and a
    // place at the end of the dispatch order made them the launch's tail)
    const int side = (MODE == kModeStepAutoReset && p.rq_mode == 1) ? p.rq_cap : 0;
    if ((int)blockIdx.x < side) {
        env_side_reset<ObsT, T, false>(p, pool, st, new_pidx, new_assign, seed, ctr, obs, (int)blockIdx.x, smem);
        return;
    }
    const int b = xcd_major((int)blockIdx.x - side, p.B, p.ablate & 4);
    const ClockStamp cs(out.clock_stamps, b);
    env_run<MODE, ObsT, T, false>(p, pool, st, actions, reset_mask, new_pidx, new_assign, seed, ctr, out, obs, b, smem,
                                  cs);
    cs.finish();
}

// The step kernel of a launch with an obs shadow (msat_env_step_delta): the same body with the shadow's loads, LDS
// words and delta write compiled in (SH), as a kernel of its own under the same name in a nested namespace.  In one
// body (and then in two bodies under one branch of the one kernel) the shadow code cost the launches WITHOUT a shadow
// 3-12 % (uf50 x 1,024: 8.45, then 8.03 vs 7.57 us: 65-68 instead of 48 VGPRs, 66-85 instead of 44 spilled SGPRs);
// apart, they run the code they ran before.  The shadow's pointer and group size are arguments of this kernel alone
// (ObsShadowArg), not EnvParams fields: 16 more bytes in every env kernel's (and eight times that in the grouped
// kernel's) arguments and an LDS carve that read them still cost uf50 x 1,024 and mixed x 1,024 1.9 %.
#ifndef MSAT_SHADOW_W8_MIN_T
#define MSAT_SHADOW_W8_MIN_T 256
#endif
namespace shadow {
template <int MODE, typename ObsT, int T>
// 256 and 512 lanes (the widths env_delta_threads picks for the shapes this write is the default of): 8 waves per
// SIMD, i.e. eight resident 256-lane workgroups per CU instead of seven, four 512-lane ones instead of three (the
// launch is bound by how many dependent chains a CU runs one after the other); without scratch
// for either ObsT (profiles/r10/resource_usage.txt).  64 and 128 lanes compile as without the attribute.
// MSAT_SHADOW_W8_MIN_T: A/B builds only (make ab)
__global__ void __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(T >= MSAT_SHADOW_W8_MIN_T ? 8 : 1, 8)))
env_kernel(EnvParams p, msat_pool pool, msat_env_state st, const int32_t *__restrict__ actions,
           const uint8_t *__restrict__ reset_mask, const int32_t *__restrict__ new_pidx,
           const uint8_t *__restrict__ new_assign, uint64_t seed, uint64_t ctr, msat_step_out out,
           ObsT *__restrict__ obs, uint32_t *__restrict__ shadow_rows, int shadow_g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const ObsShadowArg sa{shadow_rows, shadow_g};
    const int side = (MODE == kModeStepAutoReset && p.rq_mode == 1) ? p.rq_cap : 0;
    if ((int)blockIdx.x < side) {
        env_side_reset<ObsT, T, true>(p, pool, st, new_pidx, new_assign, seed, ctr, obs, (int)blockIdx.x, smem,
                                      sa);
        return;
    }
    const int b = xcd_major((int)blockIdx.x - side, p.B, p.ablate & 4);
    const ClockStamp cs(out.clock_stamps, b);
    env_run<MODE, ObsT, T, true>(p, pool, st, actions, reset_mask, new_pidx, new_assign, seed, ctr, out, obs, b, smem,
                                 cs, sa);
    cs.finish();
}

// The same kernel compiled for one geometry: an overload with the Shape (a StaticShape, env_params.h) as a fourth
// template argument, the same arguments and the same body behind pin_shape, which gives p's geometry fields the
// shape's constants.  The host's only choice is which of the two to launch (launch_env_kernel).  An overload and a
// body of its own, not a defaulted parameter or a shared body: either changes the symbols or the code of the
// kernels above (profiles/kernel_identity.py), which every other shape keeps running.
template <int MODE, typename ObsT, int T, class Shape>
__global__ void __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(T >= MSAT_SHADOW_W8_MIN_T ? 8 : 1, 8)))
env_kernel(EnvParams p, msat_pool pool, msat_env_state st, const int32_t *__restrict__ actions,
           const uint8_t *__restrict__ reset_mask, const int32_t *__restrict__ new_pidx,
           const uint8_t *__restrict__ new_assign, uint64_t seed, uint64_t ctr, msat_step_out out,
           ObsT *__restrict__ obs, uint32_t *__restrict__ shadow_rows, int shadow_g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    pin_shape<Shape>(p);
    const ObsShadowArg sa{shadow_rows, shadow_g};
    const int side = (MODE == kModeStepAutoReset && p.rq_mode == 1) ? p.rq_cap : 0;
    if ((int)blockIdx.x < side) {
        env_side_reset<ObsT, T, true>(p, pool, st, new_pidx, new_assign, seed, ctr, obs, (int)blockIdx.x, smem,
                                      sa);
        return;
    }
    const int b = xcd_major((int)blockIdx.x - side, p.B, p.ablate & 4);
    const ClockStamp cs(out.clock_stamps, b);
    env_run<MODE, ObsT, T, true>(p, pool, st, actions, reset_mask, new_pidx, new_assign, seed, ctr, out, obs, b, smem,
                                 cs, sa);
    cs.finish();
}
}  // namespace shadow

// Ragged batches (BASELINE config 5): several size classes, each its own (V, C, A) batch with its own
// pool / state / obs, advanced by ONE launch (256-lane workgroups).  Blocks map to (class, env) with
// the classes laid out most expensive first (launch_groups).  Class g draws its resets from seed ^ group_seed(g), so it
// replays exactly as a single-class launch with that seed (group_seed(0) = 0).
struct EnvGroup {
    EnvParams p;
    msat_pool pool;
    msat_env_state st;
    const int32_t *actions;
    msat_step_out out;
    void *obs;
    int begin;  // first block of the class
    int gid;    // the class's index in the caller's arrays (selects its RNG stream)
};

struct EnvGroups {
    int G, total, ablate;
    EnvGroup g[MSAT_MAX_GROUPS];
};

static_assert(sizeof(EnvGroups) <= 4096, "EnvGroups is passed by value: kernel arguments are limited to 4 KiB");

__host__ __device__ __forceinline__ uint64_t group_seed(int g) { return (uint64_t)g * 0x9E3779B97F4A7C15ull; }

template <int MODE, typename ObsT, int T>
__global__ void __launch_bounds__(T)
env_group_kernel(EnvGroups gs, uint64_t seed, uint64_t ctr) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    // Blocks in dispatch order, the classes laid out most expensive first (launch_groups): no XCD-major
    // remap here -- it put whole classes on a few XCDs (1024 mixed envs: 29.3 -> 19.4 us without it)
    const int gb = blockIdx.x;
    int g = 0;
#pragma unroll
    for (int k = 1; k < MSAT_MAX_GROUPS; ++k)
        if (k < gs.G && gb >= gs.g[k].begin) g = k;
    const EnvGroup &e = gs.g[g];
    const ClockStamp cs(e.out.clock_stamps, gb - e.begin);
    env_run<MODE, ObsT, T>(e.p, e.pool, e.st, e.actions, nullptr, nullptr, nullptr, seed ^ group_seed(e.gid), ctr, e.out,
                        reinterpret_cast<ObsT *>(e.obs), gb - e.begin, smem, cs);
    cs.finish();
}

// ------------------------------------------------------------- host glue ----

// The reset-queue role of a launch on state st (EnvParams::rq_mode): the autoreset step of the sparse reward mode
// consumes and produces it; every other state-modifying launch clears the entries of the envs it touches.
static int set_reset_queue(EnvParams *p, const msat_env_state *st, int mode) {
    p->rq_mode = 0;
    p->rq_cap = rq_capacity(p->B);
    if (st->reset_queue == nullptr || mode == kModeObs) return MSAT_OK;
    MSAT_REQUIRE((reinterpret_cast<uintptr_t>(st->reset_queue) & 15) == 0, "reset_queue must be 16-byte aligned");
    if (MSAT_DEBUG_BUILD)
        MSAT_REQUIRE(dbg_extent(st->reset_queue, 4) >= (long long)rq_words(p->B),
                     "MSAT_DEBUG: reset_queue smaller than msat_reset_queue_words(%d)", p->B);
    p->rq_serial = st->reset_serial;
    // the fast path reads an env's entry in its action load (mode 0, A < 64) and scans the entries 16 bytes at a time
    p->rq_mode = (mode == kModeStepAutoReset && p->reward_mode == MSAT_REWARD_SPARSE && p->action_mode == 0 &&
                  p->A < 64 && p->B % 4 == 0) ? 1 : 2;
    return MSAT_OK;
}

// debug builds: the extents of the launch's caller buffers (EnvParams::dbg_*)
static void set_dbg_extents(EnvParams *p, const msat_env_state *st, const int32_t *actions, const void *obs,
                            int obs_dtype) {
    if (!MSAT_DEBUG_BUILD) return;
    p->dbg_obs = dbg_extent(obs, obs_dtype == MSAT_OBS_I32 ? 4 : 1);
    p->dbg_assign = dbg_extent(st->assign, 1);
    p->dbg_sat = dbg_extent(st->clause_sat, 1);
    p->dbg_ntrue = dbg_extent(st->clause_ntrue, 1);
    p->dbg_actions = dbg_extent(actions, 4);
}

// MARLSAT_ENV_THREADS (64 / 128 / 256 / 512), read once per process: forces both width rules below; 0 if unset
static int env_threads_forced() {
    static const int forced = [] {
        const char *e = getenv("MARLSAT_ENV_THREADS");
        const int v = e ? atoi(e) : 0;
        return v == 64 || v == 128 || v == 256 || v == 512 ? v : 0;
    }();
    return forced;
}

// Workgroup size of the single-class env kernel.  Two rules, MARLSAT_ENV_THREADS overriding both:
//  - env_threads: the launches WITHOUT an obs shadow (the full observation write; msat_env_launch_threads, the bench
//    line's roofline.kernel label).  One wave per env for small instances (more envs resident per CU: the per-env
//    chain of dependent memory round trips, not bandwidth, bounds them), 512 lanes for large ones (A * D >= 16384:
//    uf200), 256 otherwise.
//  - env_delta_threads: the launches WITH an obs shadow (shadow::env_kernel; msat_env_delta_launch_threads).  Where
//    the delta write is the default (A * D >= 16384, int32) a width of its own; everywhere else env_threads.
static int env_threads(const EnvParams &p) {
    if (const int forced = env_threads_forced()) return forced;
    // Fewer lanes per env as the batch grows (more envs resident per CU), more while each env's chain bounds the
    // launch (a few envs per CU).  uf50: x 1024 7.57 us at 128 vs 7.86 at 64, 7.88 at 256; x 2048 9.86 at 64 vs 10.1
    // at 128; x 4096 14.1 at 64 vs 16.6 at 128.  uf100: x 1024 11.0 at 256 vs 11.6 at 128, 14.6 at 64; x 2048 15.3 at
    // 128 vs 16.6 at 256; x 4096 25.8 at 128 vs 26.3 at 256.  uf200 x 4096: 107 at 512 vs 109 at 256, 142 at 64
    // (profiles/r06/r06t_*, r06u_*, r06w_*, r06x_*)
    const long n = (long)p.A * p.D;
    if (n >= 16384) return 512;
    if (n > 4096) return p.B <= 1024 ? 256 : 128;
    return p.B <= 1024 ? 128 : 64;
}

// A delta launch moves a fraction of the full write's bytes and is bound by how many of its workgroups' dependent
// chains a CU runs one after the other: 256 lanes at 8 waves per SIMD hold 8 envs per CU where 512 lanes hold 4
// (uf200 x 4096: 16 step workgroups per CU in two rounds instead of four; figures: DESIGN.md section 4, round 10,
// profiles/r10/ab_widths.txt).  int8 and the shapes below A * D = 16384 (forced delta) were not measured: they keep
// the plain rule's width.
static int env_delta_threads(const EnvParams &p, int obs_dtype) {
    if (const int forced = env_threads_forced()) return forced;
    if ((long)p.A * p.D >= 16384 && obs_dtype == MSAT_OBS_I32) return 256;
    return env_threads(p);
}

// f(ObsT{}, std::integral_constant<int, W>{}) for the launch's obs dtype and its workgroup size W: the one of
// T0, Ts... equal to T, or the last of them
template <int T0, int... Ts, typename F>
static void for_width_dtype(int T, int obs_dtype, F f) {
    if constexpr (sizeof...(Ts) > 0) {
        if (T != T0) return for_width_dtype<Ts...>(T, obs_dtype, f);
    }
    if (obs_dtype == MSAT_OBS_I32)
        f(int32_t{}, std::integral_constant<int, T0>{});
    else
        f(int8_t{}, std::integral_constant<int, T0>{});
}

// The shapes shadow::env_kernel is also compiled for (int32 observations, the delta rule's 256 lanes): uf200-860 with
// 25 agents, the bench's headline shape.  MSAT_STATIC_ALL_WIDTHS: A/B builds only (make ab), the same at every width.
using StaticUf200 = StaticShape<200, 860, 25>;
#ifndef MSAT_STATIC_ALL_WIDTHS
#define MSAT_STATIC_ALL_WIDTHS 0
#endif

// MARLSAT_ENV_STATIC=0, read once per process: every launch takes the kernel of any shape
static bool env_static_enabled() {
    static const bool on = [] {
        const char *e = getenv("MARLSAT_ENV_STATIC");
        return !(e && e[0] == '0' && e[1] == '\0');
    }();
    return on;
}

// Whether a launch with an obs shadow, these parameters, this obs dtype and T lanes takes StaticUf200's kernel: the
// run-time geometry equals the shape's constants field by field
static bool takes_static_shape(const EnvParams &p, int obs_dtype, int T) {
    return env_static_enabled() && obs_dtype == MSAT_OBS_I32 && (T == 256 || MSAT_STATIC_ALL_WIDTHS) &&
           shape_matches<StaticUf200>(p);
}

// One (MODE, ObsT, T) launch: shadow::env_kernel for a step with an obs shadow (modes 1 and 2 alone have that
// kernel; the one of StaticUf200 where takes_static_shape), env_kernel otherwise
template <int MODE, typename ObsT, int T>
static void launch_env_kernel(int grid, size_t lds, hipStream_t s, const EnvParams &p, const msat_pool &pool,
                              const msat_env_state &st, const int32_t *actions, const uint8_t *mask,
                              const int32_t *npidx, const uint8_t *nassign, uint64_t seed, uint64_t ctr,
                              const msat_step_out &o, void *obs, const ObsShadowArg &sa) {
    if constexpr (MODE == kModeStep || MODE == kModeStepAutoReset) {
        if (sa.rows != nullptr) {
            if constexpr (std::is_same<ObsT, int32_t>::value && (T == 256 || MSAT_STATIC_ALL_WIDTHS)) {
                if (takes_static_shape(p, MSAT_OBS_I32, T)) {
                    hipLaunchKernelGGL((shadow::env_kernel<MODE, ObsT, T, StaticUf200>), dim3(grid), dim3(T), lds, s,
                                       p, pool, st, actions, mask, npidx, nassign, seed, ctr, o, (ObsT *)obs, sa.rows,
                                       sa.g);
                    return;
                }
            }
            hipLaunchKernelGGL((shadow::env_kernel<MODE, ObsT, T>), dim3(grid), dim3(T), lds, s, p, pool, st, actions,
                               mask, npidx, nassign, seed, ctr, o, (ObsT *)obs, sa.rows, sa.g);
            return;
        }
    }
    hipLaunchKernelGGL((env_kernel<MODE, ObsT, T>), dim3(grid), dim3(T), lds, s, p, pool, st, actions, mask, npidx,
                       nassign, seed, ctr, o, (ObsT *)obs);
}

template <int MODE>
static int launch_env(const EnvParams &p, const msat_env_desc *d, const msat_pool *pool,
                      const msat_env_state *st, const int32_t *actions, const uint8_t *mask,
                      const int32_t *npidx, const uint8_t *nassign, uint64_t seed, uint64_t ctr,
                      const msat_step_out *out, void *obs, hipStream_t s, uint32_t *shadow = nullptr,
                      int delta_g = 0) {
    EnvParams pd = p;  // + the buffer extents in debug builds, the reset queue's role
    // the obs shadow: MARLSAT_ABLATE's obs ablations do not write the observation the rows would describe, so such a
    // launch leaves them alone -- the rows mean nothing after an ablated launch (diagnostics only)
    ObsShadowArg sa{nullptr, 0};
    if ((p.ablate & 3) == 0 && shadow != nullptr) sa = ObsShadowArg{shadow, delta_g};
    if (MSAT_DEBUG_BUILD && sa.rows != nullptr)
        MSAT_REQUIRE(dbg_extent(sa.rows, 4) >= (long long)p.B * shadow_row_words(p),
                     "MSAT_DEBUG: obs_shadow smaller than msat_obs_shadow_words()");
    const size_t lds = env_lds_words(pd, sa.rows != nullptr) * 4;
    MSAT_REQUIRE(lds <= 160 * 1024, "env needs %zu B of LDS (> 160 KiB)", lds);
    msat_step_out o{};
    if (out) o = *out;
    if (p.B == 0) return MSAT_OK;
    const int T = sa.rows != nullptr ? env_delta_threads(p, d->obs_dtype) : env_threads(p);
    set_dbg_extents(&pd, st, actions, obs, d->obs_dtype);
    if (int rc = set_reset_queue(&pd, st, MODE)) return rc;
    // the reset workgroups of a queue-consuming launch come first (block ids 0 .. cap - 1)
    const int grid = p.B + (pd.rq_mode == 1 ? pd.rq_cap : 0);
    for_width_dtype<64, 128, 512, 256>(T, d->obs_dtype, [&](auto obs_t, auto width) {
        launch_env_kernel<MODE, decltype(obs_t), decltype(width)::value>(grid, lds, s, pd, *pool, *st, actions, mask,
                                                                         npidx, nassign, seed, ctr, o, obs, sa);
    });
    return check_launch("env_kernel");
}

// Workgroup size of the grouped launch: 512 lanes for small batches (<= 2048 envs over all classes: the launch is
// bound by one large env's latency; mixed 1024: 15.7 vs 16.9 us), 256 otherwise (mixed 8192: 91.5-96.9 vs 105.5 us
// on 512); MARLSAT_ENV_GROUP_THREADS (256 / 512 / 1024) overrides
static int group_threads(int total) {
    static const int forced = [] {
        const char *e = getenv("MARLSAT_ENV_GROUP_THREADS");
        const int v = e ? atoi(e) : 0;
        return v == 256 || v == 512 || v == 1024 ? v : 0;
    }();
    return forced ? forced : (total <= 2048 ? 512 : 256);
}

template <int MODE>
static int launch_groups(int G, const msat_env_desc *descs, const msat_pool *pools, const msat_env_state *states,
                         const int32_t *const *actions, uint64_t seed, uint64_t ctr, const msat_step_out *outs,
                         void *const *obs, hipStream_t s) {
    MSAT_REQUIRE(G >= 1 && G <= MSAT_MAX_GROUPS, "num_groups %d out of [1,%d]", G, MSAT_MAX_GROUPS);
    MSAT_REQUIRE(descs && pools && states && obs, "NULL group arrays");
    MSAT_REQUIRE(MODE == kModeReset || (actions && outs), "NULL actions / outs");
    EnvGroups gs{};
    gs.G = G;
    size_t lds = 0;
    int total = 0;
    // block layout: classes by descending per-env obs size (A * D), so the longest envs are dispatched
    // first and the small ones fill in behind them (stable for equal sizes)
    int order[MSAT_MAX_GROUPS];
    long cost[MSAT_MAX_GROUPS];
    for (int g = 0; g < G; ++g) {
        order[g] = g;
        cost[g] = (long)descs[g].num_agents * (2L * descs[g].num_vars + descs[g].num_clauses);
    }
    std::stable_sort(order, order + G, [&](int x, int y) { return cost[x] > cost[y]; });
    for (int pos = 0; pos < G; ++pos) {
        const int g = order[pos];
        EnvGroup &e = gs.g[pos];
        e.gid = g;
        int rc = make_params(&descs[g], &e.p);
        if (rc) return rc;
        e.begin = total;
        if (e.p.B == 0) continue;  // empty class: no blocks (its pointers may be NULL)
        if ((rc = check_state(&states[g])) || (rc = check_pool(&pools[g]))) return rc;
        MSAT_REQUIRE(descs[g].obs_dtype == descs[0].obs_dtype, "groups must share obs_dtype");
        MSAT_REQUIRE(obs[g], "NULL obs for group %d", g);
        e.pool = pools[g];
        e.st = states[g];
        e.actions = MODE == kModeReset ? nullptr : actions[g];
        if (MODE != kModeReset) {
            MSAT_REQUIRE(e.actions && outs[g].reward && outs[g].done && outs[g].solved, "NULL step I/O, group %d", g);
            e.out = outs[g];
        }
        e.obs = obs[g];
        set_dbg_extents(&e.p, &e.st, e.actions, e.obs, descs[g].obs_dtype);
        // the grouped launch keeps every reset in its step workgroup: it only clears the queue's entries
        if ((rc = set_reset_queue(&e.p, &e.st, MODE))) return rc;
        if (e.p.rq_mode == 1) e.p.rq_mode = 2;
        total += e.p.B;
        lds = std::max(lds, env_lds_words(e.p) * 4);
        gs.ablate = e.p.ablate;
    }
    MSAT_REQUIRE(lds <= 160 * 1024, "env needs %zu B of LDS (> 160 KiB)", lds);
    gs.total = total;
    if (total == 0) return MSAT_OK;
    for_width_dtype<1024, 512, 256>(group_threads(total), descs[0].obs_dtype, [&](auto obs_t, auto width) {
        hipLaunchKernelGGL((env_group_kernel<MODE, decltype(obs_t), decltype(width)::value>), dim3(total),
                           dim3(decltype(width)::value), lds, s, gs, seed, ctr);
    });
    return check_launch("env_group_kernel");
}

}  // namespace msat

using namespace msat;

extern "C" int msat_env_reset_grouped(int32_t num_groups, const msat_env_desc *descs, const msat_pool *pools,
                                      const msat_env_state *states, uint64_t seed, uint64_t rng_counter,
                                      void *const *obs, void *stream) {
    return launch_groups<kModeReset>(num_groups, descs, pools, states, nullptr, seed, rng_counter, nullptr, obs,
                                     (hipStream_t)stream);
}

extern "C" int msat_env_step_grouped(int32_t num_groups, const msat_env_desc *descs, const msat_pool *pools,
                                     const msat_env_state *states, const int32_t *const *actions, int32_t autoreset,
                                     uint64_t seed, uint64_t rng_counter, const msat_step_out *outs, void *const *obs,
                                     void *stream) {
    if (autoreset)
        return launch_groups<kModeStepAutoReset>(num_groups, descs, pools, states, actions, seed, rng_counter, outs,
                                                 obs, (hipStream_t)stream);
    return launch_groups<kModeStep>(num_groups, descs, pools, states, actions, seed, rng_counter, outs, obs,
                                    (hipStream_t)stream);
}

// The workgroup sizes the launches above use (host-only; tests and labels name the instantiation that ran)
extern "C" int msat_env_launch_threads(const msat_env_desc *desc) {
    EnvParams p;
    if (int rc = make_params(desc, &p)) return rc;
    return env_threads(p);
}

extern "C" int msat_env_delta_launch_threads(const msat_env_desc *desc) {
    EnvParams p;
    if (int rc = make_params(desc, &p)) return rc;
    return env_delta_threads(p, desc->obs_dtype);
}

extern "C" int msat_env_static_shape(const msat_env_desc *desc) {
    EnvParams p;
    if (make_params(desc, &p)) return 0;
    return takes_static_shape(p, desc->obs_dtype, env_delta_threads(p, desc->obs_dtype)) ? 1 : 0;
}

extern "C" int msat_env_group_launch_threads(int32_t total_envs) {
    MSAT_REQUIRE(total_envs >= 0, "total_envs %d < 0", total_envs);
    return group_threads(total_envs);
}

extern "C" size_t msat_reset_queue_words(int32_t num_envs) { return num_envs < 0 ? 0 : rq_words(num_envs); }

extern "C" int msat_env_reset(const msat_env_desc *desc, const msat_pool *pool,
                              const msat_env_state *state, const uint8_t *reset_mask,
                              const int32_t *new_problem_idx, const uint8_t *new_assign,
                              uint64_t seed, uint64_t rng_counter, void *obs, void *stream) {
    EnvParams p;
    if (int rc = env_entry(desc, state, pool, &p)) return rc;
    if (p.B == 0) return MSAT_OK;
    return launch_env<kModeReset>(p, desc, pool, state, nullptr, reset_mask, new_problem_idx, new_assign,
                                  seed, rng_counter, nullptr, obs, (hipStream_t)stream);
}

extern "C" int msat_env_step(const msat_env_desc *desc, const msat_pool *pool,
                             const msat_env_state *state, const int32_t *actions, int32_t autoreset,
                             const int32_t *new_problem_idx, const uint8_t *new_assign, uint64_t seed,
                             uint64_t rng_counter, const msat_step_out *out, void *obs, void *stream) {
    // a step without an obs shadow: the same checks in the same order, and launch_env's plain kernels
    return msat_env_step_delta(desc, pool, state, actions, autoreset, new_problem_idx, new_assign, seed, rng_counter,
                               out, obs, nullptr, 0, stream);
}

extern "C" size_t msat_obs_shadow_words(const msat_env_desc *desc) {
    EnvParams p;
    if (make_params(desc, &p)) return 0;
    return (size_t)p.B * shadow_row_words(p);
}

extern "C" int msat_env_step_delta(const msat_env_desc *desc, const msat_pool *pool, const msat_env_state *state,
                                   const int32_t *actions, int32_t autoreset, const int32_t *new_problem_idx,
                                   const uint8_t *new_assign, uint64_t seed, uint64_t rng_counter,
                                   const msat_step_out *out, void *obs, uint32_t *obs_shadow,
                                   int32_t delta_group_bytes, void *stream) {
    EnvParams p;
    int rc = make_params(desc, &p);
    if (rc) return rc;
    MSAT_REQUIRE(delta_group_bytes == 0 || delta_group_bytes == 16 || delta_group_bytes == 64 ||
                     delta_group_bytes == 128,
                 "delta_group_bytes %d not 0, 16, 64 or 128", delta_group_bytes);
    MSAT_REQUIRE(obs_shadow == nullptr || obs != nullptr, "obs_shadow given with NULL obs");
    MSAT_REQUIRE((reinterpret_cast<uintptr_t>(obs_shadow) & 3) == 0, "obs_shadow must be 4-byte aligned");
    if (p.B == 0) return MSAT_OK;
    if ((rc = check_state(state)) || (rc = check_pool(pool))) return rc;
    MSAT_REQUIRE(actions, "NULL actions");
    MSAT_REQUIRE(out && out->reward && out->done && out->solved, "NULL step outputs");
    if (autoreset)
        return launch_env<kModeStepAutoReset>(p, desc, pool, state, actions, nullptr, new_problem_idx, new_assign,
                                              seed, rng_counter, out, obs, (hipStream_t)stream, obs_shadow,
                                              delta_group_bytes);
    return launch_env<kModeStep>(p, desc, pool, state, actions, nullptr, nullptr, nullptr, seed, rng_counter, out,
                                 obs, (hipStream_t)stream, obs_shadow, delta_group_bytes);
}

extern "C" int msat_env_obs(const msat_env_desc *desc, const msat_pool *pool, const msat_env_state *state,
                            void *obs, void *stream) {
    EnvParams p;
    if (int rc = env_entry(desc, state, pool, &p)) return rc;
    if (p.B == 0) return MSAT_OK;
    MSAT_REQUIRE(obs, "NULL obs");
    return launch_env<kModeObs>(p, desc, pool, state, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, obs,
                                (hipStream_t)stream);
}

