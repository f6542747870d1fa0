// The sparse form of the env step's delta observation write (env_kernels.hip, stage_and_write_obs<..., SH>): which
// 16-byte chunks of an env's (A, D) observation block a step changes, and what they hold, derived from the source
// diff (x ^ shadow x, sat ^ shadow sat) and the agent tables alone -- no FM / FX / FD bit images.
//
// Plain C++ (host and device): the kernel runs these functions on LDS words, tests/obs_sparse_check.cpp runs the
// same functions on the host against a brute-force get_obs.  On the device the chunked tasks (sparse_task,
// sparse_entry) serve int8 observations; int32 ones scatter their changed elements one by one (scatter_obs in
// env_kernels.hip), which uses obs_elem (debug read-back) and the carried task index of this file.
// env_kernels.hip, the step / reset / obs kernel family, is this header's only device user.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MSAT_OS_HD __host__ __device__ __forceinline__
#else
#define MSAT_OS_HD inline
#endif

namespace msat {

// What the observation layout needs of EnvParams (env_params.h; env:345-398): row i, element k: k < V own vars, V <= k < V + C
// clause status, k >= V + C neighbour vars; agent i owns [i*base + min(i, rem), + base + (i < rem)).
struct ObsGeom {
    int V, C, A, D;  // D = 2V + C
    int WV, WC;      // uint32 words per agent row of the nbr / rel tables
    int base, rem;
};

MSAT_OS_HD uint32_t os_low_mask(int n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }
MSAT_OS_HD uint32_t os_bit(const uint32_t *w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }
MSAT_OS_HD int os_min(int a, int b) { return a < b ? a : b; }
MSAT_OS_HD int os_max(int a, int b) { return a > b ? a : b; }

// Element e (flat index into the env's A * D block) from the bit words: -1 (masked), 0 or 1.
MSAT_OS_HD int obs_elem(const ObsGeom &g, const uint32_t *x, const uint32_t *sat, const uint32_t *rel,
                        const uint32_t *nbr, int e) {
    const int i = e / g.D;
    int k = e - i * g.D;
    uint32_t m, v;
    if (k < g.V) {
        const int lo = i * g.base + os_min(i, g.rem), n = g.base + (i < g.rem ? 1 : 0);
        m = (k >= lo && k < lo + n) ? 1u : 0u;
        v = os_bit(x, k);
    } else if ((k -= g.V) < g.C) {
        m = os_bit(rel + (long)i * g.WC, k);
        v = os_bit(sat, k);
    } else {
        k -= g.C;
        m = os_bit(nbr + (long)i * g.WV, k);
        v = os_bit(x, k);
    }
    return m ? (int)v : -1;
}

// One (agent i, source word s) task of a delta step: s < nwV own vars, then nwC clause words, then nwV neighbour
// words (nwV = ceil(V / 32), nwC = ceil(C / 32)).  Positions are "shifted" element indices e + sh, sh = (the block's
// first element's absolute index) mod VEC, so that chunk k is the shifted bits [k VEC, (k + 1) VEC).
struct SparseTask {
    uint64_t dirty;  // bit j: the chunk at shifted index (P & ~31) + j (its first bit) holds a changed element of the task
    int P;           // shifted index of source bit 0
    int len;         // live source bits
    uint32_t m, x;   // the task's mask and value words
};

// False (nothing else set) when the task changes no element.  The diff word is read first: a task whose source word
// did not change loads no mask.
template <int VEC>
MSAT_OS_HD bool sparse_task(const ObsGeom &g, int i, int s, const uint32_t *x, const uint32_t *sat,
                            const uint32_t *sx, const uint32_t *ssat, const uint32_t *rel, const uint32_t *nbr,
                            int sh, SparseTask &k) {
    // (selects, not branches: the lanes of a wave hold consecutive s, i.e. all three regions at once)
    const int nwV = (g.V + 31) >> 5, nwC = (g.C + 31) >> 5;
    const bool own = s < nwV, cl = !own && s < nwV + nwC;  // else neighbour vars
    const int r = own ? s : cl ? s - nwV : s - nwV - nwC;  // word of the region's source
    k.x = (cl ? sat : x)[r];
    const uint32_t diff = k.x ^ (cl ? ssat : sx)[r];
    if (diff == 0) return false;
    const int lo = i * g.base + os_min(i, g.rem) - 32 * r, hi = lo + g.base + (i < g.rem ? 1 : 0);
    const int a = os_max(lo, 0), z = os_min(hi, 32);
    const uint32_t own_m = z > a ? (os_low_mask(z) & ~os_low_mask(a)) : 0u;
    const uint32_t tbl_m = (cl ? rel + (long)i * g.WC : nbr + (long)i * g.WV)[r];  // (own: r < nwV, a valid nbr word)
    k.m = own ? own_m : tbl_m;
    k.len = os_min(32, (cl ? g.C : g.V) - 32 * r);
    const int off = 32 * r + (own ? 0 : cl ? g.V : g.V + g.C);
    const uint32_t fd = diff & k.m & os_low_mask(k.len);
    if (fd == 0) return false;
    k.P = i * g.D + off + sh;
    uint64_t f = (uint64_t)fd << (k.P & 31);
    if (VEC == 4) {  // one bit per dirty chunk, at the chunk's first bit
        f |= f >> 1;
        f |= f >> 2;
        f &= 0x1111111111111111ull;
    } else {  // VEC == 16
        uint64_t d = 0;
        for (int c = 0; c < 4; ++c)
            if ((f >> (16 * c)) & 0xFFFFull) d |= 1ull << (16 * c);
        f = d;
    }
    k.dirty = f;
    return true;
}

// The task loop's index: lane `lane` of a T-lane workgroup takes the tasks t = lane, lane + T, lane + 2 T, ... and
// task t is (agent i, source word s) = (t / U, t % U), U = source words per row.  One division for the first pass;
// every later pass adds (T / U, T % U) -- task_stride, the same for every lane -- with one conditional carry.
struct TaskIdx {
    int i, s;
};
MSAT_OS_HD TaskIdx task_first(int lane, int U) {
    const int i = lane / U;
    return TaskIdx{i, lane - i * U};
}
MSAT_OS_HD TaskIdx task_stride(int T, int U) {
    const int q = T / U;
    return TaskIdx{q, T - q * U};
}
MSAT_OS_HD void task_advance(TaskIdx &k, const TaskIdx &stride, int U) {
    k.i += stride.i;
    k.s += stride.s;
    if (k.s >= U) {
        k.s -= U;
        ++k.i;
    }
}

// List entry of the dirty chunk at bit j of k.dirty.  Fast (VEC = 4; bit 31 set): the chunk lies wholly inside the
// task's live source bits, so its mask and value nibbles come from the task's registers:
// 1 | chunk index (23 bits) | mask nibble | value nibble.  Slow: the chunk's shifted first index; whoever stores it
// evaluates its elements with obs_elem.
constexpr uint32_t kSparseFast = 0x80000000u;
template <int VEC>
MSAT_OS_HD uint32_t sparse_entry(const SparseTask &k, int j) {
    const int ec = (k.P & ~31) + j;
    const int r = ec - k.P;
    if (VEC == 4 && r >= 0 && r + VEC <= k.len && (ec >> 2) < (1 << 23))
        return kSparseFast | ((uint32_t)(ec >> 2) << 8) | (((k.m >> r) & 15u) << 4) | ((k.x >> r) & 15u);
    return (uint32_t)ec;
}

}  // namespace msat
