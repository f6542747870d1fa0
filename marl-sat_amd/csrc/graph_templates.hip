// The GNN's graph templates of a problem pool on the device (include/marlsat_net.h, msat_graph_template_counts /
// msat_graph_template_fill): the twelve arrays of learners/graphs.py::Templates, element for element what
// build_templates makes on the host.  Cold, but the hot part of a pool refresh: once per pool.
//
// One workgroup per instance, the same kernel as a count pass (FILL = false: gv, gc, ge) and a fill pass (the row
// arrays, at the offsets the caller scanned from the counts).  Per instance, in LDS:
//   codes  [3C] u16   literal slot -> (var << 1) | neg, 0xFFFF for literal 0, a column past K, or |l| > V
//   vptr   [V + 1]    CSR over variables of their real occurrences
//   occ    [3C]       the occurrences (clause << 2) | slot, per variable ascending = (clause, slot) order; filled
//                     through an atomic cursor into `tmp`, then every entry finds its rank among its variable's
//                     (distinct values: a count of smaller ones), so no order depends on the atomics
//   relw / nbrw       per graph: related-clause and neighbour-variable bitmaps, relpre / nbrpre their per-word
//                     popcount prefixes: the row of a clause or a neighbour within its graph is a popcount prefix
//   cnt    [V]        the cursor of the fill above; per graph the neighbours' incidence counts, then their scan
// Graph 0 is every variable and clause in order.  Graph 1 + i: own variables lo .. lo + n - 1 in order, then the
// neighbours ascending; clauses the related ones ascending.  An own variable's incidences are all its occurrences
// (each of its clauses is related), a neighbour's those in related clauses.  The adjacency is the network's:
// literal 0 names no variable and adds no edge.
#include "common.h"

namespace msat {

constexpr int kGtThreads = 256;
constexpr uint32_t kGtNull = 0xFFFFu;
constexpr size_t kGtLdsLimit = 65536;  // the bound msat_walksat uses

struct GtPlan {
    int WC, WV;
    size_t codes, vptr, cnt, tmp, occ, relw, relpre, nbrw, nbrpre, scr, bytes;  // byte offsets
};

static GtPlan gt_plan(int V, int C) {
    GtPlan p;
    p.WC = (C + 31) / 32;
    p.WV = (V + 31) / 32;
    size_t o = 0;
    auto take = [&o](size_t words) {
        const size_t at = o;
        o += 4 * words;
        return at;
    };
    p.vptr = take((size_t)V + 1);
    p.cnt = take((size_t)V);
    p.tmp = take(3 * (size_t)C);
    p.occ = take(3 * (size_t)C);
    p.relw = take((size_t)p.WC);
    p.relpre = take((size_t)p.WC + 1);
    p.nbrw = take((size_t)p.WV);
    p.nbrpre = take((size_t)p.WV + 1);
    p.scr = take((size_t)kGtThreads + 1);
    p.codes = take((3 * (size_t)C + 1) / 2);
    p.bytes = (o + 15) & ~(size_t)15;
    return p;
}

struct GtArgs {
    const int32_t *clauses;  // (N, C, K)
    int N, C, K, V, A;
    int32_t *gv, *gc, *ge;                        // (N, A + 2), written by the count pass
    const int32_t *voff, *coff, *eoff, *poff;      // (N + 1,), read by the fill pass
    int32_t *vgid, *cgid, *slots, *ptr, *inc;      // the fill pass's outputs
    long long tv, tc, te;                          // their row counts (debug-build bounds)
    unsigned o_codes, o_vptr, o_cnt, o_tmp, o_occ, o_relw, o_relpre, o_nbrw, o_nbrpre, o_scr;
    int WC, WV;
};

// Exclusive scan of a[0 .. n) in place; the total to every lane.  scr: kGtThreads + 1 ints.
__device__ int gt_scan(int *a, int n, int *scr) {
    const int tid = threadIdx.x;
    const int per = (n + kGtThreads - 1) / kGtThreads;
    const int b = min(tid * per, n), e = min(b + per, n);
    int s = 0;
    for (int i = b; i < e; ++i) s += a[i];
    scr[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < kGtThreads; ++t) {
            const int x = scr[t];
            scr[t] = run;
            run += x;
        }
        scr[kGtThreads] = run;
    }
    __syncthreads();
    int run = scr[tid];
    for (int i = b; i < e; ++i) {
        const int x = a[i];
        a[i] = run;
        run += x;
    }
    __syncthreads();
    return scr[kGtThreads];
}

__device__ __forceinline__ bool gt_bit(const uint32_t *w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }
// set bits of bitmap w below position i, pre its per-word popcount prefix
__device__ __forceinline__ int gt_rank(const uint32_t *w, const int *pre, int i) {
    return pre[i >> 5] + __popc(w[i >> 5] & ((1u << (i & 31)) - 1u));
}

template <bool FILL>
__global__ void __launch_bounds__(kGtThreads) graph_templates_kernel(GtArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gt_smem[];
    const int V = g.V, C = g.C, K = g.K, A = g.A, WC = g.WC, WV = g.WV;
    uint16_t *codes = reinterpret_cast<uint16_t *>(gt_smem + g.o_codes);
    int *vptr = reinterpret_cast<int *>(gt_smem + g.o_vptr);
    int *cnt = reinterpret_cast<int *>(gt_smem + g.o_cnt);
    uint32_t *tmp = reinterpret_cast<uint32_t *>(gt_smem + g.o_tmp);
    uint32_t *occ = reinterpret_cast<uint32_t *>(gt_smem + g.o_occ);
    uint32_t *relw = reinterpret_cast<uint32_t *>(gt_smem + g.o_relw);
    int *relpre = reinterpret_cast<int *>(gt_smem + g.o_relpre);
    uint32_t *nbrw = reinterpret_cast<uint32_t *>(gt_smem + g.o_nbrw);
    int *nbrpre = reinterpret_cast<int *>(gt_smem + g.o_nbrpre);
    int *scr = reinterpret_cast<int *>(gt_smem + g.o_scr);
    const int n = blockIdx.x, tid = threadIdx.x;
    const int32_t *cl = g.clauses + (size_t)n * C * K;
    const int S = 3 * C;  // literal slots, three per clause whatever K

    // ---- the instance: slot codes, per-variable occurrence lists in (clause, slot) order
    for (int v = tid; v < V; v += kGtThreads) cnt[v] = 0;
    __syncthreads();
    for (int s = tid; s < S; s += kGtThreads) {
        const int c = s / 3, k = s - 3 * c;
        uint32_t code = kGtNull;
        if (k < K) {
            const int l = cl[(size_t)c * K + k];
            const int a = l < 0 ? -l : l;
            if (l != 0 && l != INT_MIN && a <= V) {
                code = ((uint32_t)(a - 1) << 1) | (l < 0 ? 1u : 0u);
                atomicAdd(&cnt[a - 1], 1);
            }
        }
        codes[s] = (uint16_t)code;
    }
    __syncthreads();
    for (int v = tid; v < V; v += kGtThreads) vptr[v] = cnt[v];
    __syncthreads();
    const int E0 = gt_scan(vptr, V, scr);  // real literal slots = graph 0's incidences
    if (tid == 0) vptr[V] = E0;
    for (int v = tid; v < V; v += kGtThreads) cnt[v] = 0;
    __syncthreads();
    for (int s = tid; s < S; s += kGtThreads) {
        const uint32_t code = codes[s];
        if (code == kGtNull) continue;
        const int v = (int)(code >> 1), c = s / 3;
        tmp[vptr[v] + atomicAdd(&cnt[v], 1)] = ((uint32_t)c << 2) | (uint32_t)(s - 3 * c);
    }
    __syncthreads();
    for (int p = tid; p < E0; p += kGtThreads) {
        const uint32_t e = tmp[p];
        const int v = (int)(codes[3 * (e >> 2) + (e & 3u)] >> 1);
        const int b = vptr[v], end = vptr[v + 1];
        int r = 0;
        for (int q = b; q < end; ++q) r += tmp[q] < e;
        occ[b + r] = e;
    }
    __syncthreads();

    const int base = V / A, rem = V - base * A;
    int vr = 0, cr = 0, eg = 0;  // var rows, clause rows, incidences of the graphs before this one
    const long long vo = FILL ? g.voff[n] : 0, co = FILL ? g.coff[n] : 0, eo = FILL ? g.eoff[n] : 0,
                    po = FILL ? g.poff[n] : 0;
    int32_t *gvn = FILL ? nullptr : g.gv + (size_t)n * (A + 2);
    int32_t *gcn = FILL ? nullptr : g.gc + (size_t)n * (A + 2);
    int32_t *gen = FILL ? nullptr : g.ge + (size_t)n * (A + 2);

    for (int gr = 0; gr <= A; ++gr) {
        const int i = gr - 1;
        const int lo = gr == 0 ? 0 : i * base + min(i, rem);
        const int own = gr == 0 ? V : base + (i < rem ? 1 : 0);
        // ---- bitmaps: related clauses, neighbour variables
        for (int w = tid; w < WC; w += kGtThreads) relw[w] = 0u;
        for (int w = tid; w < WV; w += kGtThreads) nbrw[w] = 0u;
        for (int v = tid; v < V; v += kGtThreads) cnt[v] = 0;
        __syncthreads();
        if (gr == 0) {
            for (int c = tid; c < C; c += kGtThreads) atomicOr(&relw[c >> 5], 1u << (c & 31));
        } else {
            // the occurrences of the own variables are one contiguous range of occ
            for (int p = vptr[lo] + tid; p < vptr[lo + own]; p += kGtThreads) {
                const int c = (int)(occ[p] >> 2);
                atomicOr(&relw[c >> 5], 1u << (c & 31));
            }
        }
        __syncthreads();
        if (gr != 0)
            for (int s = tid; s < S; s += kGtThreads) {
                const uint32_t code = codes[s];
                if (code == kGtNull || !gt_bit(relw, s / 3)) continue;
                const int v = (int)(code >> 1);
                if (v >= lo && v < lo + own) continue;
                atomicOr(&nbrw[v >> 5], 1u << (v & 31));
                atomicAdd(&cnt[v], 1);  // a neighbour's incidences: its slots in related clauses
            }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int w = 0; w < WC; ++w) {
                relpre[w] = run;
                run += __popc(relw[w]);
            }
            relpre[WC] = run;
        }
        if (tid == 64) {
            int run = 0;
            for (int w = 0; w < WV; ++w) {
                nbrpre[w] = run;
                run += __popc(nbrw[w]);
            }
            nbrpre[WV] = run;
        }
        __syncthreads();
        const int nc = relpre[WC], nv = own + nbrpre[WV];
        const int ownE = vptr[lo + own] - vptr[lo];
        const int nbrE = gt_scan(cnt, V, scr);  // cnt[v]: incidences of the neighbours below v
        if (!FILL) {
            if (tid == 0) {
                gvn[gr] = vr;
                gcn[gr] = cr;
                gen[gr] = eg;
            }
        } else {
            // ---- var rows: global id, CSR pointer, incidences (clause row << 1 | neg) in (clause, slot) order
            for (int v = tid; v < V; v += kGtThreads) {
                const bool mine = v >= lo && v < lo + own;
                if (!mine && !gt_bit(nbrw, v)) continue;
                const int row = vr + (mine ? v - lo : own + gt_rank(nbrw, nbrpre, v));
                int at = eg + (mine ? vptr[v] - vptr[lo] : ownE + cnt[v]);
                MSAT_DCHECK(vo + row, g.tv);
                g.vgid[vo + row] = v;
                g.ptr[po + row] = at;
                for (int p = vptr[v]; p < vptr[v + 1]; ++p) {
                    const uint32_t e = occ[p];
                    const int c = (int)(e >> 2);
                    if (!mine && !gt_bit(relw, c)) continue;
                    MSAT_DCHECK(eo + at, g.te);
                    g.inc[eo + at] = ((cr + gt_rank(relw, relpre, c)) << 1) | (int)(codes[3 * c + (e & 3u)] & 1u);
                    ++at;
                }
            }
            // ---- clause rows: global id, slots (var row << 1 | neg) or -1
            for (int c = tid; c < C; c += kGtThreads) {
                if (!gt_bit(relw, c)) continue;
                const long long row = co + cr + gt_rank(relw, relpre, c);
                MSAT_DCHECK(row, g.tc);
                g.cgid[row] = c;
                for (int k = 0; k < 3; ++k) {
                    const uint32_t code = codes[3 * c + k];
                    int32_t s = -1;
                    if (code != kGtNull) {
                        const int v = (int)(code >> 1);
                        const bool mine = v >= lo && v < lo + own;
                        s = ((vr + (mine ? v - lo : own + gt_rank(nbrw, nbrpre, v))) << 1) | (int)(code & 1u);
                    }
                    g.slots[row * 3 + k] = s;
                }
            }
        }
        vr += nv;
        cr += nc;
        eg += ownE + nbrE;
        __syncthreads();  // the bitmaps and cnt are read to here; the next graph rewrites them
    }
    if (tid == 0) {
        if (!FILL) {
            gvn[A + 1] = vr;
            gcn[A + 1] = cr;
            gen[A + 1] = eg;
        } else {
            g.ptr[po + vr] = eg;  // the CSR's last entry: vr + 1 per instance
        }
    }
}

static int gt_launch(bool fill, GtArgs &g, void *stream) {
    MSAT_REQUIRE(g.N >= 0, "graph_templates: num_problems %d < 0", g.N);
    MSAT_REQUIRE(g.V >= 1 && g.V <= 32000, "graph_templates: num_vars %d outside [1, 32000]", g.V);
    MSAT_REQUIRE(g.C >= 1, "graph_templates: num_clauses %d < 1", g.C);
    MSAT_REQUIRE(g.K >= 1 && g.K <= 3, "graph_templates: clause_width %d outside [1, 3]", g.K);
    MSAT_REQUIRE(g.A >= 1 && g.A <= g.V, "graph_templates: num_agents %d outside [1, num_vars %d]", g.A, g.V);
    const size_t need = msat_graph_templates_lds_bytes(g.V, g.C, g.K);
    MSAT_REQUIRE(need != 0 && need <= kGtLdsLimit, "graph_templates: V %d, C %d need %zu B of LDS, more than %zu", g.V,
                 g.C, need, kGtLdsLimit);
    if (g.N == 0) return MSAT_OK;
    MSAT_REQUIRE(g.clauses, "graph_templates: NULL clauses");
    if (fill) {
        MSAT_REQUIRE(g.voff && g.coff && g.eoff && g.poff, "graph_templates: NULL offset array");
        MSAT_REQUIRE(g.tv >= 0 && g.tc >= 0 && g.te >= 0, "graph_templates: negative row total");
        MSAT_REQUIRE(g.vgid && g.ptr && (g.cgid || g.tc == 0) && (g.slots || g.tc == 0) && (g.inc || g.te == 0),
                     "graph_templates: NULL output array");
    } else {
        MSAT_REQUIRE(g.gv && g.gc && g.ge, "graph_templates: NULL count array");
    }
    const GtPlan p = gt_plan(g.V, g.C);
    g.WC = p.WC;
    g.WV = p.WV;
    g.o_codes = (unsigned)p.codes;
    g.o_vptr = (unsigned)p.vptr;
    g.o_cnt = (unsigned)p.cnt;
    g.o_tmp = (unsigned)p.tmp;
    g.o_occ = (unsigned)p.occ;
    g.o_relw = (unsigned)p.relw;
    g.o_relpre = (unsigned)p.relpre;
    g.o_nbrw = (unsigned)p.nbrw;
    g.o_nbrpre = (unsigned)p.nbrpre;
    g.o_scr = (unsigned)p.scr;
    if (fill)
        hipLaunchKernelGGL(graph_templates_kernel<true>, dim3(g.N), dim3(kGtThreads), p.bytes, (hipStream_t)stream, g);
    else
        hipLaunchKernelGGL(graph_templates_kernel<false>, dim3(g.N), dim3(kGtThreads), p.bytes, (hipStream_t)stream, g);
    return check_launch(fill ? "graph_templates_kernel<fill>" : "graph_templates_kernel<count>");
}

}  // namespace msat

using namespace msat;

extern "C" size_t msat_graph_templates_lds_bytes(int32_t num_vars, int32_t num_clauses, int32_t clause_width) {
    if (num_vars < 1 || num_vars > 32000 || num_clauses < 1 || clause_width < 1 || clause_width > 3) return 0;
    return gt_plan(num_vars, num_clauses).bytes;
}

extern "C" int msat_graph_template_counts(const int32_t *clauses, int32_t num_problems, int32_t num_clauses,
                                          int32_t clause_width, int32_t num_vars, int32_t num_agents, int32_t *gv,
                                          int32_t *gc, int32_t *ge, void *stream) {
    GtArgs g{};
    g.clauses = clauses;
    g.N = num_problems, g.C = num_clauses, g.K = clause_width, g.V = num_vars, g.A = num_agents;
    g.gv = gv, g.gc = gc, g.ge = ge;
    return gt_launch(false, g, stream);
}

extern "C" int msat_graph_template_fill(const int32_t *clauses, int32_t num_problems, int32_t num_clauses,
                                        int32_t clause_width, int32_t num_vars, int32_t num_agents,
                                        const int32_t *voff, const int32_t *coff, const int32_t *eoff,
                                        const int32_t *poff, int32_t total_var_rows, int32_t total_clause_rows,
                                        int32_t total_incidences, int32_t *vgid, int32_t *cgid, int32_t *slots,
                                        int32_t *ptr, int32_t *inc, void *stream) {
    GtArgs g{};
    g.clauses = clauses;
    g.N = num_problems, g.C = num_clauses, g.K = clause_width, g.V = num_vars, g.A = num_agents;
    g.voff = voff, g.coff = coff, g.eoff = eoff, g.poff = poff;
    g.vgid = vgid, g.cgid = cgid, g.slots = slots, g.ptr = ptr, g.inc = inc;
    g.tv = total_var_rows, g.tc = total_clause_rows, g.te = total_incidences;
    return gt_launch(true, g, stream);
}
