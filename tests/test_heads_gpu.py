"""GPU: the exports of csrc/heads_kernels.hip (pooling, logit assembly, PPO loss, Adam), msat_relu /
msat_relu_bwd and msat_moments / msat_standardize, each called through marlsat._lib on synthetic
inputs (no network) and compared with a plain float64 reference of the same operation.

Two data regimes: "normal" (standard normal fp32, against float64 torch) and "int" (integer-valued
fp32 in {-2..2}: fp32 sums are exact and maxima tie, so sums and maxima are compared bitwise and the
even split of a gradient over tied maxima is pinned).

Bounds (u = 2^-24, the fp32 unit roundoff):
  * a sum of n fp32 terms taken in order: (n - 1) u sum|v|; a mean: (n + 2) u sum|v| / n (one more
    rounding for the division);
  * a value that is copied, selected or made by one fp32 operation: bitwise against numpy float32;
  * an accumulated gradient d0 + g: 4 u (|d0| + |g|) (two divisions, their sum, the add to d0);
  * the PPO loss kernels use __expf / __logf, whose error is not derived: every element of dlogits,
    dvalue and the per-row terms is held to 1e-5 of the tensor's largest reference magnitude, and the
    three sums to 1e-5 relative (the bar of tests/test_gnn_gpu.py::test_ppo_loss_and_grads_match_oracle);
  * Adam: |p - p_ref| <= 2^-23 |p_ref| + 2^-20 |update_ref| (fewer than 16 fp32 roundings in the
    update chain and one in the final add).
"""
import math

import numpy as np
import pytest
import torch

from oracle import net as onet

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NINF = float("-inf")


# ------------------------------------------------------------------ helpers ----
def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def call(name, *args):
    from marlsat import _lib

    _lib.check(getattr(_lib.lib, name)(*args, _lib.stream_ptr()), name)
    torch.cuda.synchronize()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bitwise(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def assert_within(got, ref, bound, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    err = np.abs(got - ref)
    ok = err <= bound  # a NaN fails
    if not ok.all():
        k = np.argmax(np.where(ok, 0.0, np.where(np.isnan(err), np.inf, err / np.maximum(bound, 1e-300))))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} outside the bound; worst at flat index {k}: "
                             f"got {got.flat[k]!r}, ref {ref.flat[k]!r}, bound {bound.flat[k]:.3g}")


def assert_normwise(got, ref, rtol, what):
    ref = np.asarray(ref, np.float64)
    assert_within(got, ref, rtol * max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-300), what)


def data(rng, shape, regime):
    if regime == "int":
        return rng.integers(-2, 3, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def make_layout(rng, nv, nc):
    """vbase / nv / cbase / nc for S samples x G graphs (nv, nc: (S, G) row counts).  The graphs lie in
    shuffled order in the row buffers, with 0-3 unused rows before, between and after them."""
    nv, nc = np.asarray(nv, np.int32), np.asarray(nc, np.int32)
    S, G = nv.shape

    def place(n):
        base = np.zeros(S * G, np.int32)
        pos = int(rng.integers(0, 4))
        for k in rng.permutation(S * G):
            base[k] = pos
            pos += int(n.reshape(-1)[k]) + int(rng.integers(0, 4))
        return base, max(pos, 1)

    vbase, Nv = place(nv)
    cbase, Nc = place(nc)
    lay = {"S": S, "G": G, "Nv": Nv, "Nc": Nc, "vbase": vbase, "nv": nv.reshape(-1), "cbase": cbase,
           "nc": nc.reshape(-1)}
    lay["dev"] = [cu(lay[k]) for k in ("vbase", "nv", "cbase", "nc")]
    return lay


def lay_ptrs(lay):
    return [t.data_ptr() for t in lay["dev"]]


def rows_mask(lay, graphs, which):
    """Boolean mask over the var (which = 'v') or clause rows owned by the listed graph ids."""
    base, n, N = (lay["vbase"], lay["nv"], lay["Nv"]) if which == "v" else (lay["cbase"], lay["nc"], lay["Nc"])
    m = np.zeros(N, bool)
    for k in graphs:
        m[base[k]:base[k] + n[k]] = True
    return m


def mean_bound(absum, n):
    """(n + 2) u sum|v| / n for the fp32 mean of n terms summed in order."""
    n = max(int(n), 1)
    return (n + 2) * U * absum / n


# ------------------------------------------------------------ critic pooling ----
CRITIC_NV = [1, 7, 8, 9, 23]  # n = 1, n < 8, n = 8 (no tail), n % 8 = 1, two unrolled rounds + a tail of 7
CRITIC_NC = [64, 1, 17, 3, 8]  # every unroll-8 tail length class again, paired crosswise with the above


def _critic_case(H, G, regime, seed):
    rng = np.random.default_rng(seed)
    S = 5
    nv = rng.integers(1, 6, (S, G))
    nc = rng.integers(1, 6, (S, G))
    nv[:, 0], nc[:, 0] = CRITIC_NV, CRITIC_NC
    lay = make_layout(rng, nv, nc)
    Hp, Hn, Hc = (data(rng, (lay["Nv"], H), regime), data(rng, (lay["Nv"], H), regime),
                  data(rng, (lay["Nc"], H), regime))
    return rng, lay, Hp, Hn, Hc


def _critic_ref(Hp, Hn, Hc, lay):
    tp, tn, tc = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (Hp, Hn, Hc))
    out, absum = [], []
    for s in range(lay["S"]):
        k = s * lay["G"]
        vb, nv, cb, nc = (int(lay[x][k]) for x in ("vbase", "nv", "cbase", "nc"))
        v = torch.cat([tp[vb:vb + nv], tn[vb:vb + nv]], 1)
        c = tc[cb:cb + nc]
        out.append(torch.cat([v.mean(0), v.amax(0), c.mean(0), c.amax(0)]))
        absum.append((v.detach().abs().sum(0).numpy(), c.detach().abs().sum(0).numpy(), nv, nc))
    return torch.stack(out), (tp, tn, tc), absum


@pytest.mark.parametrize("regime", ["normal", "int"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("H", [64, 128, 256])  # H = 256: 3H = 768 columns, three trips of the block's column loop
def test_critic_pool_forward(H, G, regime):
    rng, lay, Hp, Hn, Hc = _critic_case(H, G, regime, 100 + H + G)
    S = lay["S"]
    pooled = torch.full((S, 6 * H), float("nan"), device="cuda")
    dHp, dHn, dHc = cu(Hp), cu(Hn), cu(Hc)
    call("msat_critic_pool", dHp.data_ptr(), dHn.data_ptr(), dHc.data_ptr(), H, *lay_ptrs(lay), G, S,
         pooled.data_ptr())
    got = host(pooled)
    ref, _, absum = _critic_ref(Hp, Hn, Hc, lay)
    ref = ref.detach().numpy()
    # maxima are selected values: bitwise in both regimes
    assert_bitwise(got[:, 2 * H:4 * H], ref[:, 2 * H:4 * H].astype(np.float32), "max over var rows")
    assert_bitwise(got[:, 5 * H:], ref[:, 5 * H:].astype(np.float32), "max over clause rows")
    for s, (av, ac, nv, nc) in enumerate(absum):
        if regime == "int":  # exact sums, one rounding in the division
            bv, bc = 2 * U * np.abs(ref[s, :2 * H]), 2 * U * np.abs(ref[s, 4 * H:5 * H])
        else:
            bv, bc = mean_bound(av, nv), mean_bound(ac, nc)
        assert_within(got[s, :2 * H], ref[s, :2 * H], bv, f"mean over {nv} var rows (sample {s})")
        assert_within(got[s, 4 * H:5 * H], ref[s, 4 * H:5 * H], bc, f"mean over {nc} clause rows (sample {s})")


@pytest.mark.parametrize("regime", ["normal", "int"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_critic_pool_backward_accumulates(H, G, regime):
    rng, lay, Hp, Hn, Hc = _critic_case(H, G, regime, 200 + H + G)
    S = lay["S"]
    # dmean and dmax of a column share a sign, so |g| = |dmean / n| + |dmax / cnt| on a maximal row: the
    # two parts cannot cancel, and the rounding bound 4 u (|d0| + |g|) below covers both divisions
    sv, sc = rng.choice([-1.0, 1.0], (S, 2 * H)), rng.choice([-1.0, 1.0], (S, H))
    dp = (np.abs(data(rng, (S, 6 * H), regime)) * np.concatenate([sv, sv, sc, sc], 1)).astype(np.float32)
    d0 = [rng.standard_normal(a.shape).astype(np.float32) for a in (Hp, Hn, Hc)]
    dbuf = [cu(a) for a in d0]
    src = [cu(a) for a in (Hp, Hn, Hc)]
    d_dp = cu(dp)
    call("msat_critic_pool_bwd", *(t.data_ptr() for t in src), H, *lay_ptrs(lay), G, S, d_dp.data_ptr(),
         *(t.data_ptr() for t in dbuf))
    ref, leaves, _ = _critic_ref(Hp, Hn, Hc, lay)
    (ref * torch.tensor(dp, dtype=torch.float64)).sum().backward()
    crit = [s * G for s in range(S)]
    ties = 0
    for name, got, base, leaf, which in zip(("dHp", "dHn", "dHc"), dbuf, d0, leaves, "vvc"):
        got, g = host(got), leaf.grad.numpy()
        mine = rows_mask(lay, crit, which)
        # rows in the gaps and rows of the other graphs keep their contents bit for bit
        assert_bitwise(got[~mine], base[~mine], f"{name}: rows outside the critic graphs")
        # rows of the critic graphs receive d0 + gradient (added to, not overwritten)
        assert_within(got[mine], base[mine].astype(np.float64) + g[mine], 4 * U * (np.abs(base[mine]) + np.abs(g[mine])),
                      f"{name}: d0 + gradient")
        assert np.abs(g[mine]).max() > 0
    if regime == "int":
        for s in range(S):
            k = s * G
            for a, b, n in ((Hp, lay["vbase"][k], lay["nv"][k]), (Hn, lay["vbase"][k], lay["nv"][k]),
                            (Hc, lay["cbase"][k], lay["nc"][k])):
                blk = a[b:b + n]
                ties += int(((blk == blk.max(0)).sum(0) > 1).sum())
        assert ties > 0  # tied maxima occurred: the bound above pins dmax / count on each of them


# ------------------------------------------------------------- actor pooling ----
ACTOR_SHAPES = [  # A, base, rem, M
    (3, 7, 2, 8),  # agents of 8, 8, 7: one padded slot
    (1, 9, 0, 9),  # A = 1: sample 0 has no neighbour rows (divisor max(nv - nown, 1))
    (4, 1, 0, 1),  # one own row per agent
    (25, 8, 0, 8),
]
NBR_COUNTS = [0, 1, 13]  # n = 0 (clamped divisor), n = 1, one unrolled round + a tail of 5
CLAUSE_COUNTS = [0, 1, 9]  # nc = 0 for an agent graph, 1, one unrolled round + a tail of 1


def _actor_case(A, base, rem, M, S, E, H, regime, seed):
    rng = np.random.default_rng(seed)
    G = A + 1
    nown = np.array([base + (i < rem) for i in range(A)])
    nv = np.zeros((S, G), np.int64)
    nc = np.zeros((S, G), np.int64)
    nv[:, 0], nc[:, 0] = rng.integers(1, 5, S), rng.integers(1, 4, S)
    for s in range(S):
        for i in range(A):
            nv[s, 1 + i] = nown[i] + NBR_COUNTS[(s + i) % 3]
            nc[s, 1 + i] = CLAUSE_COUNTS[(s + 2 * i + 1) % 3]
    lay = make_layout(rng, nv, nc)
    Hp, Hn, Hc = (data(rng, (lay["Nv"], H), regime), data(rng, (lay["Nv"], H), regime),
                  data(rng, (lay["Nc"], H), regime))
    ide = data(rng, (A, E), regime)
    return rng, lay, nown, Hp, Hn, Hc, ide


def _actor_ref(Hp, Hn, Hc, ide, lay, nown, A, M):
    tp, tn, tc, ti = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (Hp, Hn, Hc, ide))
    H = Hp.shape[1]
    my, ctx, bnd = [], [], []
    for s in range(lay["S"]):
        for i in range(A):
            k = s * lay["G"] + 1 + i
            vb, nv, cb, nc = (int(lay[x][k]) for x in ("vbase", "nv", "cbase", "nc"))
            v = torch.cat([tp[vb:vb + nv], tn[vb:vb + nv]], 1)
            own, nbr, c = v[:nown[i]], v[nown[i]:], tc[cb:cb + nc]
            my.append(torch.cat([own, torch.zeros((M - nown[i], 2 * H), dtype=torch.float64)], 0))
            ctx.append(torch.cat([own.sum(0) / max(nown[i], 1), nbr.sum(0) / max(nv - nown[i], 1),
                                  c.sum(0) / max(nc, 1), ti[i]]))
            bnd.append(np.concatenate([mean_bound(own.detach().abs().sum(0).numpy(), nown[i]),
                                       mean_bound(nbr.detach().abs().sum(0).numpy(), nv - nown[i]),
                                       mean_bound(c.detach().abs().sum(0).numpy(), nc), np.zeros(ide.shape[1])]))
    return torch.stack(my), torch.stack(ctx), np.stack(bnd), (tp, tn, tc)


@pytest.mark.parametrize("regime", ["normal", "int"])
@pytest.mark.parametrize("E,H", [(16, 64), (5, 256)])  # H = 256: 2H = 512 columns, two trips of the column loop
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("A,base,rem,M", ACTOR_SHAPES)
def test_actor_pool_forward(A, base, rem, M, S, E, H, regime):
    rng, lay, nown, Hp, Hn, Hc, ide = _actor_case(A, base, rem, M, S, E, H, regime, 300 + A + S + H)
    my = torch.full((S * A * M, 2 * H), float("nan"), device="cuda")
    ctx = torch.full((S * A, 5 * H + E), float("nan"), device="cuda")
    src = [cu(a) for a in (Hp, Hn, Hc)]
    d_id = cu(ide)
    call("msat_actor_pool", *(t.data_ptr() for t in src), H, *lay_ptrs(lay), A + 1, S, A, M, base, rem,
         d_id.data_ptr(), E, my.data_ptr(), ctx.data_ptr())
    rmy, rctx, bnd, _ = _actor_ref(Hp, Hn, Hc, ide, lay, nown, A, M)
    got_my = host(my).reshape(S * A, M, 2 * H)
    # own rows are copies, padded slots exactly +0 (the NaN fill is gone everywhere)
    assert_bitwise(got_my, rmy.detach().numpy().astype(np.float32), "my_emb")
    got_ctx, rctx = host(ctx), rctx.detach().numpy()
    assert_bitwise(got_ctx[:, 5 * H:], np.tile(ide, (S, 1)), "id embedding")
    if regime == "int":  # exact sums: one rounding in the division (0 / 1 = 0 where the count is 0)
        bnd = 2 * U * np.abs(rctx)
    assert_within(got_ctx[:, :5 * H], rctx[:, :5 * H], bnd[:, :5 * H], "ctx means (divisors clamped at 1)")


@pytest.mark.parametrize("E,H", [(16, 64), (5, 256)])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("A,base,rem,M", ACTOR_SHAPES)
def test_actor_pool_backward_accumulates(A, base, rem, M, S, E, H):
    rng, lay, nown, Hp, Hn, Hc, ide = _actor_case(A, base, rem, M, S, E, H, "normal", 400 + A + S + H)
    # dmy and the own-mean part of dctx share a sign per (row, column): the two parts of an own row's gradient
    # cannot cancel, so 4 u (|d0| + |g|) covers the division, the sum and the add to d0
    sg = rng.choice([-1.0, 1.0], (S * A, 2 * H)).astype(np.float32)
    dmy = np.abs(rng.standard_normal((S * A, M, 2 * H))).astype(np.float32) * sg[:, None, :]
    dctx = rng.standard_normal((S * A, 5 * H + E)).astype(np.float32)
    dctx[:, :2 * H] = np.abs(dctx[:, :2 * H]) * sg
    d0 = [rng.standard_normal(a.shape).astype(np.float32) for a in (Hp, Hn, Hc)]
    dbuf = [cu(a) for a in d0]
    did = torch.full((S * A, E), float("nan"), device="cuda")
    d_dmy, d_dctx = cu(dmy), cu(dctx)
    call("msat_actor_pool_bwd", H, *lay_ptrs(lay), A + 1, S, A, M, base, rem, E, d_dmy.data_ptr(), d_dctx.data_ptr(),
         *(t.data_ptr() for t in dbuf), did.data_ptr())
    assert_bitwise(host(did), dctx[:, 5 * H:], "did = tail of dctx")
    rmy, rctx, _, leaves = _actor_ref(Hp, Hn, Hc, ide, lay, nown, A, M)
    ((rmy * torch.tensor(dmy, dtype=torch.float64)).sum() + (rctx * torch.tensor(dctx, dtype=torch.float64)).sum()).backward()
    agents = [s * (A + 1) + 1 + i for s in range(S) for i in range(A)]
    for name, got, base0, leaf, which in zip(("dHp", "dHn", "dHc"), dbuf, d0, leaves, "vvc"):
        got = host(got)
        g = leaf.grad.numpy() if leaf.grad is not None else np.zeros(base0.shape)
        mine = rows_mask(lay, agents, which)
        assert_bitwise(got[~mine], base0[~mine], f"{name}: critic-graph rows and gaps")
        assert_within(got[mine], base0[mine].astype(np.float64) + g[mine],
                      4 * U * (np.abs(base0[mine]) + np.abs(g[mine])), f"{name}: d0 + gradient")


# ------------------------------------------------------- element-wise kernels ----
ELEMENTWISE_SHAPES = [(37, 3, 128), (1, 1, 1), (5, 8, 67), (0, 3, 16)]  # R, M, W; R = 0: nothing is launched


@pytest.mark.parametrize("R,M,W", ELEMENTWISE_SHAPES)
def test_bcast_add_relu_and_group_sum(R, M, W):
    rng = np.random.default_rng(R * 100 + W)
    Q = rng.standard_normal((max(R, 1) * M, W)).astype(np.float32)
    P = rng.standard_normal((max(R, 1), W)).astype(np.float32)
    dQ, dP_ = cu(Q), cu(P)
    call("msat_bcast_add_relu", dQ.data_ptr(), dP_.data_ptr(), R, M, W)
    want = np.maximum(Q + np.repeat(P, M, 0), np.float32(0)) if R else Q
    assert_bitwise(host(dQ), want, "relu(Q + P[r // M])")
    assert R * M * W < 64 or ((want == 0).any() and (want > 0).any())  # both sides of the ReLU
    out = torch.full((max(R, 1), W), float("nan"), device="cuda")
    d_in = cu(Q)
    call("msat_group_sum", d_in.data_ptr(), R, M, W, out.data_ptr())
    if R:
        acc = np.zeros((R, W), np.float32)
        for m in range(M):  # the kernel's order
            acc = acc + Q.reshape(R, M, W)[:, m]
        assert_bitwise(host(out), acc, "group sum in order")
    else:
        assert bool(torch.isnan(out).all())


LOGIT_SHAPES = [  # S, A, M, base, rem
    (5, 3, 8, 7, 2),  # SA * (M + 1) = 135: one partial block; agents of 8, 8, 7
    (1, 1, 1, 1, 0),
    (37, 3, 10, 9, 1),  # 1221 elements: five blocks, the last partial
    (2, 4, 3, 0, 2),  # agents of 1, 1, 0, 0 variables
    (0, 3, 8, 7, 2),  # n = 0
]


def _slot_mask(S, A, M, base, rem):
    """(S*A, M) True where slot j belongs to agent i = r % A (j < base + (i < rem))."""
    n = np.array([base + (i < rem) for i in range(A)])
    return np.tile(np.arange(M)[None, :] < n[:, None], (S, 1))


@pytest.mark.parametrize("S,A,M,base,rem", LOGIT_SHAPES)
def test_assemble_mask_split_logits(S, A, M, base, rem):
    rng = np.random.default_rng(S * 10 + M)
    SA, SA1 = S * A, max(S * A, 1)
    live = _slot_mask(S, A, M, base, rem) if S else np.zeros((0, M), bool)
    flip = rng.standard_normal((SA1, M)).astype(np.float32)
    noop = rng.standard_normal(SA1).astype(np.float32)
    logits = torch.full((SA1, M + 1), float("nan"), device="cuda")
    d_flip, d_noop = cu(flip), cu(noop)
    call("msat_assemble_logits", d_flip.data_ptr(), d_noop.data_ptr(), SA, A, M, base, rem, logits.data_ptr())
    if S:
        want = np.concatenate([np.where(live, flip, np.float32(NINF)), noop[:, None]], 1)
        assert_bitwise(host(logits), want, "logits = [flip | noop] with -inf in padded slots")
        assert rem == 0 or (want == NINF).any()
    else:
        assert bool(torch.isnan(logits).all())
    # mode 1: (SA * M, 2), both logits of a padded slot -inf, everything else untouched
    vl = rng.standard_normal((SA1 * M, 2)).astype(np.float32)
    d_vl = cu(vl)
    call("msat_mask_var_logits", d_vl.data_ptr(), SA, A, M, base, rem)
    want = np.where(live.reshape(-1, 1), vl[:SA * M], np.float32(NINF)) if S else vl
    assert_bitwise(host(d_vl)[:want.shape[0]], want, "masked variable logits")
    # split: every position of dlogits lands in dflip or dnoop, padded ones included
    dl = rng.standard_normal((SA1, M + 1)).astype(np.float32)
    dflip = torch.full((SA1, M), float("nan"), device="cuda")
    dnoop = torch.full((SA1,), float("nan"), device="cuda")
    d_dl = cu(dl)
    call("msat_split_dlogits", d_dl.data_ptr(), SA, M, dflip.data_ptr(), dnoop.data_ptr())
    if S:
        assert_bitwise(host(dflip), dl[:, :M], "dflip")
        assert_bitwise(host(dnoop), dl[:, M], "dnoop")
    else:
        assert bool(torch.isnan(dflip).all()) and bool(torch.isnan(dnoop).all())


@pytest.mark.parametrize("n", [0, 1, 255, 37 * 3 * 128 + 1])
def test_relu_forward_backward(n):
    rng = np.random.default_rng(n)
    m = max(n, 1)
    x = rng.standard_normal(m).astype(np.float32)
    x[: min(m, 3)] = np.array([0.0, -0.0, -1.5], np.float32)[: min(m, 3)]
    d_x = cu(x)
    call("msat_relu", d_x.data_ptr(), n)
    y = host(d_x)
    pos = x > 0
    if n:
        assert_bitwise(y[pos], x[pos], "relu keeps positives")
        assert (y[~pos] == 0).all()  # +0, -0 and negatives all give zero
    else:
        assert_bitwise(y, x, "n = 0 leaves the buffer alone")
    dy = rng.standard_normal(m).astype(np.float32)
    d_dy, d_y = cu(dy), cu(np.where(pos, x, np.float32(0)) if n else x)
    if n >= 2:
        d_y[1] = -0.0  # an output of -0 also stops the gradient
    call("msat_relu_bwd", d_dy.data_ptr(), d_y.data_ptr(), n)
    want = np.where(pos, dy, np.float32(0)) if n else dy
    assert_bitwise(host(d_dy), want, "relu_bwd zeroes the gradient where y == 0")


# ------------------------------------------------------------------ PPO loss ----
# every coefficient is exact in fp32, so the kernel and the float64 reference use the same numbers
PPO_CFG = {"CLIP_EPS": 0.125, "VF_CLIP": 0.5, "ENT_COEF": 2.0 ** -7, "VF_COEF": 0.5}
SUMS0 = np.array([1.5, -2.25, 3.0])  # loss_sums is added to, never overwritten


def _sample(logits2d, greedy, seed=77, counter=3):
    R, W = logits2d.shape
    act = torch.full((R,), -9, dtype=torch.int32, device="cuda")
    lp = torch.full((R,), float("nan"), device="cuda")
    d_lg = cu(logits2d)
    call("msat_sample_actions", d_lg.data_ptr(), R, W, 1 if greedy else 0, seed, counter, act.data_ptr(),
         lp.data_ptr())
    return host(act), host(lp)


def _run_ppo(c, cfg, mb=None, sums=None, sl=slice(None)):
    """msat_ppo_loss on the samples sl of case c -> dlogits, dvalue, surrogate rows, entropy rows,
    value terms, loss_sums (numpy)."""
    lg = c["logits"][sl]
    S, A, M, mode = lg.shape[0], c["A"], c["M"], c["mode"]
    R = S * A
    dev = {k: cu(c[k][sl]) for k in ("logits", "action", "old_logp", "gae", "value", "old_value", "targets")}
    dl = torch.full(lg.shape, float("nan"), device="cuda")
    dv = torch.full((S,), float("nan"), device="cuda")
    rows = torch.full((2 * R + S,), float("nan"), device="cuda")
    d_sums = cu(np.zeros(3)) if sums is None else sums
    call("msat_ppo_loss", dev["logits"].data_ptr(), S, A, M, mode, c["base"], c["rem"], dev["action"].data_ptr(),
         dev["old_logp"].data_ptr(), dev["gae"].data_ptr(), dev["value"].data_ptr(), dev["old_value"].data_ptr(),
         dev["targets"].data_ptr(), cfg["CLIP_EPS"], cfg["VF_CLIP"], cfg["ENT_COEF"], cfg["VF_COEF"],
         S if mb is None else mb, dl.data_ptr(), dv.data_ptr(), rows.data_ptr(), d_sums.data_ptr())
    r = host(rows)
    return {"dlogits": host(dl), "dvalue": host(dv), "surr": r[0:2 * R:2].reshape(S, A),
            "ent": r[1:2 * R:2].reshape(S, A), "vterms": r[2 * R:], "sums": host(d_sums)}


def _ref_ppo(c, cfg, mb=None, log_prob=None):
    """oracle.net.ppo_terms in float64 on the same fp32 inputs, with the action clamped into its row as
    the kernel does; the three means divide by the minibatch size mb (default: the S of the call)."""
    mode, A, M = c["mode"], c["A"], c["M"]
    S = c["logits"].shape[0]
    mb = S if mb is None else mb
    lg = torch.tensor(c["logits"], dtype=torch.float64, requires_grad=True)
    v = torch.tensor(c["value"], dtype=torch.float64, requires_grad=True)
    act = np.clip(c["action"], 0, M) if mode == 0 else (c["action"] & 1)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    bt = {"action": torch.tensor(act).long(), "log_prob": t64(c["old_logp"]) if log_prob is None else log_prob,
          "gae": t64(c["gae"]), "value": t64(c["old_value"]), "targets": t64(c["targets"])}
    mask = torch.from_numpy(_slot_mask(1, A, M, c["base"], c["rem"]))
    total, (vl, la, ent), surr, ent_rows, vterms = onet.ppo_terms(lg, v, bt, cfg, mask, mode)
    n_ent = ent_rows.numel() // S
    scaled = surr.sum() / (mb * A) - cfg["ENT_COEF"] * ent_rows.sum() / (mb * n_ent) + cfg["VF_COEF"] * vterms.sum() / mb
    if mb == S:
        assert abs(float(scaled.detach()) - float(total.detach())) <= 1e-12 * (1 + abs(float(total.detach())))
    scaled.backward()
    return {"dlogits": lg.grad.numpy(), "dvalue": v.grad.numpy(), "surr": surr.detach().numpy(),
            "ent": (ent_rows if mode == 0 else ent_rows.sum(-1)).detach().numpy(), "vterms": vterms.detach().numpy(),
            "means": tuple(float(t.detach()) for t in (vl, la, ent)), "n_ent": n_ent}


def _check_ppo(got, ref, sums0=None, rtol=1e-5):
    assert np.isfinite(got["dlogits"]).all() and np.isfinite(got["dvalue"]).all()
    for k in ("dlogits", "dvalue", "surr", "ent", "vterms"):  # every row, not only the sums
        assert_normwise(got[k], ref[k], rtol, k)
    S, A = got["surr"].shape
    s = got["sums"] - (0.0 if sums0 is None else sums0)
    own = np.array([got["vterms"].astype(np.float64).sum(), got["surr"].astype(np.float64).sum(),
                    got["ent"].astype(np.float64).sum()])
    scale = np.array([np.abs(got[k]).astype(np.float64).sum() for k in ("vterms", "surr", "ent")]) + 1.0
    assert (np.abs(s - own) <= 1e-12 * scale).all(), (s, own)  # fp64 sums of the fp32 row terms
    for k, cnt in enumerate((S, S * A, S * ref["n_ent"])):
        np.testing.assert_allclose(s[k] / cnt, ref["means"][k], rtol=1e-5, atol=1e-7)


def _ppo_case(S, A, M, base, rem, mode, seed):
    """Random logits with the per-agent masks in place, valid actions, old log-probs near the new ones
    (ratios on both sides of the clip range)."""
    rng = np.random.default_rng(seed)
    live = _slot_mask(S, A, M, base, rem).reshape(S, A, M)
    if mode == 0:
        lg = rng.standard_normal((S, A, M + 1)).astype(np.float32) * 1.5
        lg[..., :M][~live] = NINF
        p = torch.softmax(torch.tensor(lg, dtype=torch.float64), -1)
        act = torch.multinomial(p.reshape(S * A, M + 1), 1, generator=torch.Generator().manual_seed(seed)).reshape(S, A)
        lp = torch.log_softmax(torch.tensor(lg, dtype=torch.float64), -1).gather(-1, act[..., None])[..., 0].numpy()
        act = act.numpy().astype(np.int32)
        olp = (lp + rng.normal(0, 0.1, lp.shape)).astype(np.float32)
    else:
        lg = rng.standard_normal((S, A, M, 2)).astype(np.float32) * 1.5
        lg[~live] = NINF
        act = rng.integers(0, 2, (S, A, M)).astype(np.int32)
        lp = onet.log_softmax(torch.tensor(lg, dtype=torch.float64)).gather(-1, torch.tensor(act).long()[..., None])[..., 0]
        olp = (lp.numpy() + rng.normal(0, 0.1 / math.sqrt(M), lp.shape)).astype(np.float32)
        # padded slots: whatever the caller left there must be ignored
        olp[~live] = np.nan
        act[~live] = rng.choice(np.array([-7, 12345, 3, -1], np.int32), int((~live).sum()))
    val = rng.standard_normal(S).astype(np.float32)
    return {"S": S, "A": A, "M": M, "base": base, "rem": rem, "mode": mode, "logits": lg, "action": act,
            "old_logp": olp, "gae": rng.standard_normal(S).astype(np.float32), "value": val,
            "old_value": (val + rng.normal(0, 0.4, S)).astype(np.float32),
            "targets": (val + rng.normal(0, 1, S)).astype(np.float32), "live": live}


PPO_MODE0_CASES = [  # S, A, M (W = M + 1), base, rem
    (5, 3, 1, 0, 2),  # W = 2; agent 2 owns no variable: its row is [-inf, noop]
    (5, 3, 10, 9, 2),  # W = 11
    (5, 3, 63, 62, 2),  # W = 64: exactly one trip of the j += 64 loops
    (5, 3, 64, 63, 2),  # W = 65: lane 0 takes a second trip of the j += 64 loops
    (5, 3, 129, 128, 2),  # W = 130: three trips
    (1, 1, 10, 9, 0),  # S * A = 1: one wave of the block has a row
    (1, 7, 10, 9, 3),  # S * A = 7: R % 4 != 0, two blocks, the second partial; r / A and r % A over one sample
    (7, 1, 10, 9, 0),  # A = 1: every row is an agent-0 row and writes a value term
    # R = 32775 > 8192 blocks x 4 rows: 7 rows take the grid-stride trip of ppo_loss_kernel's row loop (a partial
    # trip: R % 4 = 3); M = 1, agents 13.. own nothing
    (1311, 25, 1, 0, 13),
]


@pytest.mark.parametrize("S,A,M,base,rem", PPO_MODE0_CASES)
def test_ppo_loss_mode0_matches_oracle(S, A, M, base, rem):
    c = _ppo_case(S, A, M, base, rem, 0, 500 + M + S)
    assert (c["logits"] == NINF).any()  # the masked-lane branches of the kernel run
    got = _run_ppo(c, PPO_CFG, sums=cu(SUMS0))
    ref = _ref_ppo(c, PPO_CFG)
    _check_ppo(got, ref, SUMS0)
    assert (got["dlogits"][c["logits"] == NINF] == 0).all()  # masked columns get exactly zero


@pytest.mark.parametrize("M", [1, 4, 10])
def test_ppo_loss_mode1_matches_oracle(M):
    # R = S * A = 300 > 256: the second block of ppo_loss_multi_kernel (one thread per row) runs, partly filled
    S, A = 100, 3
    c = _ppo_case(S, A, M, M - 1, 2, 1, 600 + M)
    assert np.isnan(c["old_logp"]).any() and (c["action"] > 1).any()  # garbage sits in the padded slots
    got = _run_ppo(c, PPO_CFG, sums=cu(SUMS0))
    ref = _ref_ppo(c, PPO_CFG)
    _check_ppo(got, ref, SUMS0)
    assert (got["dlogits"][~c["live"]] == 0).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_ppo_loss_out_of_range_actions_are_clamped(mode):
    """Actions -1, W and one that points at a masked slot: every output is finite and equals the
    reference evaluated with the action the kernel uses (clamped into the row; bit 0 in mode 1)."""
    S, A, M = 2, 3, 10
    c = _ppo_case(S, A, M, 9, 2, mode, 700 + mode)
    if mode == 0:
        c["action"][0, 0], c["action"][0, 1], c["action"][0, 2] = -1, M + 1, M - 1
        assert c["logits"][0, 2, M - 1] == NINF  # agent 2 has 9 variables: slot 9 is masked, ratio = 0
    else:
        c["action"][0, 0, :3] = [-1, 2, 7]
    got = _run_ppo(c, PPO_CFG)
    for k in ("dlogits", "dvalue", "surr", "ent", "vterms"):
        assert np.isfinite(got[k]).all(), k
    _check_ppo(got, _ref_ppo(c, PPO_CFG))


@pytest.mark.parametrize("mode", [0, 1])
def test_ppo_loss_micro_batches_add_up(mode):
    """minibatch != S: two calls over S1 = 2 and S2 = 3 samples with minibatch = 5 give, row for row,
    the bits of the single call over all five, and loss_sums receives the sum of both on top of its
    contents (the 1 / n factors come from the minibatch size, not from the S of the call)."""
    c = _ppo_case(5, 3, 10, 9, 2, mode, 800 + mode)
    whole = _run_ppo(c, PPO_CFG, sums=cu(SUMS0))
    _check_ppo(whole, _ref_ppo(c, PPO_CFG), SUMS0)
    sums = cu(SUMS0)
    a = _run_ppo(c, PPO_CFG, mb=5, sums=sums, sl=slice(0, 2))
    b = _run_ppo(c, PPO_CFG, mb=5, sums=sums, sl=slice(2, 5))
    for k in ("dlogits", "dvalue", "surr", "ent", "vterms"):
        assert_bitwise(np.concatenate([a[k], b[k]], 0), whole[k], k)
    assert np.abs(b["sums"] - whole["sums"]).max() <= 1e-12 * np.abs(whole["sums"]).max()
    assert np.abs(whole["sums"] - SUMS0).min() > 1e-3
    # and one micro-batch alone against the reference scaled by the minibatch size
    ref = _ref_ppo({**c, **{k: c[k][:2] for k in ("logits", "action", "old_logp", "gae", "value", "old_value",
                                                  "targets")}}, PPO_CFG, mb=5)
    for k in ("dlogits", "dvalue"):
        assert_normwise(a[k], ref[k], 1e-5, k + " of a micro-batch")


# ---- ties: each of these is exact ----
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
def test_ratio_is_exactly_one_on_sampled_log_probs(mode, greedy):
    """old_logp from msat_sample_actions on the same logits: the loss kernel reproduces the sampler's
    log-prob bits, so ratio == 1, the surrogate is -gae bit for bit (the first minibatch of the first
    epoch), and with clip_eps = 0 (lo == hi == ratio) the actor gradient is the balanced-tie
    0.5 * (g + 0.25 * g) = 0.625 g of jnp.minimum / jnp.clip."""
    S, A, M = 6, 3, 10
    c = _ppo_case(S, A, M, 9, 2, mode, 900 + mode)
    flat = c["logits"].reshape(-1, c["logits"].shape[-1])
    act, lp = _sample(flat, greedy)
    c["action"], c["old_logp"] = act.reshape(c["action"].shape), lp.reshape(c["action"].shape)
    if mode == 1:
        assert (c["old_logp"][~c["live"]] == 0).all()
    want = np.broadcast_to(-c["gae"][:, None], (S, A))
    assert (c["gae"] != 0).all()
    for eps in (0.125, 0.0):
        cfg = dict(PPO_CFG, CLIP_EPS=eps, ENT_COEF=0.0)
        got = _run_ppo(c, cfg)
        assert_bitwise(got["surr"], want, f"surrogate == -gae (clip_eps {eps})")
        assert int((bits(got["surr"]) == bits(want)).sum()) == S * A  # the tie occurred on every row
    # the reference at its own log-probs (ratio exactly 1 there too), clip_eps = 0
    lg64 = torch.tensor(c["logits"], dtype=torch.float64)
    a64 = torch.tensor(c["action"] if mode == 0 else c["action"] & 1).long()
    lp64 = onet.log_softmax(lg64).gather(-1, a64[..., None])[..., 0]
    ref = _ref_ppo(c, cfg, log_prob=lp64)
    assert (ref["surr"] == -c["gae"].astype(np.float64)[:, None]).all()
    assert_normwise(got["dlogits"], ref["dlogits"], 1e-5, "dlogits under the 0.625 g tie rule")
    # the rule itself, at the action's logit of every mode-0 row: d = -0.625 g (1 - p_a) / (S A)
    if mode == 0:
        p = torch.softmax(lg64, -1).gather(-1, a64[..., None])[..., 0].numpy()
        rule = -0.625 * c["gae"].astype(np.float64)[:, None] * (1 - p) / (S * A)
        at = np.take_along_axis(got["dlogits"], c["action"][..., None].astype(np.int64), -1)[..., 0]
        assert_normwise(at, rule, 1e-5, "0.625 g at the action")


def test_value_clip_and_maximum_ties():
    """v == v_old and v - v_old == +-vf_clip exactly: a1 == a2, and on the clip bound d clip = 0.5, so
    dvalue = 0.75 (v - t) vf_coef / minibatch there (1.0 inside the range)."""
    v = np.array([1.0, 1.5, 0.5, 1.25], np.float32)
    vo = np.ones(4, np.float32)
    t = np.array([0.25, 0.25, 2.0, 3.0], np.float32)
    vc = vo + np.clip(v - vo, np.float32(-0.5), np.float32(0.5))
    assert (((v - t) ** 2 == (vc - t) ** 2).sum() == 4) and (np.abs(v - vo)[1:3] == 0.5).all()  # the ties occur
    c = {"S": 4, "A": 1, "M": 1, "base": 1, "rem": 0, "mode": 0, "logits": np.zeros((4, 1, 2), np.float32),
         "action": np.zeros((4, 1), np.int32), "old_logp": np.full((4, 1), -math.log(2.0), np.float32),
         "gae": np.zeros(4, np.float32), "value": v, "old_value": vo, "targets": t}
    got = _run_ppo(c, PPO_CFG)
    ref = _ref_ppo(c, PPO_CFG)
    want = np.array([1.0, 0.75, 0.75, 1.0]) * (v.astype(np.float64) - t) * 0.5 / 4
    assert (ref["dvalue"] == want).all()
    assert_bitwise(got["dvalue"], want.astype(np.float32), "dvalue at the ties")
    assert_bitwise(got["vterms"], (0.5 * (v.astype(np.float64) - t) ** 2).astype(np.float32), "value terms")


@pytest.mark.parametrize("mode", [0, 1])
def test_zero_advantage_gives_zero_actor_gradient(mode):
    """gae == 0: ratio * g == clip(ratio) * g == 0 ties whatever the ratio; both branches carry 0."""
    c = _ppo_case(4, 3, 10, 9, 2, mode, 1000 + mode)
    c["gae"][[0, 2]] = 0.0
    got = _run_ppo(c, dict(PPO_CFG, ENT_COEF=0.0))
    assert (got["surr"][[0, 2]] == 0).all() and (got["dlogits"][[0, 2]] == 0).all()
    assert np.abs(got["dlogits"][[1, 3]]).max() > 0
    _check_ppo(got, _ref_ppo(c, dict(PPO_CFG, ENT_COEF=0.0)))


# ---------------------------------------------------------------------- Adam ----
INT32_MAX = 2 ** 31 - 1


def _adam(p, g, m, v, lr, count, gs, first_bad=None):
    n = p.numel()
    call("msat_adam_checked", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, 0.9, 0.999, 1e-8, count,
         gs, None if first_bad is None else first_bad.data_ptr())


@pytest.mark.parametrize("gs", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("count", [1, 2, 1000, 200000])  # 200000: both bias corrections are exactly 1 in fp32
@pytest.mark.parametrize("n", [1, 255, 257, 100003])  # below / above one block, and a partial last block of 391
def test_adam_matches_optax_in_float64(n, count, gs):
    rng = np.random.default_rng(n + count)
    p0 = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    for k, special in enumerate((0.0, 1e-30, 1e15)):  # zero, tiny (its square underflows) and huge gradients
        g[(7 * k + count) % n] = special
    # m0 has the sign of its gradient: b1 m0 + (1 - b1) g does not cancel, so the relative error of m (and of
    # the update) stays within the few roundings that the bound on p counts
    m0 = (np.where(g < 0, -1.0, 1.0) * (0.1 * np.abs(rng.standard_normal(n)) + 1e-4)).astype(np.float32)
    v0 = (0.01 * rng.standard_normal(n) ** 2 + 1e-6).astype(np.float32)
    dp, dg, dm, dv = cu(p0), cu(g), cu(m0), cu(v0)
    bad = torch.full((1,), INT32_MAX, dtype=torch.int32, device="cuda")
    _adam(dp, dg, dm, dv, 1e-3, count, gs, bad)
    # optax.adam in float64 on the fp32 inputs; b1 / b2 / lr / eps / grad_scale as the fp32 numbers the kernel
    # receives (1.0f - 0.999f differs from 0.001 by 1.3e-5 relative)
    f = lambda x: float(np.float32(x))
    b1, b2, lr, eps, s = f(0.9), f(0.999), f(1e-3), f(1e-8), f(gs)
    gi = g.astype(np.float64) * s
    m = b1 * m0.astype(np.float64) + (1 - b1) * gi
    v = b2 * v0.astype(np.float64) + (1 - b2) * gi * gi
    upd = -lr * (m / (1 - b1 ** count)) / (np.sqrt(v / (1 - b2 ** count)) + eps)
    p = p0.astype(np.float64) + upd
    # m: g * s, (1 - b1) * gi, b1 * m, the add; v: two roundings of gi, three products, the add (+ underflow)
    assert_within(host(dm), m, 4 * U * (np.abs(b1 * m0) + np.abs((1 - b1) * gi)), "m")
    assert_within(host(dv), v, 6 * U * (b2 * v0 + (1 - b2) * gi * gi) + 1e-37, "v")
    assert_within(host(dp), p, 2.0 ** -23 * np.abs(p) + 2.0 ** -20 * np.abs(upd), "p")
    assert int(bad.item()) == INT32_MAX  # finite inputs leave first_bad alone


def test_adam_first_bad_keeps_the_minimum():
    n = 300
    rng = np.random.default_rng(3)
    g = rng.standard_normal(n).astype(np.float32)
    g[277] = np.nan
    dp, dg, dm, dv = (cu(rng.standard_normal(n).astype(np.float32)), cu(g), cu(np.zeros(n, np.float32)),
                      cu(np.zeros(n, np.float32)))
    bad = torch.full((1,), INT32_MAX, dtype=torch.int32, device="cuda")
    _adam(dp, dg, dm, dv, 1e-3, 5, 1.0, bad)
    assert int(bad.item()) == 5
    _adam(dp, dg, dm, dv, 1e-3, 9, 1.0, bad)
    assert int(bad.item()) == 5
    assert int(torch.isnan(dp).sum().item()) == 1  # only the parameter of the NaN gradient


# ------------------------------------------------- moments / standardize ----
@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 1])  # 1024 blocks x 256 threads + 1: one grid-stride trip
def test_moments_and_standardize(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 3 + 0.5).astype(np.float32)
    d_x = cu(x)
    out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((2 * 1024 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    call("msat_moments", d_x.data_ptr(), n, out.data_ptr(), ws.data_ptr())
    x64 = x.astype(np.float64)
    s1, s2 = math.fsum(x64), math.fsum(x64 * x64)  # the squares of fp32 numbers are exact in fp64
    got = host(out)
    assert abs(got[0] - s1) <= n * 2.0 ** -53 * np.abs(x64).sum()
    assert abs(got[1] - s2) <= n * 2.0 ** -53 * s2
    mean, std = np.float32(s1 / n), np.float32(math.sqrt(max(s2 / n - (s1 / n) ** 2, 0.0)) + 1e-8)
    call("msat_standardize", d_x.data_ptr(), n, float(mean), float(std))
    assert_bitwise(host(d_x), (x - mean) / std, "(x - mean) / std")
