"""GPU: the exports of csrc/gnn_kernels.hip (and the fp64-accumulating product of gemm.hip) that no other test calls,
and the gathers past their grid caps and at the narrow widths their argument check accepts.

  * msat_gru_ln_fwd / msat_gru_ln_bwd, the unfused GRU + LayerNorm (Gi, Gh of 3H each): forward against
    _ref_gru_ln's float64 at 1e-5 |ref| + 1e-5, backward against float64 autograd w.r.t. Gi, Gh, h, scale, bias at the
    two bars of tests/test_gru_bwd_gpu.py; strided operands with canaries; the refusals.
  * msat_gemm_f64acc: all of transA x transB x accumulate against float64 at the DERIVED bound
        |C - ref64| <= 2^-24 |ref64| + (K + 2) 2^-52 sum |a b|
    (one fp32 rounding of the result + the two fp64 summation orders), on inputs spread over binades whose products
    cancel -- a plain float32 product of the same inputs violates the bound (asserted on the CPU).
  * msat_clause_gather / msat_var_gather (one [pos | neg] source of ld 2H), H = 32 and 96, strided destinations, and
    row counts past the 8192-block grids (a second trip of the grid-stride loops): BITWISE against float32 sums
    added in slot / entry order.
"""
import functools

import numpy as np
import pytest
import torch

from test_gathers_gpu import _clause_ref, _graph, _var_ref
from test_gru_bwd_gpu import CANARY, _compare, _inputs, _padded
from test_gru_fused_gpu import _ref_gru_ln

pytestmark = pytest.mark.gpu

# Worst (|err| - 1e-5 |ref|) / E32 printed by test_unfused_backward_matches_float64 on MI355X, per tensor: see
# GRAD_FACTOR in tests/test_gru_bwd_gpu.py (the same bar; _compare applies it).


# ------------------------------------------------------------------ unfused GRU + LN --
def _gates(R, H, seed):
    """Gi, Gh (R, 3H), h, dy, scale, bias on the CPU from the tape of test_gru_bwd_gpu._inputs (its saturated,
    constant-h' and zero-dy rows included): Gi_r + Gh_r = r_pre and Gi_z + Gh_z = z_pre exactly (two equal halves)."""
    g4, h, dy, sc, lb, _ = _inputs(R, H, 0, seed)
    Gi = torch.cat([0.5 * g4[:, :2 * H], g4[:, 2 * H:3 * H]], 1)
    Gh = torch.cat([0.5 * g4[:, :2 * H], g4[:, 3 * H:]], 1)
    return Gi, Gh, h, dy, sc, lb


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("R", [0, 1, 5, 77, 32773])  # 32773: past the 8192-block grid (4 rows per block)
def test_unfused_forward_matches_reference(R, H):
    from marlsat import _lib

    Gi, Gh, h, _, sc, lb = _gates(R, H, seed=3 * R + H)
    ldi, ldh, ldp, ldo = 3 * H + 4, 3 * H + 8, H + 4, H + 12
    gib, gip = _padded(Gi, ldi, fill=float("nan"))  # gap columns NaN: never read
    ghb, ghp = _padded(Gh, ldh, fill=float("nan"))
    hb, hp = _padded(h, ldp, fill=float("nan"))
    scd, lbd = sc.cuda(), lb.cuda()
    ob, op = _padded(torch.full((R, H), float("nan")), ldo)
    _lib.check(_lib.lib.msat_gru_ln_fwd(gip, ldi, ghp, ldh, hp, ldp, scd.data_ptr(), lbd.data_ptr(), op, ldo, R, H,
                                        _lib.stream_ptr()), "gru_ln_fwd")
    torch.cuda.synchronize()
    out = ob.view(R + 1, ldo).cpu()
    assert bool((out[:, H:] == CANARY).all()) and bool((out[R] == CANARY).all())
    if R == 0:
        return
    d = lambda t: t.double()
    # _ref_gru_ln with gi = 0 @ 0 + Gi, gh = h @ 0 + Gh
    ref, _, _ = _ref_gru_ln(torch.zeros(R, 1, dtype=torch.float64), d(h), torch.zeros(1, 3 * H, dtype=torch.float64),
                            d(Gi), torch.zeros(H, 3 * H, dtype=torch.float64), d(Gh), d(sc), d(lb), H)
    err = (out[:R, :H].double() - ref).abs()
    assert bool((err <= 1e-5 * ref.abs() + 1e-5).all()), float(err.max())


def _unfused_formula(inp, H, dtype):
    Gi, Gh, h, dy, sc, lb = (t.to(dtype) for t in inp)
    Gi, Gh, h, sc, lb = (t.clone().requires_grad_(True) for t in (Gi, Gh, h, sc, lb))
    r = torch.sigmoid(Gi[:, :H] + Gh[:, :H])
    z = torch.sigmoid(Gi[:, H:2 * H] + Gh[:, H:2 * H])
    n = torch.tanh(Gi[:, 2 * H:] + r * Gh[:, 2 * H:])
    hn = (1 - z) * n + z * h
    mean = hn.mean(-1, keepdim=True)
    var = (hn * hn).mean(-1, keepdim=True) - mean * mean
    y = (hn - mean) * torch.rsqrt(var + 1e-6) * sc + lb
    (y * dy).sum().backward()
    return {"dGi": Gi.grad, "dGh": Gh.grad, "dh": h.grad, "dln": torch.cat([sc.grad, lb.grad])}


@functools.lru_cache(maxsize=None)
def _unfused_case(R, H, seed):
    inp = _gates(R, H, seed)
    return inp, _unfused_formula(inp, H, torch.float64), _unfused_formula(inp, H, torch.float32)


def _unfused_bwd(inp, R, H, acc, pad, dh0, dln0, dln_bias_off=None, H_arg=None):
    """One msat_gru_ln_bwd launch; returns (rc, outputs on the CPU)."""
    from marlsat import _lib

    Gi, Gh, h, dy, sc, lb = inp
    nan = float("nan")
    ldy, ldi, ldh, ldp = H + 4 * pad, 3 * H + 4 * pad, 3 * H + 8 * pad, H + 4 * pad
    lddi, lddh, lddp = 3 * H + 8 * pad, 3 * H + 4 * pad, H + 12 * pad
    dyb, dyp = _padded(dy, ldy, fill=nan)
    gib, gip = _padded(Gi, ldi, fill=nan)
    ghb, ghp = _padded(Gh, ldh, fill=nan)
    hb, hp = _padded(h, ldp, fill=nan)
    scd = sc.cuda()
    dgib, dgip = _padded(torch.full((R, 3 * H), nan), lddi)
    dghb, dghp = _padded(torch.full((R, 3 * H), nan), lddh)
    dhb, dhp = _padded(dh0, lddp)
    dln = dln0.cuda()
    nfl = int(_lib.lib.msat_gru_ln_bwd_partial_floats(R, H))
    part = torch.full((nfl + 64,), CANARY, device="cuda")
    Hk = H if H_arg is None else H_arg
    rc = _lib.lib.msat_gru_ln_bwd(dyp, ldy, gip, ldi, ghp, ldh, hp, ldp, scd.data_ptr(), dgip, lddi, dghp, lddh, dhp,
                                  lddp, dln.data_ptr(), dln.data_ptr() + 4 * (H if dln_bias_off is None else dln_bias_off),
                                  part.data_ptr(), R, Hk, acc, _lib.stream_ptr())
    torch.cuda.synchronize()  # every device tensor above is still referenced here
    return rc, {"dGi": dgib.view(R + 1, lddi).cpu(), "dGh": dghb.view(R + 1, lddh).cpu(),
                "dh": dhb.view(R + 1, lddp).cpu(), "dln": dln.cpu(), "part_tail": part[nfl:].cpu()}


UNFUSED_BWD = [  # H, R, accumulate_ln, strided
    (64, 0, 1, False), (128, 1, 0, True), (256, 3, 1, False), (64, 4, 0, False), (128, 5, 1, True),
    (256, 77, 0, True), (64, 77, 1, False), (128, 77, 1, False), (128, 4097, 0, False), (256, 4097, 1, True),
    (64, 8195, 0, True), (128, 8195, 1, False),
]


@pytest.mark.parametrize("H,R,acc,pad", UNFUSED_BWD)
def test_unfused_backward_matches_float64(H, R, acc, pad):
    from marlsat import _lib

    seed = 31 * R + H + acc
    inp, ref, yard = _unfused_case(R, H, seed)
    g = torch.Generator().manual_seed(seed + 5)
    dh0 = torch.randn(R, H, generator=g)
    dln0 = torch.randn(2 * H, generator=g) if acc else torch.full((2 * H,), float("nan"))
    rc, out = _unfused_bwd(inp, R, H, acc, pad, dh0, dln0)
    _lib.check(rc, "gru_ln_bwd")
    for k in ("dGi", "dGh"):
        assert bool((out[k][:, 3 * H:] == CANARY).all()) and bool((out[k][R] == CANARY).all()), k
    assert bool((out["dh"][:, H:] == CANARY).all()) and bool((out["dh"][R] == CANARY).all())
    assert bool((out["part_tail"] == CANARY).all())
    if R == 0:
        assert torch.equal(out["dln"], dln0)
        return
    report = []
    _compare("dGi", out["dGi"][:R, :3 * H], ref["dGi"], yard["dGi"], report)
    _compare("dGh", out["dGh"][:R, :3 * H], ref["dGh"], yard["dGh"], report)
    _compare("dh", out["dh"][:R, :H], ref["dh"] + dh0.double(), dh0 + yard["dh"], report)  # always accumulates
    if acc:
        _compare("dln", out["dln"], ref["dln"] + dln0.double(), dln0 + yard["dln"], report)
    else:
        _compare("dln", out["dln"], ref["dln"], yard["dln"], report)
    zero = torch.zeros(R, dtype=torch.bool)
    zero[2::9] = True
    assert bool((out["dGi"][:R, :3 * H][zero] == 0).all()) and bool((out["dGh"][:R, :3 * H][zero] == 0).all())
    print(f"unfused bwd H={H} R={R} acc={acc} strided={pad}: max err / E32, worst (err - 1e-5 |ref|) / E32:",
          [(w, round(a, 2), round(b, 2)) for w, a, b in report])


def test_unfused_refusals_launch_nothing():
    """dln_bias != dln_scale + H and H = 96: a nonzero return code and no output written."""
    from marlsat import _lib

    R, H = 5, 128
    inp, _, _ = _unfused_case(R, H, 1)
    dh0 = torch.full((R, H), CANARY)
    dln0 = torch.full((2 * H + 8,), CANARY)
    for kw in ({"dln_bias_off": H + 4}, {"H_arg": 96}):
        rc, out = _unfused_bwd(inp, R, H, 1, False, dh0, dln0, **kw)
        assert rc != 0 and _lib.lib.msat_last_error()
        assert bool((out["dh"] == CANARY).all()) and bool((out["dln"] == CANARY).all())
        assert bool(torch.isnan(out["dGi"][:R]).all()) and bool(torch.isnan(out["dGh"][:R]).all())
        assert bool((out["part_tail"] == CANARY).all())
    # forward: H = 96 refused, output untouched
    Gi, Gh, h, _, sc, lb = inp
    dev = [t.cuda() for t in (Gi, Gh, h, sc, lb)]
    o = torch.full((R, H), CANARY, device="cuda")
    rc = _lib.lib.msat_gru_ln_fwd(dev[0].data_ptr(), 3 * H, dev[1].data_ptr(), 3 * H, dev[2].data_ptr(), H,
                                  dev[3].data_ptr(), dev[4].data_ptr(), o.data_ptr(), H, R, 96, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and bool((o == CANARY).all())


# ------------------------------------------------------------------ msat_gemm_f64acc --
def _gemm_inputs(M, N, K, seed):
    """A (M, K), B (K, N), C0 (M, N) float32 on the CPU: magnitudes over ~12 binades, and adjacent k pairs whose
    products nearly cancel (a' = -a (1 + d), b' = b (1 + d'), d ~ 1e-3), so |sum a b| << sum |a b|."""
    g = torch.Generator().manual_seed(seed)
    spread = lambda *s: torch.randn(*s, generator=g) * torch.pow(2.0, torch.randint(-6, 7, s, generator=g).float())
    A, B = spread(M, K), spread(K, N)
    if K >= 2:
        ke = K // 2 * 2
        A[:, 1:ke:2] = -A[:, 0:ke:2] * (1 + 1e-3 * torch.randn(M, ke // 2, generator=g))
        B[1:ke:2] = B[0:ke:2] * (1 + 1e-3 * torch.randn(ke // 2, N, generator=g))
    C0 = spread(M, N) * 1e-3
    return A, B, C0


def _gemm_bound(A, B, C0, acc):
    """float64 reference and the derived bound (one fp32 rounding + two fp64 summation orders over K + 1 terms)."""
    K = A.shape[1]
    ref = A.double() @ B.double()
    absab = A.double().abs() @ B.double().abs()
    if acc:
        ref, absab = ref + C0.double(), absab + C0.double().abs()
    return ref, 2.0 ** -24 * ref.abs() + (K + 2) * 2.0 ** -52 * absab, absab


def _run_gemm(A, B, C0, tA, tB, acc, lda=None, ldb=None, ldc=None):
    """C on the CPU after one msat_gemm_f64acc launch; operands stored as the trans flags say, gap columns NaN
    (A, B: never read) or canaries (C: never written)."""
    from marlsat import _lib

    M, K = A.shape
    N = B.shape[1]
    As, Bs = (A.t() if tA else A).contiguous(), (B.t() if tB else B).contiguous()
    lda = lda or As.shape[1] + 3
    ldb = ldb or Bs.shape[1] + 5
    ldc = ldc or N + 7
    ab, ap = _padded(As, lda, fill=float("nan"))
    bb, bp = _padded(Bs, ldb, fill=float("nan"))
    cb, cp = _padded(C0, ldc)
    _lib.check(_lib.lib.msat_gemm_f64acc(ap, lda, tA, bp, ldb, tB, cp, ldc, M, N, K, acc, _lib.stream_ptr()),
               "gemm_f64acc")
    torch.cuda.synchronize()
    out = cb.view(M + 1, ldc).cpu()
    assert bool((out[:, N:] == CANARY).all()) and bool((out[M] == CANARY).all()), "C canaries"
    return out[:M, :N]


def _check_gemm(M, N, K, tA, tB, acc, seed, **ld):
    A, B, C0 = _gemm_inputs(M, N, K, seed)
    ref, bound, absab = _gemm_bound(A, B, C0, acc)
    if M and K >= 128:
        # the inputs are hard enough: a plain float32 product of the same operands misses the bound, and the
        # results are far below sum |a b| on many elements
        c32 = A @ B + C0 if acc else A @ B
        assert bool(((c32.double() - ref).abs() > bound).any()), "inputs too tame: float32 passes the fp64 bound"
        assert float((ref.abs() < 1e-2 * absab).float().mean()) > 0.25
    out = _run_gemm(A, B, C0, tA, tB, acc, **ld)
    if K == 0:
        assert torch.equal(out, C0 if acc else torch.zeros(M, N))
        return 0.0
    err = (out.double() - ref).abs()
    assert bool((err <= bound).all()), (M, N, K, tA, tB, acc, float((err / bound).max()))
    return float((err / bound).max()) if M else 0.0


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("tB", [0, 1])
@pytest.mark.parametrize("tA", [0, 1])
def test_gemm_f64acc_holds_the_fp64_bound(tA, tB, acc):
    worst = 0.0
    for M in (0, 1, 7):
        for N in (1, 257):
            for K in (0, 1, 384):
                worst = max(worst, _check_gemm(M, N, K, tA, tB, acc, seed=1000 * M + 10 * N + K + tA + 2 * tB + 4 * acc))
    print(f"gemm_f64acc tA={tA} tB={tB} acc={acc}: worst err / bound {worst:.3f}")


def test_gemm_f64acc_fold_shapes():
    """The learner's own calls at H = 128 (gnn.py _fold_phi / _unfuse_grads): M, N, K, transA, transB, accumulate and
    the leading dimensions of the stored operands."""
    H, W3 = 128, 384
    shapes = [
        (H, W3, H, 0, 0, 0, H, W3, W3), (1, W3, H, 0, 0, 0, H, W3, W3), (H, W3, H, 0, 0, 0, 2 * H, W3, W3),
        (H, H, W3, 0, 1, 1, W3, W3, H), (1, H, W3, 0, 1, 1, W3, W3, H), (H, H, W3, 0, 1, 1, W3, W3, 2 * H),
        (H, W3, H, 1, 0, 1, H, W3, W3), (H, W3, H, 1, 0, 1, 2 * H, W3, W3), (H, W3, 1, 1, 0, 1, H, W3, W3),
    ]
    worst = 0.0
    for i, (M, N, K, tA, tB, acc, lda, ldb, ldc) in enumerate(shapes):
        worst = max(worst, _check_gemm(M, N, K, tA, tB, acc, seed=77 + i, lda=lda, ldb=ldb, ldc=ldc))
    print(f"gemm_f64acc fold shapes: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------- gathers --
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dst(rows, W, ld, old):
    """Device destination (rows + 1, ld): `old` (or NaN, for an assigning call) in the first W columns, canaries in
    the gap columns and the extra row."""
    t = torch.from_numpy(old) if old is not None else torch.full((rows, W), float("nan"))
    return _padded(t, ld)


def _dst_result(buf, rows, W, ld):
    out = buf.view(rows + 1, ld).cpu().numpy()
    assert (out[:, W:] == CANARY).all() and (out[rows] == CANARY).all(), "destination canaries"
    return out[:rows, :W]


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_single_source_gathers_bitwise(H, acc):
    """msat_clause_gather / msat_var_gather: one [pos | neg] source of ld 2H (src + H, dst + H)."""
    from marlsat import _lib

    Nv, Nc = 37, 101
    slots, ptr, inc = _graph(Nv, Nc, seed=H + 3)
    rng = np.random.default_rng(H + acc)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    X, Y = f(Nv, 2 * H), f(Nc, 2 * H)
    dev = [cu(a) for a in (X, Y, slots, ptr, inc)]
    s = _lib.stream_ptr()
    old = f(Nc, 2 * H) if acc else None
    ld = 2 * H + 4
    gb, gp = _dst(Nc, 2 * H, ld, old)
    _lib.check(_lib.lib.msat_clause_gather(dev[0].data_ptr(), 2 * H, dev[2].data_ptr(), gp, ld, Nc, H, acc, s),
               "clause_gather")
    torch.cuda.synchronize()
    assert np.array_equal(_dst_result(gb, Nc, 2 * H, ld), _clause_ref(X[:, :H], X[:, H:], slots, H, False, old))
    oldv = f(Nv, 2 * H) if acc else None
    vb, vp = _dst(Nv, 2 * H, ld, oldv)
    _lib.check(_lib.lib.msat_var_gather(dev[1].data_ptr(), 2 * H, dev[3].data_ptr(), dev[4].data_ptr(), vp, ld, Nv, H,
                                        acc, s), "var_gather")
    torch.cuda.synchronize()
    P, N = _var_ref(Y[:, :H], Y[:, H:], ptr, inc, H, oldv[:, :H] if acc else None, oldv[:, H:] if acc else None)
    assert np.array_equal(_dst_result(vb, Nv, 2 * H, ld), np.concatenate([P, N], 1))


@pytest.mark.parametrize("H", [32, 96])
def test_narrow_widths_bitwise(H):
    """H % 32 == 0 passes the argument check: H = 32 and 96 through clause_gather2 (split, merged) and var_gather2,
    assigned and accumulating, strided destinations."""
    from marlsat import _lib

    Nv, Nc = 37, 101
    slots, ptr, inc = _graph(Nv, Nc, seed=H)
    rng = np.random.default_rng(H)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    Xp, Xn, Yp, Yn = f(Nv, H), f(Nv, H), f(Nc, H), f(Nc, H)
    dev = [cu(a) for a in (Xp, Xn, Yp, Yn, slots, ptr, inc)]
    s = _lib.stream_ptr()
    for merged in (0, 1):
        for acc in (0, 1):
            W = H if merged else 2 * H
            old = f(Nc, W) if acc else None
            gb, gp = _dst(Nc, W, W + 8, old)
            _lib.check(_lib.lib.msat_clause_gather2(dev[0].data_ptr(), dev[1].data_ptr(), H, dev[4].data_ptr(), gp,
                                                    W + 8, Nc, H, merged, acc, s), "clause_gather2")
            torch.cuda.synchronize()
            assert np.array_equal(_dst_result(gb, Nc, W, W + 8), _clause_ref(Xp, Xn, slots, H, bool(merged), old))
    for acc in (0, 1):
        op, on = (f(Nv, H), f(Nv, H)) if acc else (None, None)
        pb, pp = _dst(Nv, H, H + 4, op)
        nb, np_ = _dst(Nv, H, H + 4, on)
        _lib.check(_lib.lib.msat_var_gather2(dev[2].data_ptr(), dev[3].data_ptr(), H, dev[5].data_ptr(),
                                             dev[6].data_ptr(), pp, np_, H + 4, Nv, H, acc, s), "var_gather2")
        torch.cuda.synchronize()
        P, N = _var_ref(Yp, Yn, ptr, inc, H, op, on)
        assert np.array_equal(_dst_result(pb, Nv, H, H + 4), P) and np.array_equal(_dst_result(nb, Nv, H, H + 4), N)


def _ordered_sum(terms, init):
    """init (+ term 0) (+ term 1) ... in float32, one add per slot; a term is (selected (rows,), values (rows, H))."""
    acc = init
    for sel, val in terms:
        acc = np.where(sel[:, None], (acc + val).astype(np.float32), acc)
    return acc


def test_clause_gather_merged_past_the_grid_cap():
    """Nc = 65541 > 8192 blocks x 4 waves x 2 rows: clause_gather_kernel's stride loop takes a second trip."""
    from marlsat import _lib

    H, Nc, Nv = 64, 65541, 300
    rng = np.random.default_rng(1)
    var = rng.integers(0, Nv, (Nc, 3))
    slots = ((var << 1) | rng.integers(0, 2, (Nc, 3))).astype(np.int32)
    slots[rng.random((Nc, 3)) < 0.3] = -1  # empty slots anywhere in the row
    slots[-1] = -1  # an empty last row
    Xp, Xn = (rng.standard_normal((Nv, H)).astype(np.float32) for _ in range(2))
    old = rng.standard_normal((Nc, H)).astype(np.float32)
    dev = [cu(a) for a in (Xp, Xn, slots)]
    ld = H + 4
    gb, gp = _dst(Nc, H, ld, old)
    _lib.check(_lib.lib.msat_clause_gather2(dev[0].data_ptr(), dev[1].data_ptr(), H, dev[2].data_ptr(), gp, ld, Nc, H,
                                            1, 1, _lib.stream_ptr()), "clause_gather2 merged")
    torch.cuda.synchronize()
    row = np.maximum(slots, 0) >> 1
    terms = [(slots[:, u] >= 0, np.where((slots[:, u] & 1)[:, None] == 1, Xn[row[:, u]], Xp[row[:, u]]))
             for u in range(3)]
    want = (_ordered_sum(terms, np.zeros((Nc, H), np.float32)) + old).astype(np.float32)
    got = _dst_result(gb, Nc, H, ld)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[-1], old[-1])


@pytest.mark.parametrize("H,Nv", [(128, 65541), (64, 32773)])  # var_gather_hw_kernel (2 rows / wave), var_gather_kernel
def test_var_gather_past_the_grid_cap(H, Nv):
    from marlsat import _lib

    Nc = 300
    rng = np.random.default_rng(H)
    deg = rng.integers(0, 4, Nv)
    deg[-1] = 0  # an empty last row
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    inc = ((rng.integers(0, Nc, ptr[-1]) << 1) | rng.integers(0, 2, ptr[-1])).astype(np.int32)
    Yp, Yn = (rng.standard_normal((Nc, H)).astype(np.float32) for _ in range(2))
    dev = [cu(a) for a in (Yp, Yn, ptr, inc)]
    ld = H + 4
    pb, pp = _dst(Nv, H, ld, None)
    nb, np_ = _dst(Nv, H, ld, None)
    _lib.check(_lib.lib.msat_var_gather2(dev[0].data_ptr(), dev[1].data_ptr(), H, dev[2].data_ptr(), dev[3].data_ptr(),
                                         pp, np_, ld, Nv, H, 0, _lib.stream_ptr()), "var_gather2")
    torch.cuda.synchronize()
    tp, tn = [], []
    for u in range(3):
        valid = u < deg
        e = inc[np.minimum(ptr[:-1] + u, max(len(inc) - 1, 0))]
        tp.append((valid & ((e & 1) == 0), Yp[e >> 1]))
        tn.append((valid & ((e & 1) == 1), Yn[e >> 1]))
    zero = np.zeros((Nv, H), np.float32)
    P, N = _dst_result(pb, Nv, H, ld), _dst_result(nb, Nv, H, ld)
    assert np.array_equal(P.view(np.int32), _ordered_sum(tp, zero).view(np.int32))
    assert np.array_equal(N.view(np.int32), _ordered_sum(tn, zero).view(np.int32))
    assert not P[-1].any() and not N[-1].any()
