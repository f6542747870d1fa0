"""GPU: the matrix-product exports against the float64 product at every operand placement their dispatch
distinguishes (tests/gemm_placement.py: misaligned pointers, ld % 4 != 0, strided outputs, a workspace one
float off alignment), with NaN in the guard rows and ld gaps of every input and a canary pattern around every
output.  Per case and accumulate value: the fp64 bound of tests/test_gemm_gpu.py, no NaN in the output,
guards and gaps bit-identical afterwards, and a second launch bitwise equal to the first."""
import zlib

import pytest
import torch

import gemm_placement as gp
from gemm_placement import Placement, operand, vector, workspace

pytestmark = pytest.mark.gpu


def _ref_close(out, ref, absprod, rtol=2e-6):
    """tests/test_gemm_gpu.py's bound: |out - ref| <= rtol * sum |a b| elementwise."""
    err = (out.double() - ref).abs()
    bound = rtol * absprod + 1e-30
    assert bool((err <= bound).all()), float((err / bound).max())


def row_exp(G: torch.Tensor) -> torch.Tensor:
    """The fp16x2 row scale exponent (split3.h f16x2_row_exp): max|row| * 2^e in [2^14, 2^15)."""
    m = G.abs().amax(dim=1) if G.shape[0] else G.new_zeros(0)
    e = 15 - torch.frexp(m)[1]
    return torch.where(m == 0, torch.full_like(e, 0x3FFF), e).to(torch.int32)


def _gen(*key):
    g = torch.Generator(device="cuda")
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def _scaled_rows(g, M, cols, lo, hi, zero_from, zero_step):
    """Rows spread over 10^lo .. 10^hi with all-zero rows (as test_gemm_h2 / test_wgrad_h2)."""
    X = _randn(g, M, cols) * torch.pow(10.0, torch.empty(M, 1, device="cuda").uniform_(lo, hi, generator=g))
    X[zero_from::zero_step] = 0
    return X


def _launch_checked(make_out, launch, inputs, what):
    """Two launches on two fresh outputs: guards of every operand intact, no NaN, bitwise repeatable.
    Returns the first output's logical view."""
    from marlsat import _lib

    outs = []
    for _ in range(2):
        o = make_out()
        os_ = o if isinstance(o, tuple) else (o,)
        _lib.check(launch(*os_), what)
        torch.cuda.synchronize()
        for x in os_ + tuple(inputs):
            x.check()
        for x in os_:
            assert not bool(torch.isnan(x.view).any()), "NaN in the output"
        outs.append(tuple(x.view.clone() for x in os_))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "second launch differs"
    return outs[0] if len(outs[0]) > 1 else outs[0][0]


# ------------------------------------------------------------------------------------------------ msat_gemm

def _gemm_data(c):
    g = _gen("gemm", c.M, c.N, c.K, c.transB)  # the placement is not part of the seed: pairs share their data
    A = _randn(g, c.M, c.K)
    B = _randn(g, *((c.N, c.K) if c.transB else (c.K, c.N)))
    return A, B, _randn(g, c.N), _randn(g, c.M, c.N)


def _gemm_run(c, acc, check_ref=True):
    from marlsat import _lib

    A, B, bias, C0 = _gemm_data(c)
    a, b = operand(A, c.a), operand(B, c.b)
    bv = None if c.bias is None else vector(bias, c.bias)
    ins = [a, b] + ([bv] if bv else [])
    s = _lib.stream_ptr()
    C = _launch_checked(
        lambda: operand(C0, c.c, "out"),
        lambda o: _lib.lib.msat_gemm(a.ptr, a.ld, b.ptr, b.ld, c.transB, o.ptr, o.ld, bv.ptr if bv else None, c.M, c.N,
                                     c.K, acc, s), ins, "gemm")
    if check_ref:
        Bop = B.double().t() if c.transB else B.double()
        bd = bias.double() if bv else torch.zeros(c.N, dtype=torch.float64, device="cuda")
        ref = A.double() @ Bop + bd + (C0.double() if acc else 0)
        absprod = A.double().abs() @ Bop.abs() + bd.abs() + (C0.double().abs() if acc else 0)
        _ref_close(C, ref, absprod)
    return C


@pytest.mark.parametrize("c", gp.GEMM_CASES + gp.GEMM_K0_CASES, ids=lambda c: c.name)
def test_gemm_placement(c):
    for acc in (0, 1):
        _gemm_run(c, acc)


@pytest.mark.parametrize("c", gp.GEMM_ACC2_CASES, ids=lambda c: c.name)
def test_gemm_accumulate_is_a_flag(c):
    """Any nonzero accumulate adds: 2 gives bitwise what 1 gives, on each of the three kernels / epilogues."""
    c1, c2 = _gemm_run(c, 1), _gemm_run(c, 2)
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32))


@pytest.mark.parametrize("vec,scalar", gp.GEMM_VEC_SCALAR_PAIRS)
def test_gemm2_epilogues_bitwise_equal(vec, scalar):
    """The float4 and the scalar epilogue of gemm2_kernel follow the same main loop and both add the bias
    first and then C: same A, B, bias and C values at another C / bias placement give the same bits."""
    by = {c.name: c for c in gp.GEMM_CASES}
    for acc in (0, 1):
        cv, cs = _gemm_run(by[vec], acc), _gemm_run(by[scalar], acc)
        assert torch.equal(cv.view(torch.int32), cs.view(torch.int32))


# -------------------------------------------------------------------------------- msat_gemm_wgrad and _rot

def _wgrad_run(c, acc, tail=4096):
    from marlsat import _lib

    g = _gen("wgrad", c.M, c.K, c.N)
    A, G, W0 = _randn(g, c.M, c.K), _randn(g, c.M, c.N), _randn(g, c.K, c.N)
    a, gg = operand(A, c.a), operand(G, c.g)
    ws = workspace(int(_lib.lib.msat_gemm_wgrad_workspace_bytes(c.M, c.K, c.N)), c.ws_off, tail)
    s = _lib.stream_ptr()
    W = _launch_checked(
        lambda: operand(W0, c.w, "out"),
        lambda o: _lib.lib.msat_gemm_wgrad_rot(a.ptr, a.ld, gg.ptr, gg.ld, o.ptr, o.ld, c.M, c.K, c.N, c.rot, acc, ws.ptr,
                                               s) if c.rot else
        _lib.lib.msat_gemm_wgrad(a.ptr, a.ld, gg.ptr, gg.ld, o.ptr, o.ld, c.M, c.K, c.N, acc, ws.ptr, s),
        [a, gg, ws], "wgrad")
    ref = torch.roll(A.double().t() @ G.double(), c.rot, dims=1) + (W0.double() if acc else 0)
    absprod = torch.roll(A.double().abs().t() @ G.double().abs(), c.rot, dims=1) + (W0.double().abs() if acc else 0)
    _ref_close(W, ref, absprod)
    if c.M == 0:  # the contract of the header: zeros, or W unchanged
        assert torch.equal(W, W0 if acc else torch.zeros_like(W0))
    return W


@pytest.mark.parametrize("c", gp.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_placement(c, c_precision):
    c_precision(c.precision)
    for acc in (0, 1):
        _wgrad_run(c, acc)


@pytest.mark.parametrize("c", gp.WGRAD_ROT_CASES, ids=lambda c: c.name)
def test_wgrad_rot_placement(c, c_precision):
    c_precision(c.precision)
    for acc in (0, 1):
        _wgrad_run(c, acc)


def test_wgrad_rot_skinny_two_range_workspace(c_precision):
    """K <= 8 with a rotation: the two-range fallback's 60-column sub-product takes one column block and 625
    row splits, more partial floats than the full 68 columns at 512 splits; msat_gemm_wgrad_workspace_bytes
    must cover it (the canary tail after the workspace stays untouched)."""
    c = gp.WGRAD_ROT_SKINNY_WIDE
    c_precision(c.precision)
    assert gp.two_range_subpaths(c)[0].startswith("skinny/")
    for acc in (0, 1):
        _wgrad_run(c, acc, tail=1 << 16)


@pytest.mark.parametrize("vec,scalar", gp.WGRAD_REDUCE_PAIRS)
def test_wgrad_reduces_bitwise_equal(vec, scalar, c_precision):
    """wgrad_reduce_kernel and wgrad_reduce4_kernel both start from zero and add the splits in ascending
    order, then add W: after the same partial kernel they give the same bits."""
    by = {c.name: c for c in gp.WGRAD_CASES}
    c_precision(by[vec].precision)
    for acc in (0, 1):
        wv, wsc = _wgrad_run(by[vec], acc), _wgrad_run(by[scalar], acc)
        assert torch.equal(wv.view(torch.int32), wsc.view(torch.int32))


# ------------------------------------------------------------------------------------- msat_gemm_wgrad_h2

@pytest.mark.parametrize("c", gp.H2W_CASES, ids=lambda c: c.name)
def test_wgrad_h2_placement(c):
    from marlsat import _lib

    g = _gen("h2w", c.M, c.K, c.N)
    A, W0 = _randn(g, c.M, c.K), _randn(g, c.K, c.N)
    G = _scaled_rows(g, c.M, c.N, -30, 2, 3, 7)
    a, gg, rexp = operand(A, c.a), operand(G, c.g), vector(row_exp(G))
    ws = workspace(int(_lib.lib.msat_gemm_wgrad_workspace_bytes(c.M, c.K, c.N)))
    s = _lib.stream_ptr()
    for acc in (0, 1):
        W = _launch_checked(
            lambda: operand(W0, c.w, "out"),
            lambda o: _lib.lib.msat_gemm_wgrad_h2(a.ptr, a.ld, gg.ptr, gg.ld, rexp.ptr, o.ptr, o.ld, c.M, c.K, c.N, c.rot,
                                                  acc, ws.ptr, s), [a, gg, rexp, ws], "wgrad_h2")
        ref = torch.roll(A.double().t() @ G.double(), c.rot, dims=1) + (W0.double() if acc else 0)
        absprod = torch.roll(A.double().abs().t() @ G.double().abs(), c.rot, dims=1) + (W0.double().abs() if acc else 0)
        _ref_close(W, ref, absprod, rtol=4e-6)
        if c.M == 0:
            assert torch.equal(W, W0 if acc else torch.zeros_like(W0))


# ----------------------------------------------------------------------------- msat_gemm_x3, msat_gemm_h2

def _planes(W, rot):
    from marlsat import _lib

    N, K = W.shape
    p2 = torch.empty(2 * N * K + 8, dtype=torch.int16, device="cuda")
    p3 = torch.empty(3 * N * K + 8, dtype=torch.int16, device="cuda")
    bad = torch.empty(1, dtype=torch.int32, device="cuda")
    s = _lib.stream_ptr()
    _lib.check(_lib.lib.msat_split_f16x2_rot(W.data_ptr(), N, K, K, rot, p2.data_ptr(), bad.data_ptr(), s), "split2")
    _lib.check(_lib.lib.msat_split_bf16x3_rot(W.data_ptr(), N, K, K, rot, p3.data_ptr(), s), "split3")
    return p2, p3, bad


@pytest.mark.parametrize("c", gp.X3_CASES, ids=lambda c: c.name)
def test_gemm_x3_placement(c):
    from marlsat import _lib

    g = _gen("x3", c.M, c.N, c.K)
    A = _randn(g, c.M, c.K) * torch.exp2(torch.randint(-6, 7, (c.M, c.K), device="cuda", generator=g).float())
    W, bias, C0 = _randn(g, c.N, c.K), _randn(g, c.N), _randn(g, c.M, c.N)
    _, p3, _ = _planes(W, 0)
    a = operand(A, c.a)
    bv = None if c.bias is None else vector(bias, c.bias)
    s = _lib.stream_ptr()
    bd = bias.double() if bv else torch.zeros(c.N, dtype=torch.float64, device="cuda")
    for acc in (0, 1):
        C = _launch_checked(
            lambda: operand(C0, c.c, "out"),
            lambda o: _lib.lib.msat_gemm_x3(a.ptr, a.ld, p3.data_ptr(), o.ptr, o.ld, bv.ptr if bv else None, c.M, c.N,
                                            c.K, acc, s), [a] + ([bv] if bv else []), "gemm_x3")
        ref = A.double() @ W.double().t() + bd + (C0.double() if acc else 0)
        absprod = A.double().abs() @ W.double().abs().t() + bd.abs() + (C0.double().abs() if acc else 0)
        _ref_close(C, ref, absprod)


@pytest.mark.parametrize("c", gp.H2_CASES, ids=lambda c: c.name)
def test_gemm_h2_placement(c):
    from marlsat import _lib

    g = _gen("h2", c.M, c.N, c.K)
    A = _scaled_rows(g, c.M, c.K, -30, 2, 2, 5)
    W, bias, C0 = _randn(g, c.N, c.K) * 0.1, _randn(g, c.N), _randn(g, c.M, c.N)
    p2, p3, bad = _planes(W, c.rot)
    assert int(bad) == 0
    a, rexp = operand(A, c.a), vector(row_exp(A))
    bv = None if c.bias is None else vector(bias, c.bias)
    s = _lib.stream_ptr()
    bd = bias.double() if bv else torch.zeros(c.N, dtype=torch.float64, device="cuda")
    Wr = torch.roll(W.double(), -c.rot, dims=1)  # planes hold W[:, (k + rot) % K]
    for acc in (0, 1):
        C = _launch_checked(
            lambda: operand(C0, c.c, "out"),
            lambda o: _lib.lib.msat_gemm_h2(a.ptr, a.ld, rexp.ptr, p2.data_ptr(), p3.data_ptr(), bad.data_ptr(), o.ptr,
                                            o.ld, bv.ptr if bv else None, c.M, c.N, c.K, acc, s),
            [a, rexp] + ([bv] if bv else []), "gemm_h2")
        ref = A.double() @ Wr.t() + bd + (C0.double() if acc else 0)
        absprod = A.double().abs() @ Wr.abs().t() + bd.abs() + (C0.double().abs() if acc else 0)
        _ref_close(C, ref, absprod)


# --------------------------------------------------------- msat_gemm_h2_dual, msat_gemm_wgrad_h2_dual

def _dual_data(c):
    H = c.H
    g = _gen("dual", c.M, c.K1)
    D = _scaled_rows(g, c.M, 4 * H, -12, 1, 5, 7)
    return g, operand(D, c.d), D, vector(row_exp(D))


@pytest.mark.parametrize("c", [c for c in gp.DUAL_CASES if c.M > 0], ids=lambda c: c.name)
def test_gemm_h2_dual_placement(c):
    """dh (+)= D[:, H:] @ Wh^T and dx (+)= D[:, :3H] @ F^T from one packed buffer D (M x 4H) with NaN in its
    ld gap and guard rows; both outputs strided."""
    from marlsat import _lib

    H, K1, M = c.H, c.K1, c.M
    g, d, D, rexp = _dual_data(c)
    Wh, F = _randn(g, H, 3 * H) * 0.1, _randn(g, K1, 3 * H) * 0.1
    pl0, pl1 = _planes(Wh, 0), _planes(F, 2 * H)
    C0, C1 = _randn(g, M, H), _randn(g, M, K1)
    s = _lib.stream_ptr()
    dgh, dgi = D[:, H:].double(), D[:, :3 * H].double()
    Fr = torch.roll(F.double(), -2 * H, dims=1)
    for acc in (0, 1):
        dh, dx = _launch_checked(
            lambda: (operand(C0, c.c0, "out"), operand(C1, c.c1, "out")),
            lambda o0, o1: _lib.lib.msat_gemm_h2_dual(
                d.ptr + 4 * H, d.ld, pl0[0].data_ptr(), pl0[1].data_ptr(), pl0[2].data_ptr(), o0.ptr, o0.ld, H, acc,
                d.ptr, d.ld, pl1[0].data_ptr(), pl1[1].data_ptr(), pl1[2].data_ptr(), o1.ptr, o1.ld, K1, acc,
                rexp.ptr, M, 3 * H, s), [d, rexp], "gemm_h2_dual")
        _ref_close(dh, dgh @ Wh.double().t() + (C0.double() if acc else 0),
                   dgh.abs() @ Wh.double().abs().t() + (C0.double().abs() if acc else 0))
        _ref_close(dx, dgi @ Fr.t() + (C1.double() if acc else 0),
                   dgi.abs() @ Fr.abs().t() + (C1.double().abs() if acc else 0))


def _ld4(p: Placement) -> Placement:
    """An input of the dual weight gradient must keep ld % 4 == 0 and 16-byte alignment."""
    return p if p.pad % 4 == 0 and p.off % 4 == 0 else Placement()


@pytest.mark.parametrize("c", gp.DUAL_CASES, ids=lambda c: c.name)
def test_wgrad_h2_dual_placement(c):
    """dWh (+)= h^T D[:, H:] and dF (+)= x^T D[:, :3H] rotated by 2H, W strided on one or both sides
    (ldw % 4 != 0 on either takes the separate scalar reduces instead of the dual float4 one).

    M = 1 is the case that made wgrad_w_body scale A by 2^8 before its fp16 split (gemm_x3.hip kWgA): unscaled,
    dF row k = 24 (|x| = 0.00593) measured err / (4e-6 |x g|) = 1.0152, the lo half of the split sitting on
    fp16's subnormal grid; with one row nothing averages that out."""
    from marlsat import _lib

    H, K1, M = c.H, c.K1, c.M
    g, d, D, rexp = _dual_data(c)
    hx, xx = _randn(g, M, H), _randn(g, M, K1)
    W0, W1 = _randn(g, H, 3 * H), _randn(g, K1, 3 * H)
    h, x = operand(hx, _ld4(c.c0)), operand(xx, _ld4(c.c1))
    ws = workspace(int(_lib.lib.msat_gemm_wgrad_dual_workspace_bytes(M, H, 3 * H, K1, 3 * H)))
    s = _lib.stream_ptr()
    dgh, dgi = D[:, H:].double(), D[:, :3 * H].double()
    for acc in (0, 1):
        g0, g1 = _launch_checked(
            lambda: (operand(W0, c.w0, "out"), operand(W1, c.w1, "out")),
            lambda o0, o1: _lib.lib.msat_gemm_wgrad_h2_dual(
                h.ptr, h.ld, d.ptr + 4 * H, d.ld, o0.ptr, o0.ld, H, 3 * H, 0,
                x.ptr, x.ld, d.ptr, d.ld, o1.ptr, o1.ld, K1, 3 * H, 2 * H, rexp.ptr, M, acc, ws.ptr, s),
            [h, x, d, rexp, ws], "wgrad_h2_dual")
        _ref_close(g0, hx.double().t() @ dgh + (W0.double() if acc else 0),
                   hx.double().abs().t() @ dgh.abs() + (W0.double().abs() if acc else 0), rtol=4e-6)
        _ref_close(g1, torch.roll(xx.double().t() @ dgi, 2 * H, dims=1) + (W1.double() if acc else 0),
                   torch.roll(xx.double().abs().t() @ dgi.abs(), 2 * H, dims=1) + (W1.double().abs() if acc else 0),
                   rtol=4e-6)
        if M == 0:
            assert torch.equal(g0, W0 if acc else torch.zeros_like(W0))
            assert torch.equal(g1, W1 if acc else torch.zeros_like(W1))


# ---------------------------------------------------------------------------------------------- msat_colsum

@pytest.mark.parametrize("c", gp.COLSUM_CASES, ids=lambda c: c.name)
def test_colsum_placement(c):
    """The placements of test_colsum_deterministic with NaN in G's ld gap and guard rows and a canary around
    the output."""
    from marlsat import _lib

    g = _gen("colsum", c.M, c.N)
    G, out0 = _randn(g, c.M, c.N), _randn(g, c.N)
    gg = operand(G, c.g)
    ws = workspace(4 * int(_lib.lib.msat_colsum_workspace_floats(c.M, c.N)))
    s = _lib.stream_ptr()
    for acc in (0, 1):
        out = _launch_checked(lambda: vector(out0, c.out_off, "out"),
                              lambda o: _lib.lib.msat_colsum(gg.ptr, gg.ld, c.M, c.N, o.ptr, acc, ws.ptr, s), [gg, ws],
                              "colsum")
        ref = G.double().sum(0) + (out0.double() if acc else 0)
        err = (out.double() - ref).abs()
        assert bool((err <= 2e-6 * G.double().abs().sum(0) + 1e-6).all())
