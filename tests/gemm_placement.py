"""Operand placements for the matrix-product tests: where an operand sits, not what shape it has.

The matrix-product exports pick their kernel from the operands' placement as well as from M, N and K:
16-byte alignment of each pointer, ``ld % 4`` of each leading dimension, the alignment of bias and
workspace.  This module holds what the placement tests share:

* ``Placement``: (offset in floats from a 16-byte aligned base, leading dimension) of one operand;
* ``operand`` / ``vector`` (fp32 or int32) / ``workspace``: device buffers with the logical operand inside
  guard rows and ``ld - cols`` gaps -- NaN around inputs, a canary bit pattern around outputs -- and a
  ``check()`` that asserts guards and gaps bit-identical afterwards (torch is imported only there, so the
  case tables and ``expected_path`` load on a machine without a GPU);
* ``expected_path``: a host-only restatement of the dispatch predicates, used ONLY to prove that the case
  tables below reach every branch (tests/test_gemm_placement_cpu.py).  No test derives an expected number
  from it;
* the case tables, one per export: an all-aligned, tightly packed base case, one placement factor varied at
  a time, and a few all-misaligned combinations.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Tuple

GUARD_ROWS = 16
CANARY = 0x7FC5A5A5  # a quiet NaN with a payload: an output guard that reaches arithmetic also poisons it
REXP_POISON = -(1 << 20)  # a guard row exponent: picked up by a split's minimum, it flushes the product to zero
SKINNY_K = 8   # gemm.hip kSkinnyK
WW_N = 384     # gemm_x3.hip kWWN


@dataclass(frozen=True)
class Placement:
    off: int = 0          # floats from a 16-byte aligned base
    pad: int = 0          # leading dimension = minimum + pad

    def aligned(self) -> bool:
        return self.off % 4 == 0


P0 = Placement()


# ----------------------------------------------------------------------------------------------------------
# operand builders (device)

@dataclass
class Operand:
    buf: "object"            # the whole flat buffer
    view: "object"           # (rows, cols) strided view of the logical operand
    ptr: int
    ld: int
    check: Callable[[], None]


def _fill_pattern(torch, n, kind, dtype, fill=None):
    if dtype == torch.int32:
        return torch.full((n,), REXP_POISON, dtype=torch.int32, device="cuda")
    if kind == "in":
        return torch.full((n,), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    return torch.full((n,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def operand(data, place: Placement = P0, kind: str = "in", min_ld: Optional[int] = None,
            fill: Optional[float] = None) -> Operand:
    """Place the (rows, cols) tensor `data` at `place` inside a larger buffer: GUARD_ROWS rows of ld elements
    before and after it and the ld - cols gap in every row, NaN (kind 'in'; `fill` puts a finite value there
    instead) or the canary pattern (kind 'out').  check() asserts everything outside the view bit-identical
    to what it was when built."""
    import torch

    rows, cols = data.shape
    ld = (cols if min_ld is None else min_ld) + place.pad
    assert ld >= cols and data.dtype in (torch.float32, torch.int32)
    n = place.off + (2 * GUARD_ROWS + max(rows, 1)) * ld + 4
    buf = _fill_pattern(torch, n, kind, data.dtype, fill)
    assert buf.data_ptr() % 16 == 0
    start = place.off + GUARD_ROWS * ld  # GUARD_ROWS * ld * 4 bytes is a multiple of 16: alignment = off's
    view = buf.as_strided((rows, cols), (ld, 1), start)
    view.copy_(data)
    outside = torch.ones(n, dtype=torch.bool, device="cuda")
    outside.as_strided((rows, cols), (ld, 1), start).fill_(False)
    bits = buf.view(torch.int32)
    snap = bits[outside].clone()

    def check():
        assert torch.equal(bits[outside], snap), f"{kind}put guard rows / ld gaps changed"

    return Operand(buf, view, buf.data_ptr() + 4 * start, ld, check)


def vector(data, off: int = 0, kind: str = "in", fill: Optional[float] = None) -> Operand:
    """A 1-D operand (bias, colsum output, row exponents) with GUARD_ROWS * len guard entries either side."""
    op = operand(data.view(1, -1), Placement(off, 0), kind, fill=fill)
    op.view = op.view.view(-1)
    return op


def workspace(nbytes: int, off: int = 0, tail: int = 4096) -> Operand:
    """A workspace of `nbytes` (+ the slack one float of offset needs) followed by `tail` canary floats that
    must stay untouched; off = 1 hands the library a pointer one float past 16-byte alignment."""
    import torch

    nf = (nbytes + 3) // 4
    buf = torch.full((off + nf + tail,), CANARY, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    tl = buf[off + nf:]

    def check():
        assert bool((tl == CANARY).all()), "wrote past the workspace"
        assert bool((buf[:off] == CANARY).all()), "wrote before the workspace"

    return Operand(buf, buf[off:off + nf], buf.data_ptr() + 4 * off, 0, check)


# ----------------------------------------------------------------------------------------------------------
# expected_path: the dispatch, restated.  Sources (marl-sat_amd/csrc):
#   gemm2.hip  msat_gemm2_ok       K % 32, K != 0, lda % 4, ldb % 4, aligned A and B, N % 4 for B[K][N], N >= 4
#   gemm2.hip  msat_gemm2_launch   vec = N % 4 == 0 && ldc % 4 == 0 && aligned C && (no bias || aligned bias)
#   gemm2.hip  msat_wgrad2_ok      K % 4, N % 4, K >= 4, N >= 4, lda % 4, ldg % 4, aligned A and G
#   gemm_x3.hip msat_wgrad_x3_ok   K % 4, N % 4, K >= 16, lda % 4, ldg % 4, aligned A and G
#   gemm_x3.hip msat_wgrad_x3w_ok  N <= kWWN (384) && msat_wgrad_x3_ok
#   gemm_x3.hip msat_gemm_x3       K % 32 == 0 -> gemm_x3r16_kernel else gemm_x3_kernel; vec as gemm2's
#   gemm_x3.hip msat_gemm_h2, gemm_h2_dual_impl   vec_out per product (the dual has no bias)
#   gemm.hip   skinny_ok           K <= 8, N % 4, ldg % 4, ldw % 4, aligned G and W (+ aligned workspace at the call)
#   gemm.hip   msat_gemm_wgrad     x3w, then skinny (av = lda % 4 == 0 && aligned A), then x3 tiles / wgrad2 / generic
#   gemm.hip   wgrad_reduce        float4 when N % 4 == 0 && ldw % 4 == 0 && aligned W and partials
#   gemm.hip   msat_gemm_wgrad_rot rot == 0 -> msat_gemm_wgrad; x3w with the rotated store when rot % 4 == 0;
#                                  else two column ranges through msat_gemm_wgrad
#   gemm.hip   wgrad_h2_dual_impl  one dual float4 reduce when both sides allow float4, else one reduce each
#   gnn_kernels.hip colsum_det    float4 when N % 4 == 0 && ldg % 4 == 0 && aligned G, out and workspace

def _al(p: Placement) -> bool:
    return p.off % 4 == 0


def _wgrad_x3_ok(a, lda, g, ldg, K, N):
    return K % 4 == 0 and N % 4 == 0 and K >= 16 and lda % 4 == 0 and ldg % 4 == 0 and _al(a) and _al(g)


def _wgrad2_ok(a, lda, g, ldg, K, N):
    return K % 4 == 0 and N % 4 == 0 and K >= 4 and N >= 4 and lda % 4 == 0 and ldg % 4 == 0 and _al(a) and _al(g)


def _reduce(w, ldw, N, ws_off):
    return "reduce4" if N % 4 == 0 and ldw % 4 == 0 and _al(w) and ws_off % 4 == 0 else "reduce_scalar"


def _vec_out(c, ldc, N, bias):
    return N % 4 == 0 and ldc % 4 == 0 and _al(c) and (bias is None or bias % 4 == 0)


def _wgrad_path(c: "WgradCase", N=None, w_shift=0, g_shift=0) -> str:
    N = c.N if N is None else N
    a, g, w = c.a, replace(c.g, off=c.g.off + g_shift), replace(c.w, off=c.w.off + w_shift)
    lda, ldg, ldw = c.K + a.pad, c.N + g.pad, c.N + w.pad
    x3 = c.precision != "fp32"
    K = c.K
    if x3 and K > SKINNY_K and N <= WW_N and _wgrad_x3_ok(a, lda, g, ldg, K, N):
        return "x3w/" + _reduce(w, ldw, N, c.ws_off)
    if (K <= SKINNY_K and N % 4 == 0 and ldg % 4 == 0 and ldw % 4 == 0 and _al(g) and _al(w)
            and c.ws_off % 4 == 0):
        return "skinny/av" if lda % 4 == 0 and _al(a) else "skinny/scalarA"
    if x3 and _wgrad_x3_ok(a, lda, g, ldg, K, N):
        part = "x3_tiles"
    elif _wgrad2_ok(a, lda, g, ldg, K, N):
        part = "wgrad2"
    else:
        part = "wgrad_generic"
    return part + "/" + _reduce(w, ldw, N, c.ws_off)


def expected_path(export: str, c) -> str:
    if export == "msat_gemm":
        lda, ldb, ldc = c.K + c.a.pad, (c.K if c.transB else c.N) + c.b.pad, c.N + c.c.pad
        ok = (c.K % 32 == 0 and c.K != 0 and lda % 4 == 0 and ldb % 4 == 0 and _al(c.a) and _al(c.b)
              and (c.transB or c.N % 4 == 0) and c.N >= 4)
        if not ok:
            return "gemm_kernel"
        return "gemm2/vec" if _vec_out(c.c, ldc, c.N, c.bias) else "gemm2/scalar"
    if export == "msat_gemm_wgrad":
        return _wgrad_path(c)
    if export == "msat_gemm_wgrad_rot":
        if c.rot == 0:
            return _wgrad_path(c)
        lda, ldg, ldw = c.K + c.a.pad, c.N + c.g.pad, c.N + c.w.pad
        if (c.precision != "fp32" and c.K > SKINNY_K and c.rot % 4 == 0 and c.N <= WW_N
                and _wgrad_x3_ok(c.a, lda, c.g, ldg, c.K, c.N)):
            return "x3w_rot/" + _reduce(c.w, ldw, c.N, c.ws_off)
        return "two_range"
    if export == "msat_gemm_wgrad_h2":
        return "h2w/" + _reduce(c.w, c.N + c.w.pad, c.N, 0)
    if export == "msat_gemm_wgrad_h2_dual":
        r0 = _reduce(c.w0, 3 * c.H + c.w0.pad, 3 * c.H, 0)
        r1 = _reduce(c.w1, 3 * c.H + c.w1.pad, 3 * c.H, 0)
        return "h2w_dual/reduce4_dual" if r0 == r1 == "reduce4" else f"h2w_dual/{r0}+{r1}"
    if export in ("msat_gemm_x3", "msat_gemm_h2"):
        vec = "vec" if _vec_out(c.c, c.N + c.c.pad, c.N, c.bias) else "scalar"
        if export == "msat_gemm_h2":
            return "h2r16/" + vec
        return ("x3r16/" if c.K % 32 == 0 else "x3lds/") + vec
    if export == "msat_gemm_h2_dual":
        v = ["vec" if _vec_out(p, n + p.pad, n, None) else "scalar" for p, n in ((c.c0, c.H), (c.c1, c.K1))]
        return "h2r16_dual/" + "+".join(v)
    if export == "msat_colsum":
        vec = c.N % 4 == 0 and (c.N + c.g.pad) % 4 == 0 and _al(c.g) and c.out_off % 4 == 0
        return "colsum/vec" if vec else "colsum/scalar"
    raise KeyError(export)


def two_range_subpaths(c: "WgradCase") -> Tuple[str, str]:
    """The two msat_gemm_wgrad calls of msat_gemm_wgrad_rot's fallback: W + rot over N - rot columns, then
    G + (N - rot) over rot columns."""
    return _wgrad_path(c, N=c.N - c.rot, w_shift=c.rot), _wgrad_path(c, N=c.rot, g_shift=c.N - c.rot)


_RED = ("reduce4", "reduce_scalar")
BRANCHES: Dict[str, List[str]] = {
    "msat_gemm": ["gemm2/vec", "gemm2/scalar", "gemm_kernel"],
    "msat_gemm_wgrad": [f"{p}/{r}" for p in ("x3w", "x3_tiles", "wgrad2", "wgrad_generic") for r in _RED]
                       + ["skinny/av", "skinny/scalarA"],
    "msat_gemm_wgrad_rot": [f"x3w_rot/{r}" for r in _RED] + ["two_range"],
    "msat_gemm_wgrad_h2": [f"h2w/{r}" for r in _RED],
    "msat_gemm_wgrad_h2_dual": ["h2w_dual/reduce4_dual", "h2w_dual/reduce_scalar+reduce4",
                                "h2w_dual/reduce4+reduce_scalar", "h2w_dual/reduce_scalar+reduce_scalar"],
    "msat_gemm_x3": ["x3r16/vec", "x3r16/scalar", "x3lds/vec", "x3lds/scalar"],
    "msat_gemm_h2": ["h2r16/vec", "h2r16/scalar"],
    "msat_gemm_h2_dual": ["h2r16_dual/vec+vec", "h2r16_dual/scalar+vec", "h2r16_dual/vec+scalar"],
    "msat_colsum": ["colsum/vec", "colsum/scalar"],
}
# the sub-products of the two-range fallback that the _rot table must reach (both fast and generic partials)
TWO_RANGE_SUBPATHS = ["x3w/reduce4", "wgrad_generic/reduce_scalar", "wgrad2/reduce4", "skinny/av"]


# ----------------------------------------------------------------------------------------------------------
# case tables

def _id(**kw) -> str:
    return "-".join(f"{k}{v}" for k, v in kw.items())


@dataclass(frozen=True)
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    transB: int
    a: Placement = P0
    b: Placement = P0
    c: Placement = P0
    bias: Optional[int] = 0   # offset of the bias in floats, None: no bias


def _gemm_factors(M, N, K, transB) -> List[GemmCase]:
    base = GemmCase(_id(M=M, N=N, K=K, t=transB), M, N, K, transB)
    out = [base]
    for f, v in (("a", Placement(1, 0)), ("b", Placement(1, 0)), ("c", Placement(1, 0)), ("bias", 1), ("bias", None),
                 ("a", Placement(0, 1)), ("a", Placement(0, 4)), ("b", Placement(0, 1)), ("b", Placement(0, 4)),
                 ("c", Placement(0, 1)), ("c", Placement(0, 4))):
        tag = f"{f}{'none' if v is None else v if isinstance(v, int) else f'o{v.off}p{v.pad}'}"
        out.append(replace(base, name=base.name + "-" + tag, **{f: v}))
    return out


def _gemm_cases() -> List[GemmCase]:
    out: List[GemmCase] = []
    # one placement factor at a time on the smallest shapes with a second row tile and a column tail
    out += _gemm_factors(129, 130, 32, 1)
    out += _gemm_factors(129, 132, 64, 0)
    # the remaining shapes at the base placement and all-misaligned
    mis = dict(a=Placement(1, 1), b=Placement(3, 1), c=Placement(2, 1), bias=3)
    for M, N, K, t in [(1, 6, 32, 1), (1, 4, 32, 0), (129, 6, 64, 1), (1, 130, 64, 1), (1, 132, 32, 0),
                       (129, 4, 64, 0), (129, 130, 36, 1), (129, 132, 36, 0), (1, 6, 36, 1)]:
        base = GemmCase(_id(M=M, N=N, K=K, t=t), M, N, K, t)
        out += [base, replace(base, name=base.name + "-mis", **mis),
                replace(base, name=base.name + "-co1", c=Placement(1, 0)),
                replace(base, name=base.name + "-ao1", a=Placement(1, 0))]
    return out


GEMM_CASES = _gemm_cases()
# accumulate = 2 must equal accumulate = 1 bitwise: one case on each of the three paths
GEMM_ACC2_CASES = [c for c in GEMM_CASES if c.name in ("M129-N132-K64-t0", "M129-N130-K32-t1",
                                                        "M129-N132-K64-t0-ao1p0")]
GEMM_K0_CASES = [GemmCase(_id(M=M, N=N, K=0, t=t) + f"-bias{b}", M, N, 0, t, bias=b)
                 for M, N, t in [(129, 130, 1), (1, 4, 0)] for b in (0, None)]
# gemm2/vec against gemm2/scalar on the same A and B: only C's and the bias's placement differ
GEMM_VEC_SCALAR_PAIRS = [("M129-N132-K64-t0", s) for s in ("M129-N132-K64-t0-co1p0", "M129-N132-K64-t0-co0p1",
                                                           "M129-N132-K64-t0-bias1")]


@dataclass(frozen=True)
class WgradCase:
    name: str
    M: int
    K: int
    N: int
    precision: str = "fp16x2"
    a: Placement = P0
    g: Placement = P0
    w: Placement = P0
    ws_off: int = 0
    rot: int = 0


_WGRAD_FACTORS = [("a", Placement(1, 0)), ("g", Placement(1, 0)), ("w", Placement(1, 0)), ("ws_off", 1),
                  ("a", Placement(0, 1)), ("a", Placement(0, 4)), ("g", Placement(0, 1)), ("g", Placement(0, 4)),
                  ("w", Placement(0, 1)), ("w", Placement(0, 4))]
_WGRAD_MIS = dict(a=Placement(1, 1), g=Placement(2, 1), w=Placement(3, 1), ws_off=1)


def _tag(f, v) -> str:
    return f"{f}{v}" if isinstance(v, int) else f"{f}o{v.off}p{v.pad}"


def _wgrad_cases(rots=(0,)) -> List[WgradCase]:
    out: List[WgradCase] = []
    for prec in ("fp16x2", "fp32"):
        for rot in rots:
            # every factor on the smallest whole-row shape, on the tiled shape past 384 columns only those
            # that change its path (each of its cases stages 1025 x 388 operands)
            for (M, K, N), factors in [((513, 16, 8), _WGRAD_FACTORS), ((1025, 128, 388), _WGRAD_FACTORS[:4]),
                                       ((513, 8, 8), _WGRAD_FACTORS), ((1025, 12, 36), _WGRAD_FACTORS[:4])]:
                base = WgradCase(_id(p=prec, M=M, K=K, N=N, r=rot), M, K, N, prec, rot=rot)
                out.append(base)
                out += [replace(base, name=base.name + "-" + _tag(f, v), **{f: v}) for f, v in factors]
                out.append(replace(base, name=base.name + "-mis", **_WGRAD_MIS))
            for M, K, N in [(1, 16, 8), (1025, 16, 8), (1, 132, 128), (513, 132, 128), (1, 12, 36), (513, 12, 36),
                            (1, 128, 388), (1, 3, 8), (513, 3, 8), (1025, 3, 8), (1, 8, 8), (1025, 8, 8),
                            (0, 16, 8), (0, 128, 388), (0, 3, 8), (0, 12, 36)]:
                base = WgradCase(_id(p=prec, M=M, K=K, N=N, r=rot), M, K, N, prec, rot=rot)
                out += [base, replace(base, name=base.name + "-mis", **_WGRAD_MIS),
                        replace(base, name=base.name + "-wo0p1", w=Placement(0, 1))]
    return out


WGRAD_CASES = _wgrad_cases()
WGRAD_ROT_CASES = _wgrad_cases(rots=(4, 6))
# .../reduce4 against .../reduce_scalar after the same partial kernel: only W's placement differs
_WGRAD_PAIR_SHAPES = ["M513-K16-N8", "M1025-K128-N388", "M1025-K12-N36"]
WGRAD_REDUCE_PAIRS = [(f"p{p}-{s}-r0", f"p{p}-{s}-r0-{t}") for p in ("fp16x2", "fp32") for s in _WGRAD_PAIR_SHAPES
                      for t in ("wo1p0", "ws_off1")]
# the workspace of the two-range fallback at K <= 8: the narrower sub-product takes more splits than the full
# width (60 columns: one column block, 626 splits; 68 columns: two column blocks, 512 splits)
WGRAD_ROT_SKINNY_WIDE = WgradCase("skinny-two-range-workspace", 40000, 3, 68, "fp16x2", rot=8)


@dataclass(frozen=True)
class H2wCase:
    name: str
    M: int
    K: int
    N: int
    rot: int
    a: Placement = P0
    g: Placement = P0
    w: Placement = P0


def _h2w_cases() -> List[H2wCase]:
    out = []
    for M in (1, 385, 513, 0):
        base = H2wCase(_id(M=M), M, 128, 384, 256)
        out.append(base)
        if M in (0, 1):
            out.append(replace(base, name=base.name + "-wp1", w=Placement(0, 1)))
            continue
        for f, v in [("a", Placement(0, 4)), ("a", Placement(0, 8)), ("g", Placement(0, 4)), ("g", Placement(0, 8)),
                     ("w", Placement(0, 4)), ("w", Placement(0, 8)), ("w", Placement(0, 1)), ("w", Placement(1, 0)),
                     ("a", Placement(4, 0)), ("g", Placement(8, 4)), ("w", Placement(12, 4))]:
            out.append(replace(base, name=base.name + "-" + _tag(f, v), **{f: v}))
    out.append(H2wCase("M513-K16-N260", 513, 16, 260, 4, g=Placement(4, 8), w=Placement(0, 1)))
    return out


H2W_CASES = _h2w_cases()


@dataclass(frozen=True)
class X3Case:
    name: str
    M: int
    N: int
    K: int
    a: Placement = P0
    c: Placement = P0
    bias: Optional[int] = 0
    rot: int = 0          # msat_gemm_h2 only: the planes' column rotation


def _x3_cases(shapes, rot) -> List[X3Case]:
    out = []
    for M, N, K in shapes:
        base = X3Case(_id(M=M, N=N, K=K), M, N, K, rot=rot if rot < K else 32)
        out.append(base)
        for f, v in [("a", Placement(0, 4)), ("a", Placement(0, 8)), ("c", Placement(0, 4)), ("c", Placement(0, 8)),
                     ("a", Placement(4, 4)), ("c", Placement(8, 4)), ("bias", 4), ("bias", None),
                     ("c", Placement(0, 1)), ("c", Placement(1, 0)), ("bias", 1)]:
            tag = "biasnone" if v is None else _tag(f, v)
            out.append(replace(base, name=base.name + "-" + tag, **{f: v}))
    return out


X3_CASES = _x3_cases([(385, 128, 384), (513, 130, 96), (1, 128, 48), (385, 130, 48)], 0)
H2_CASES = _x3_cases([(385, 128, 384), (513, 130, 96), (1, 128, 384)], 256)


@dataclass(frozen=True)
class DualCase:
    name: str
    M: int
    K1: int
    H: int = 128
    d: Placement = P0      # the packed rows D (M x 4H): both products read column slices of it
    c0: Placement = P0     # dh / h
    c1: Placement = P0     # dx / x
    w0: Placement = P0     # dWh
    w1: Placement = P0     # dF


def _dual_cases() -> List[DualCase]:
    out = []
    for M, K1 in [(1, 128), (385, 256), (513, 128), (0, 128)]:
        base = DualCase(_id(M=M, K1=K1), M, K1)
        out.append(base)
        if M == 1:
            continue
        for f, v in [("d", Placement(0, 4)), ("d", Placement(8, 8)), ("c0", Placement(0, 4)), ("c1", Placement(4, 8)),
                     ("w0", Placement(0, 4)), ("w1", Placement(0, 8)), ("w0", Placement(0, 1)), ("w1", Placement(0, 1)),
                     ("c0", Placement(0, 1)), ("c1", Placement(0, 1))]:
            out.append(replace(base, name=base.name + "-" + _tag(f, v), **{f: v}))
        out.append(replace(base, name=base.name + "-w01p1", w0=Placement(0, 1), w1=Placement(0, 1)))
    return out


DUAL_CASES = _dual_cases()


@dataclass(frozen=True)
class ColsumCase:
    name: str
    M: int
    N: int
    g: Placement = P0
    out_off: int = 0


# the placements of test_colsum_deterministic (tests/test_gemm_gpu.py), here inside NaN gaps and guard rows
COLSUM_CASES = [ColsumCase(_id(M=M, N=N, ld=N + p, off=o), M, N, Placement(o, p), o % 4)
                for M, N, p, o in [(1, 4, 0, 0), (2100, 128, 128, 128), (500, 384, 0, 0), (777, 7, 2, 1),
                                   (0, 8, 0, 0), (100, 130, 2, 2)]]

TABLES = {
    "msat_gemm": GEMM_CASES, "msat_gemm_wgrad": WGRAD_CASES, "msat_gemm_wgrad_rot": WGRAD_ROT_CASES,
    "msat_gemm_wgrad_h2": H2W_CASES, "msat_gemm_wgrad_h2_dual": DUAL_CASES, "msat_gemm_x3": X3_CASES,
    "msat_gemm_h2": H2_CASES, "msat_gemm_h2_dual": DUAL_CASES, "msat_colsum": COLSUM_CASES,
}
