"""What the fused GRU + LayerNorm forward tests share (no test functions here).

* ``_ref_gru_ln``: the one torch restatement of flax nn.GRUCell + nn.LayerNorm (any dtype);
* ``build_planes``: the transposed bf16x3 / fp16x2 weight planes of the register-A kernels;
* ``gru_data`` / ``reference``: deterministic CPU inputs of a case and their float64 result, tape and
  sum|terms|;
* ``_fwd``: one launch of msat_gru_ln_fused_fwd / _x3r / _h2r with every operand placed by a
  ``gemm_placement.Placement`` inside guard rows and ld gaps (NaN or 1e30 around inputs, the canary pattern
  around outputs), guards asserted intact afterwards;
* the case tables, built as the matrix-product tables are: a tight all-aligned base case, one factor varied
  at a time, a few combinations.  Every case carries the names of the factors it exercises (``tags``);
  tests/test_gru_fused_placement_cpu.py proves that the tables name every factor the tests promise.

torch is imported inside the functions only: the tables load on a machine without a GPU.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import List, Optional, Tuple

from gemm_placement import P0, Placement, operand, vector

HUGE = 1.0e30           # the finite guard fill: a leaked read times a zero weight stays finite, but raises a range flag
LAYOUTS = (("plain", 64), ("plain", 128), ("plain", 256), ("x3r", 128), ("h2r", 128))
TILE = {"plain": 64, "x3r": 128, "h2r": 128}


def _ref_gru_ln(x, h, wi, bi, wh, bh, sc, lb, H):
    import torch

    gi = x @ wi + bi
    gh = h @ wh + bh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    hn = (1 - z) * n + z * h
    mean = hn.mean(-1, keepdim=True)
    # flax's LayerNorm clamps its E[x^2] - E[x]^2 variance at 0, as the kernels do; in float64 this changes
    # nothing, the float32 restatement of a near-constant row would take the root of a negative number without
    var = ((hn * hn).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    return (hn - mean) * torch.rsqrt(var + 1e-6) * sc + lb, gi, gh


def build_planes(wi, wh, H, layout, kxp=None):
    """The weight planes of the register-A kernels from contiguous device weights wi (Kx, 3H), wh (H, 3H):
    bf16x3 planes (pi, ph) for 'x3r', in addition fp16x2 planes (qi, qh) and the two split flags `bad`
    (pre-set to 7) for 'h2r'.  kxp: Wi^T's padded depth, default the smallest multiple of 32 >= Kx."""
    import torch

    from marlsat import _lib

    K = wi.shape[0]
    kxp = (K + 31) // 32 * 32 if kxp is None else kxp
    s = _lib.stream_ptr()
    p = SimpleNamespace(kxp=kxp, qi=None, qh=None, bad=None)
    p.pi = torch.empty(3 * 3 * H * kxp + 8, dtype=torch.int16, device="cuda")
    p.ph = torch.empty(3 * 3 * H * H + 8, dtype=torch.int16, device="cuda")
    _lib.check(_lib.lib.msat_split_bf16x3_t(wi.data_ptr(), K, 3 * H, 3 * H, kxp, p.pi.data_ptr(), s), "split_t")
    _lib.check(_lib.lib.msat_split_bf16x3_t(wh.data_ptr(), H, 3 * H, 3 * H, H, p.ph.data_ptr(), s), "split_t")
    if layout == "h2r":
        p.qi = torch.empty(2 * 3 * H * kxp + 8, dtype=torch.int16, device="cuda")
        p.qh = torch.empty(2 * 3 * H * H + 8, dtype=torch.int16, device="cuda")
        p.bad = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib.msat_split_f16x2_t(wi.data_ptr(), K, 3 * H, 3 * H, kxp, p.qi.data_ptr(), p.bad.data_ptr(),
                                               s), "split_f16x2_t")
        _lib.check(_lib.lib.msat_split_f16x2_t(wh.data_ptr(), H, 3 * H, 3 * H, H, p.qh.data_ptr(),
                                               p.bad.data_ptr() + 4, s), "split_f16x2_t")
    return p


# ----------------------------------------------------------------------------------------------------------
# cases

@dataclass(frozen=True)
class GruCase:
    name: str
    layout: str                       # 'plain' (fp32 MFMA), 'x3r' (register-A bf16x3), 'h2r' (fp16x2 + fix-up)
    H: int
    R: int
    segs: Tuple[Tuple[int, Placement], ...]   # (width, placement) of x0 / x1 / x2
    hprev: Placement = P0
    out: Placement = P0
    g4: Placement = P0
    bi: int = 0                       # offsets in floats of the 1-D operands
    bh: int = 0
    sc: int = 0
    lb: int = 0
    kxp_extra: int = 0                # Wi^T planes padded this much deeper than the minimum
    fill: str = "nan"                 # guard rows and gaps of the inputs: 'nan' or 'huge' (1e30)
    h_row0: Optional[float] = None    # hprev[0, :32], the line the register-A kernels read for padding k
    tags: Tuple[str, ...] = ()

    @property
    def widths(self) -> Tuple[int, ...]:
        return tuple(w for w, _ in self.segs)

    @property
    def Kx(self) -> int:
        return sum(self.widths)

    @property
    def kxp(self) -> int:
        return (self.Kx + 31) // 32 * 32 + self.kxp_extra


def kind_segs(kind: str, H: int) -> Tuple[Tuple[int, Placement], ...]:
    """The encoder's two fused-order calls: var8 = [gathered half of a 2H buffer | 8 features], clause4 =
    [gathered 2H | 4 features]."""
    if kind == "var8":
        return ((H, Placement(0, H)), (8, P0))
    assert kind == "clause4"
    return ((2 * H, P0), (4, P0))


def tight_segs(*widths: int) -> Tuple[Tuple[int, Placement], ...]:
    return tuple((w, P0) for w in widths)


def _c(layout, H, R, segs, name, tags, **kw) -> GruCase:
    return GruCase(f"{layout}{H}-R{R}-{name}", layout, H, R, segs, tags=tuple(tags), **kw)


TILE_EDGE_ROWS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
TILE_EDGE_CASES: List[GruCase] = [
    _c(lay, H, R, kind_segs(kind, H), kind, (f"R{R}", kind, f"{lay}{H}"))
    for lay, H in LAYOUTS for kind in ("var8", "clause4") for R in TILE_EDGE_ROWS]
# The fp16x2 kernel's tile edges again with 1e30 in the guards: its range check is built on fmaxf, which drops a
# NaN, so a tile taken for full one row early shows only when the row past R holds a finite out-of-range value
TILE_EDGE_HUGE_CASES = [replace(c, name=c.name + "-huge", fill="huge", tags=c.tags + ("fill-huge",))
                        for c in TILE_EDGE_CASES if c.layout == "h2r"]


def ragged_rows(layout: str) -> int:
    return TILE[layout] + 1  # 65 / 129: one full tile and a one-row tail


def base_case(layout: str, H: int) -> GruCase:
    """Tight and all-aligned: x = [H | 8], every ld the minimum, every offset 0."""
    return _c(layout, H, ragged_rows(layout), tight_segs(H, 8), "base", ("base", "feat-ld8-w8"))


def _placement_cases() -> List[GruCase]:
    out: List[GruCase] = []
    for lay, H in LAYOUTS:
        base = base_case(lay, H)
        out.append(base)
        if H != 128:  # the other widths of the fp32 kernel: the base and one combination below
            continue
        one = [("out", Placement(0, H), "out-ld2H@0"), ("out", Placement(H, H), "out-ld2H@H"),
               ("hprev", Placement(0, H), "hprev-ld2H@0"), ("hprev", Placement(H, H), "hprev-ld2H@H"),
               ("g4", Placement(0, 4), "g4-ld4H+4"), ("g4", Placement(0, 64), "g4-ld4H+64"),
               ("bi", 1, "bi+1"), ("bh", 1, "bh+1"), ("sc", 1, "ln_scale+1"), ("lb", 1, "ln_bias+1")]
        if lay == "plain":  # the header asks for no alignment of out / g4 there
            one += [("out", Placement(1, 0), "out+1"), ("g4", Placement(1, 0), "g4+1"),
                    ("out", Placement(0, 1), "ldo%4"), ("g4", Placement(0, 3), "ldg%4")]
        for f, v, tag in one:
            out.append(replace(base, name=f"{base.name[:-4]}{tag}", tags=(tag,), **{f: v}))
        for segs, tag in [(((H, P0), (4, Placement(0, 4))), "feat-ld8-w4"),
                          (((H, Placement(0, 4)), (8, P0)), "seg0-ld-w+4"),
                          (((H, Placement(0, 60)), (8, P0)), "seg0-ld-w+60"),
                          (((H, P0), (8, Placement(0, 4))), "seg1-ld-w+4"),
                          (((H, P0), (8, Placement(0, 60))), "seg1-ld-w+60")]:
            out.append(replace(base, name=f"{base.name[:-4]}{tag}", tags=(tag,), segs=segs))
    # everything at once
    for lay, H in LAYOUTS:
        R = ragged_rows(lay)
        mis = dict(bi=1, bh=3, sc=2, lb=1)
        if lay == "plain":
            out.append(_c(lay, H, R, ((H // 2, Placement(H, H + 4)), (H // 2, Placement(0, 60)), (4, Placement(4, 4))),
                          "all-mis", ("combination",), hprev=Placement(H, H), out=Placement(1, 1),
                          g4=Placement(3, 3), **mis))
        out.append(_c(lay, H, R, ((H, Placement(H, H)), (4, Placement(0, 4)), (8, Placement(8, 60))), "all",
                      ("combination",), hprev=Placement(H, H + 4), out=Placement(H, H), g4=Placement(4, 64),
                      kxp_extra=32, **mis))
    return out


PLACEMENT_CASES = _placement_cases()


def _segment_cases() -> List[GruCase]:
    out: List[GruCase] = []
    for lay, H in LAYOUTS:
        R = 129
        lays = [((4, H), "4|H", "boundary@4"), ((H // 2, H // 2, 8), "H2|H2|8", "three-segments"),
                ((36, 64, 8), "36|64|8", "boundary-in-32-step-and-16-slab"), ((H, 4), "H|4", "Kx-quad-past-32"),
                ((2 * H,), "2H", "one-segment-2H")]
        for widths, name, tag in lays:
            out.append(_c(lay, H, R, tight_segs(*widths), name, (tag,)))
        out.append(_c(lay, H, R, tight_segs(H, 8), "kxp+32", ("kxp+32",), kxp_extra=32))
    return out


SEGMENT_CASES = _segment_cases()

# (d) padding and tail reads: the base placement and the segment layouts again, both guard fills; the line read
# for padding k (hprev's first row) ordinary and at 200.0 (in range: no flag)
PADDING_CASES: List[GruCase] = (
    [replace(c, name=f"{c.name}-{fill}", fill=fill, tags=c.tags + (f"fill-{fill}",))
     for c in [base_case(lay, H) for lay, H in LAYOUTS] + SEGMENT_CASES for fill in ("nan", "huge")]
    + [replace(c, name=f"{c.name}-row0-{'ordinary' if v is None else 200}-{fill}", h_row0=v, fill=fill,
               tags=("padline-ordinary" if v is None else "padline-200", f"fill-{fill}"))
       for c in SEGMENT_CASES if "boundary-in-32-step-and-16-slab" in c.tags or "kxp+32" in c.tags
       for v in (None, 200.0) for fill in ("nan", "huge")])

# the same line at 300.0, out of fp16x2's range: row 0's own tile is flagged, and only a padding read that is not
# discarded before the range check would flag the second tile as well
PADLINE_OUT_OF_RANGE = 300.0
PADLINE_FLAG_CASES = [replace(c, name=f"{c.name}-row0-300", h_row0=PADLINE_OUT_OF_RANGE)
                      for c in SEGMENT_CASES if c.layout == "h2r" and c.kxp > c.Kx]

# (e) gate limits: bi of one gate set to +-m on a third of the units
GATE_M = (20.0, 89.0, 104.0, 1.0e4)
GATE_CASES = [(lay, H, ragged_rows(lay), gate, m, sign)
              for lay, H in LAYOUTS for gate in (0, 1, 2) for m in GATE_M for sign in (1.0, -1.0)]
CONST_ROWS = (1.0, -0.5, 2.0 ** -20)
NEAR_CONST = (10.0, 100.0)
TANH_CUT = 0.625

FACTORS = {
    "tile edges": [f"R{R}" for R in TILE_EDGE_ROWS] + ["var8", "clause4"] + [f"{lay}{H}" for lay, H in LAYOUTS],
    "placements": ["base", "out-ld2H@0", "out-ld2H@H", "hprev-ld2H@0", "hprev-ld2H@H", "g4-ld4H+4", "g4-ld4H+64",
                   "out+1", "g4+1", "ldo%4", "ldg%4", "bi+1", "bh+1", "ln_scale+1", "ln_bias+1", "feat-ld8-w4",
                   "feat-ld8-w8", "seg0-ld-w+4", "seg0-ld-w+60", "seg1-ld-w+4", "seg1-ld-w+60", "combination"],
    "segments": ["boundary@4", "three-segments", "boundary-in-32-step-and-16-slab", "Kx-quad-past-32",
                 "one-segment-2H", "kxp+32"],
    "padding": ["fill-nan", "fill-huge", "padline-ordinary", "padline-200"],
}
TABLES = {"tile edges": TILE_EDGE_CASES, "placements": PLACEMENT_CASES, "segments": SEGMENT_CASES,
          "padding": PADDING_CASES}


# ----------------------------------------------------------------------------------------------------------
# data and reference (CPU generator: the same numbers with and without a GPU)

def gru_data(H: int, R: int, widths: Tuple[int, ...], h_row0: Optional[float] = None, device="cpu"):
    """x segments, h ~ N(0, 1); weights N(0, 1) / sqrt(fan-in); biases and LayerNorm parameters as the
    standing GRU tests draw them (b_hr = b_hz = 0: flax has none).  The placement is no part of the seed."""
    import torch

    g = torch.Generator().manual_seed(zlib.crc32(repr((H, R, tuple(widths))).encode()))
    rnd = lambda *s: torch.randn(*s, generator=g)
    Kx = sum(widths)
    d = SimpleNamespace(H=H, R=R)
    d.xs = [rnd(R, w) for w in widths]
    d.h = rnd(R, H)
    d.wi = rnd(Kx, 3 * H) / Kx ** 0.5
    d.wh = rnd(H, 3 * H) / H ** 0.5
    d.bi = rnd(3 * H) * 0.1
    d.bh = torch.cat([torch.zeros(2 * H), rnd(H) * 0.1])
    d.sc = 1 + 0.1 * rnd(H)
    d.lb = 0.1 * rnd(H)
    if h_row0 is not None:
        d.h[0, :32] = h_row0
    return to_device(d, device)


def to_device(d, device):
    o = SimpleNamespace(H=d.H, R=d.R, xs=[x.to(device).contiguous() for x in d.xs])
    for k in ("h", "wi", "wh", "bi", "bh", "sc", "lb"):
        setattr(o, k, getattr(d, k).to(device).contiguous())
    return o


def case_data(c: GruCase, device="cpu"):
    return gru_data(c.H, c.R, c.widths, c.h_row0, device)


def reference(d, dtype=None):
    """(out, tape [r_pre | z_pre | gin | ghn], sum|terms| of each tape entry) of the restatement in `dtype`
    (default float64) on d's device.  The weight has Kx rows in the segments' order."""
    import torch

    dtype = torch.float64 if dtype is None else dtype
    t = lambda v: v.to(dtype)
    H = d.H
    x = torch.cat([t(s) for s in d.xs], 1)
    ref, gi, gh = _ref_gru_ln(x, t(d.h), t(d.wi), t(d.bi), t(d.wh), t(d.bh), t(d.sc), t(d.lb), H)
    tape = torch.cat([gi[:, :H] + gh[:, :H], gi[:, H:2 * H] + gh[:, H:2 * H], gi[:, 2 * H:], gh[:, 2 * H:]], 1)
    absx = torch.cat([x.abs() @ t(d.wi).abs() + t(d.bi).abs(), t(d.h).abs() @ t(d.wh).abs() + t(d.bh).abs()], 1)
    ab = torch.cat([absx[:, :H] + absx[:, 3 * H:4 * H], absx[:, H:2 * H] + absx[:, 4 * H:5 * H],
                    absx[:, 2 * H:3 * H], absx[:, 5 * H:]], 1)
    return ref, tape, ab


def out_bar(ref):
    return 1e-5 * ref.abs() + 1e-5


def tape_bar(ab):
    return 2e-6 * ab + 1e-30


# ----------------------------------------------------------------------------------------------------------
# the launch

def _fwd(d, c: GruCase, tape: bool = True):
    """One launch of case c's entry point on the device data d (case_data(c, 'cuda'), possibly modified), every
    operand at c's placement.  Asserts all guards and gaps intact and no NaN in out / g4; returns
    (out, g4 or None, h2r tile flags or None, bad or None)."""
    import torch

    from marlsat import _lib

    H, R = c.H, c.R
    fill = None if c.fill == "nan" else HUGE
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    xs = [operand(x, pl, fill=fill) for x, (_, pl) in zip(d.xs, c.segs)]
    hp = operand(d.h, c.hprev, fill=fill)
    wi, wh = operand(d.wi, fill=fill), operand(d.wh, fill=fill)
    bi, bh = vector(d.bi, c.bi, fill=fill), vector(d.bh, c.bh, fill=fill)
    sc, lb = vector(d.sc, c.sc, fill=fill), vector(d.lb, c.lb, fill=fill)
    out = operand(nan(R, H), c.out, "out")
    g4 = operand(nan(R, 4 * H), c.g4, "out") if tape else None
    args = []
    for i in range(3):
        args += [xs[i].ptr, xs[i].ld, c.segs[i][0]] if i < len(xs) else [0, 0, 0]
    tail = [out.ptr, out.ld, g4.ptr if tape else 0, g4.ld if tape else 4 * H, R, H]
    s = _lib.stream_ptr()
    flags = bad = None
    if c.layout == "plain":
        rc = _lib.lib.msat_gru_ln_fused_fwd(*args, hp.ptr, hp.ld, wi.ptr, bi.ptr, wh.ptr, bh.ptr, sc.ptr, lb.ptr,
                                            *tail, s)
    else:
        p = build_planes(wi.view, wh.view, H, c.layout, c.kxp)
        if c.layout == "x3r":
            rc = _lib.lib.msat_gru_ln_fused_fwd_x3r(*args, hp.ptr, hp.ld, p.pi.data_ptr(), p.kxp, bi.ptr,
                                                    p.ph.data_ptr(), bh.ptr, sc.ptr, lb.ptr, *tail, s)
        else:
            tiles = (R + 127) // 128
            fl = torch.full((tiles + 1,), 7, dtype=torch.int32, device="cuda")
            rc = _lib.lib.msat_gru_ln_fused_fwd_h2r(*args, hp.ptr, hp.ld, p.qi.data_ptr(), p.qh.data_ptr(),
                                                    p.pi.data_ptr(), p.ph.data_ptr(), p.kxp, bi.ptr, bh.ptr, sc.ptr,
                                                    lb.ptr, *tail, fl.data_ptr(), p.bad.data_ptr(), s)
    _lib.check(rc, f"gru_ln_fused_fwd ({c.layout})")
    torch.cuda.synchronize()
    for o in xs + [hp, wi, wh, bi, bh, sc, lb, out] + ([g4] if tape else []):
        o.check()
    if c.layout == "h2r":
        assert int(fl[tiles]) == 7, "wrote past the tile flags"
        flags, bad = fl[:tiles].cpu(), p.bad.cpu()
    assert not bool(torch.isnan(out.view).any()), "NaN in out"
    assert not tape or not bool(torch.isnan(g4.view).any()), "NaN in g4"
    return out.view.clone(), g4.view.clone() if tape else None, flags, bad


# ----------------------------------------------------------------------------------------------------------
# (e) gate limits: inputs that steer the gates through bi (x, h ~ N(0, 1), weights as gru_data draws them)

GATE_WIDTHS = lambda H: (H, 8)


def gate_limit_data(H, R, gate, m, sign, device="cpu"):
    """bi of gate `gate` (0 r, 1 z, 2 n) = sign * m on every third unit."""
    import torch

    d = gru_data(H, R, GATE_WIDTHS(H))
    d.bi[gate * H + torch.arange(0, H, 3)] = sign * m
    return to_device(d, device)


def zero_data(H, R, device="cpu"):
    """x = 0, h = 0, bi = bh = 0: every hn is 0, the LayerNorm sees variance 0 and out is ln_bias."""
    d = gru_data(H, R, GATE_WIDTHS(H))
    for t in d.xs + [d.h, d.bi, d.bh]:
        t.zero_()
    return to_device(d, device)


def z_saturated_data(H, R, h_const=None, near=None, device="cpu"):
    """z_pre = 1e4 + O(1) on every unit: z = 1, hn = h, out = LN(h).  h_const: h = c everywhere (variance 0);
    near: h = c + 1e-3 N(0, 1)."""
    import torch

    d = gru_data(H, R, GATE_WIDTHS(H))
    d.bi[H:2 * H] = 1.0e4
    if h_const is not None:
        d.h.fill_(h_const)
    if near is not None:
        g = torch.Generator().manual_seed(int(near) + H)
        d.h = near + 1e-3 * torch.randn(R, H, generator=g)
    return to_device(d, device)


def tanh_cut_grid(H):
    """n-gate pre-activations per unit: +-0.625 and 1..3 ulp either side of each (an ulp there is 2^-24), the
    rest spread over (-1.5, 1.5)."""
    import torch

    near = [s * (TANH_CUT + k * 2.0 ** -24) for s in (1.0, -1.0) for k in range(-3, 4)]
    return torch.cat([torch.tensor(near, dtype=torch.float64),
                      torch.linspace(-1.5, 1.5, H - len(near), dtype=torch.float64)]).float()


def tanh_cut_data(H, R, device="cpu"):
    """hn = tanh(bi_n) exactly: zero weights into the n gate, r = 0 (bias -1e4) so r * ghn vanishes, z = 0
    (bias -1e4); LayerNorm scale 1, bias 0."""
    d = gru_data(H, R, GATE_WIDTHS(H))
    d.wi[:, 2 * H:] = 0
    d.bi[:2 * H] = -1.0e4
    d.bi[2 * H:] = tanh_cut_grid(H)
    d.sc.fill_(1.0)
    d.lb.zero_()
    return to_device(d, device)
