"""GPU: the fused GRU + LayerNorm forward -- the fp32 MFMA kernel (H 64 / 128 / 256), the register-A bf16x3
kernel and the fp16x2 kernel with its bf16x3 fix-up launch (H 128) -- against the float64 restatement at tile
edges, at every operand placement the header admits, at segment layouts whose boundaries fall inside a kernel's
k step, with NaN or 1e30 wherever a kernel may read but must not use, and at the limits of the gate functions.

Bars (tests/test_gru_fused_gpu.py's): out within 1e-5 |ref| + 1e-5; tape within 2e-6 sum|terms|; out with and
without the tape bitwise equal; a second identical launch bitwise equal.  Every launch also asserts guard rows
and ld gaps of every operand bit-identical afterwards and no NaN in out / g4 (gru_placement._fwd).  Inputs and
case tables: tests/gru_placement.py; tests/test_gru_fused_placement_cpu.py shows that the float32 restatement
meets the same bars on the same inputs."""
import pytest
import torch

import gru_placement as gr
from gru_placement import _fwd, case_data, reference

pytestmark = pytest.mark.gpu

_bits = lambda t: t.view(torch.int32)


def _close(out, ref, what="out"):
    err = (out.double() - ref).abs()
    bar = gr.out_bar(ref)
    assert bool((err <= bar).all()), (what, float((err / bar).max()))


def _tape_close(g4, tape, ab, cols=None):
    err, bar = (g4.double() - tape).abs(), gr.tape_bar(ab)
    if cols is not None:
        err, bar = err[:, cols], bar[:, cols]
    assert bool((err <= bar).all()), ("tape", float((err / bar).max()))


def _run(c, d, tape_cols=slice(None), check_out=True):
    """The standing checks of one case on device data d: two launches with the tape (bitwise equal), one
    without (out bitwise equal), out and tape against float64.  Returns (out, g4, flags, bad, ref)."""
    out, g4, flags, bad = _fwd(d, c)
    out2, g42, flags2, bad2 = _fwd(d, c)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(g4), _bits(g42)), "second launch differs"
    out_nt, _, _, _ = _fwd(d, c, tape=False)
    assert torch.equal(_bits(out), _bits(out_nt)), "out differs without the tape"
    ref, tape, ab = reference(d)
    if check_out:
        _close(out, ref)
    assert bool(torch.isfinite(g4).all()) and bool(torch.isfinite(out).all())
    if tape_cols is not None:
        _tape_close(g4, tape, ab, tape_cols)
    return out, g4, flags, bad, ref


def _no_flags(c, flags, bad):
    if c.layout == "h2r":
        assert flags.tolist() == [0] * ((c.R + 127) // 128) and bad.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------- a. tile edges

@pytest.mark.parametrize("c", gr.TILE_EDGE_CASES + gr.TILE_EDGE_HUGE_CASES, ids=lambda c: c.name)
def test_tile_edges(c):
    _, _, flags, bad, _ = _run(c, case_data(c, "cuda"))
    _no_flags(c, flags, bad)


@pytest.mark.parametrize("c", [c for c in gr.TILE_EDGE_CASES if c.layout == "h2r"], ids=lambda c: c.name)
def test_h2r_flags_exactly_the_last_partial_tile(c):
    """One activation of 300 (>= 256: outside fp16x2's range after the 2^7 pre-scale) in the last row: that
    tile's flag alone is set and its rows are bitwise the bf16x3 kernel's."""
    d = case_data(c, "cuda")
    d.xs[0][c.R - 1, 5] = -300.0
    out, g4, flags, bad, _ = _run(c, d)
    tiles = (c.R + 127) // 128
    assert bad.tolist() == [0, 0] and flags.tolist() == [0] * (tiles - 1) + [1]
    ox, gx, _, _ = _fwd(d, gr.replace(c, layout="x3r"))
    rows = slice(128 * (tiles - 1), c.R)
    assert torch.equal(_bits(out[rows]), _bits(ox[rows])) and torch.equal(_bits(g4[rows]), _bits(gx[rows]))


# ------------------------------------------------------------- b. placements, c. segment layouts, d. padding

@pytest.mark.parametrize("c", gr.PLACEMENT_CASES + gr.SEGMENT_CASES + gr.PADDING_CASES, ids=lambda c: c.name)
def test_placements_segments_and_padding(c):
    _, _, flags, bad, _ = _run(c, case_data(c, "cuda"))
    _no_flags(c, flags, bad)  # also with 1e30 in every guard and gap, and with 200.0 in the padding line


@pytest.mark.parametrize("c", gr.PADLINE_FLAG_CASES, ids=lambda c: c.name)
def test_h2r_padding_line_cannot_flag_another_tile(c):
    """hprev[0, :32] = 300, outside fp16x2's range: tile 0, which holds row 0, takes the bf16x3 path; tile 1 reads
    that line only for its padding k and must discard it before the range check."""
    _, _, flags, bad, _ = _run(c, case_data(c, "cuda"))
    assert flags.tolist() == [1, 0] and bad.tolist() == [0, 0]


def test_placement_does_not_change_the_result():
    """Nothing but the operands' addresses differs between the cases of one kernel that share their data: out and
    tape are bitwise the base case's."""
    for lay, H in gr.LAYOUTS:
        base = gr.base_case(lay, H)
        d = case_data(base, "cuda")
        out0, g0, _, _ = _fwd(d, base)
        for c in gr.PLACEMENT_CASES:
            if (c.layout, c.H, c.widths, c.kxp_extra) == (lay, H, base.widths, 0) and c is not base:
                out, g4, _, _ = _fwd(d, c)
                assert torch.equal(_bits(out), _bits(out0)) and torch.equal(_bits(g4), _bits(g0)), c.name


# ------------------------------------------------------------------------------------------- e. gate limits

def _gate_case(lay, H):
    return gr.replace(gr.base_case(lay, H), name=f"{lay}{H}-gates")


@pytest.mark.parametrize("lay,H,R,gate,m,sign", gr.GATE_CASES,
                         ids=lambda v: str(v) if not isinstance(v, float) else f"{v:g}")
def test_gate_limits(lay, H, R, gate, m, sign):
    """bi of one gate at +-m on a third of the units: past exp's overflow (88.7) and exp2's 128 the sigmoid and
    tanh forms must saturate, not produce Inf - Inf or 0 * Inf.  The tape bar holds as well (sum|terms|
    contains m)."""
    _run(_gate_case(lay, H), gr.gate_limit_data(H, R, gate, m, sign, "cuda"))


@pytest.mark.parametrize("lay,H", gr.LAYOUTS)
def test_all_zero_activations_give_ln_bias(lay, H):
    c = _gate_case(lay, H)
    d = gr.zero_data(H, c.R, "cuda")
    out, g4, flags, bad, _ = _run(c, d)
    assert torch.equal(_bits(out), _bits(d.lb.expand(c.R, H).contiguous()))  # variance 0: (0 - 0) * rs * scale + bias
    assert not bool(g4.any())
    _no_flags(c, flags, bad)


@pytest.mark.parametrize("lay,H", gr.LAYOUTS)
def test_z_saturated_is_the_layer_norm_of_hprev(lay, H):
    c = _gate_case(lay, H)
    d = gr.z_saturated_data(H, c.R, device="cuda")
    out, g4, _, _, _ = _run(c, d, tape_cols=slice(H, 2 * H))
    h = d.h.double()
    mean = h.mean(-1, keepdim=True)
    var = (h * h).mean(-1, keepdim=True) - mean * mean
    _close(out, (h - mean) * torch.rsqrt(var + 1e-6) * d.sc.double() + d.lb.double(), "LN(hprev)")


@pytest.mark.parametrize("const", gr.CONST_ROWS)
@pytest.mark.parametrize("lay,H", gr.LAYOUTS)
def test_constant_rows_give_ln_bias(lay, H, const):
    """z = 1 and h = c, a power of two: every partial sum of E[x] and E[x^2] is exact in any order, the variance
    is exactly 0 (the clamp's case) and out is ln_bias bitwise."""
    c = _gate_case(lay, H)
    d = gr.z_saturated_data(H, c.R, h_const=const, device="cuda")
    out, _, _, _, _ = _run(c, d, tape_cols=slice(H, 2 * H))
    assert torch.equal(_bits(out), _bits(d.lb.expand(c.R, H).contiguous()))


@pytest.mark.parametrize("lay,H", gr.LAYOUTS)
def test_tanh_through_its_branch_cut(lay, H):
    """hn = tanh(bi_n) with bi_n on a grid through +-0.625 +- 3 ulp (ftanh_fast switches from its polynomial to
    2 sigmoid(2x) - 1 there): parity at the out bar and no step across the cut beyond it."""
    c = _gate_case(lay, H)
    d = gr.tanh_cut_data(H, c.R, "cuda")
    out, g4, _, _, ref = _run(c, d, tape_cols=slice(2 * H, 3 * H))
    assert torch.equal(_bits(g4[:, 2 * H:3 * H]), _bits(d.bi[2 * H:].expand(c.R, H).contiguous()))  # gin == bi_n
    err = out.double() - ref
    for s0 in (0, 7):  # units s0 .. s0 + 6: the cut (+ / -) at -3 .. +3 ulp, the cut itself in the middle
        below, above = err[:, s0:s0 + 3], err[:, s0 + 3:s0 + 7]
        step = (above.unsqueeze(2) - below.unsqueeze(1)).abs().amax()
        assert float(step) <= float(gr.out_bar(ref[:, s0:s0 + 7]).min()), float(step)


@pytest.mark.parametrize("near", gr.NEAR_CONST)
@pytest.mark.parametrize("lay,H", gr.LAYOUTS)
def test_near_constant_rows_against_float32s_own_error(lay, H, near):
    """h = c + 1e-3 N(0, 1), z = 1: fp32's E[x^2] - mean^2 cancels (mean^2 = 1e2 / 1e4 against a variance of 1e-6),
    so the bar is the float32 restatement's own error E32 = max |ref32 - ref64| on the CPU:
    |dev - ref64| <= 1e-5 |ref64| + 1e-5 + 4 E32 (4: the project's GRAD_FACTOR).  E32 is 1.6 .. 2.0 at c = 10 and
    2.4 .. 2.8 at c = 100 for outputs of O(1): float32's variance is noise there, so what this case pins is that the
    clamp keeps the result finite and of the restatement's scale.
    Measured on an MI355X, max |dev - ref64| / E32 at c = 10 / c = 100: fp32 kernel H 64 0.75 / 0.89, H 128
    0.83 / 1.17, H 256 1.21 / 1.00; bf16x3 1.00 / 1.00; fp16x2 1.00 / 1.00 (printed per kernel)."""
    c = _gate_case(lay, H)
    d = gr.z_saturated_data(H, c.R, near=near, device="cuda")
    out, _, _, _, ref = _run(c, d, tape_cols=slice(H, 2 * H), check_out=False)
    dc = gr.z_saturated_data(H, c.R, near=near)
    ref64, _, _ = reference(dc)
    ref32, _, _ = reference(dc, torch.float32)
    e32 = float((ref32.double() - ref64).abs().max())
    err = (out.double().cpu() - ref64).abs()
    print(f"near-constant rows c={near:g} {lay}{H}: max|dev - ref64| = {float(err.max()):.3g}, E32 = {e32:.3g}, "
          f"ratio {float(err.max()) / e32:.3g}")
    assert bool((err <= gr.out_bar(ref64) + 4.0 * e32).all()), float(err.max())
