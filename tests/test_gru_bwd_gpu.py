"""GPU: gru_ln_bwd_kernel in every form its tape entry points reach (msat_gru_ln_bwd_g4 / _g4f / _g4fe), against
float64 autograd of the same cell.

The reference takes a random tape g4 = [r_pre | z_pre | gin | ghn] as a leaf (no forward kernel involved):
    r = s(r_pre), z = s(z_pre), n = tanh(gin + r ghn), h' = (1 - z) n + z h,
    y = (h' - mean) rsqrt(E[h'^2] - mean^2 + 1e-6) scale + bias,   loss = sum(y dy)
so g4.grad = [dar | daz | dan | dan r]: the packed row is [dan | dar | daz | dan r], dGi = [dar | daz | dan],
dGh = [dar | daz | dan r], dbi = sum dGi, dbh_n = sum dan r, dfeat = feat[:, :nfeat]^T dGi.

Covered: the three entry points, H 64 / 128 / 256 (PER 1 / 2 / 4), nfeat 0 / 2 / 6 with ldf 4, 7, 8, 6, the form
without gate-bias outputs (NQ = 2), packed and unpacked rows, the fp16x2 plane store, the vector body and the scalar
body at nfeat 6 (dy one float into a buffer of ld H + 1), all four combinations of flags bits 0 / 1, every leading
dimension wider than needed with canaries in the gaps, and R = 0, 1, 3, 4, 5, 77, 4097 (a wave's first second row:
the grid caps at 1024 blocks of 4 waves) and 8195 (third trip and a ragged tail).

Value rows (R >= 77): rows 8..15 hold saturated gates (r_pre, z_pre at +-40 and +-100, gin at +-20); row 21 has
z_pre = +100 and a constant h, so h' is constant, var clamps to 0 and rs = 1000; every ninth row of dy is zero (its
packed row must be all zero and rexp == 0x3FFF); dy rows are spread over 1e-8 .. 1e1.  No row has |mean h'| far above
its spread (E[x^2] - mean^2 cancels there in any fp32 evaluation of the formula).

Bars, per tensor: normwise max|err| <= 1e-4 max|ref| + 1e-6, and elementwise |err| <= 1e-5 |ref| + FACTOR x E32, where
E32 is the largest error over that tensor of the SAME formula evaluated in float32 on the CPU with torch against the
float64 reference (never the kernel's output).  rexp is exactly row_exp of the fp32 packed row of the same launch; a
plane launch is bitwise the host split of the rows of the launch without bit 3, every other output bitwise equal.
"""
import functools

import pytest
import torch

from test_planes_gpu import KZERO, host_planes, row_exp

pytestmark = pytest.mark.gpu

# Elementwise bar: |err| <= 1e-5 |ref| + FACTOR[tensor] x E32 (GRAD_FACTOR of tests/test_gnn_gpu.py).
# Printed on MI355X, worst over all cases of this file and of test_unfused_backward_matches_float64
# (tests/test_gnn_exports_gpu.py), per tensor -- max |err| / E32, then max (|err| - 1e-5 |ref|) / E32, the figure
# the factor bounds:
#   packed 1.65 / 0.10   dGi 1.85 / 0.22   dGh 1.72 / 0.20   dh 1.54 / 0.08
#   dln    2.37 / 1.09   dbi 1.39 / 0.50   dbh_n 1.51 / 0.72   dfeat 1.38 / 0.22
# (dln 2.37: g4fe H 128 R 8195 nfeat 6 strided; its sums run over the 1024 block partials in a fixed order, the
# yardstick's over torch's pairwise order).  Nothing is above 4, so no tensor has a factor of its own.
GRAD_FACTOR = 4.0
FACTOR = {}  # per-tensor overrides (measured ratio x 1.5): none

CANARY = 777.25
SAT_ROWS = slice(8, 16)
CONST_ROW = 21


def _inputs(R, H, ldf, seed):
    """CPU float32 inputs of one case: tape, h, dy, LN scale / bias, features (R, ldf)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    g4, h, dy = rnd(R, 4 * H), rnd(R, H), rnd(R, H)
    sc, lb = 1 + 0.3 * rnd(H), 0.1 * rnd(H)
    feat = rnd(R, max(ldf, 1))
    dy *= torch.pow(10.0, torch.empty(R, 1).uniform_(-8, 1, generator=g))
    dy[2::9] = 0
    if R > CONST_ROW:
        j = torch.arange(H)
        sat = torch.tensor([40.0, -40.0, 100.0, -100.0])
        half = j < H // 2  # the other half of the columns stays unsaturated: h' keeps its spread
        blk = g4[SAT_ROWS]
        blk[:, :H][:, half] = sat[j[half] % 4]
        blk[:, H:2 * H][:, half] = sat[(j[half] // 4) % 4]
        third = j % 3 == 0
        blk[:, 2 * H:3 * H][:, third] = torch.where(j[third] % 2 == 0, 20.0, -20.0)
        g4[CONST_ROW, H:2 * H] = 100.0
        h[CONST_ROW] = 0.75
        dy[SAT_ROWS] = rnd(8, H)  # O(1) cotangents on the saturated rows (row 11 zero, below)
        dy[11] = 0
        dy[CONST_ROW] = rnd(H)
    return g4, h, dy, sc, lb, feat


def _formula(inp, H, nfeat, dtype):
    """The cell and its gradients in `dtype` on the CPU (float64: the reference; float32: the yardstick)."""
    g4, h, dy, sc, lb, feat = (t.to(dtype) for t in inp)
    g4, h, sc, lb = (t.clone().requires_grad_(True) for t in (g4, h, sc, lb))
    r = torch.sigmoid(g4[:, :H])
    z = torch.sigmoid(g4[:, H:2 * H])
    n = torch.tanh(g4[:, 2 * H:3 * H] + r * g4[:, 3 * H:])
    hn = (1 - z) * n + z * h
    mean = hn.mean(-1, keepdim=True)
    var = (hn * hn).mean(-1, keepdim=True) - mean * mean
    y = (hn - mean) * torch.rsqrt(var + 1e-6) * sc + lb
    (y * dy).sum().backward()
    dar, daz, dan, danr = g4.grad.split(H, dim=1)
    dGi = torch.cat([dar, daz, dan], 1)
    return {"packed": torch.cat([dan, dar, daz, danr], 1), "dGi": dGi, "dGh": torch.cat([dar, daz, danr], 1),
            "dh": h.grad, "dln": torch.cat([sc.grad, lb.grad]), "dbi": dGi.sum(0), "dbh_n": danr.sum(0),
            "dfeat": feat[:, :nfeat].t() @ dGi}


@functools.lru_cache(maxsize=None)
def _case(R, H, nfeat, ldf, seed):
    """Inputs, float64 reference and float32 yardstick of one case (computed once, shared, never modified)."""
    inp = _inputs(R, H, ldf, seed)
    return inp, _formula(inp, H, nfeat, torch.float64), _formula(inp, H, nfeat, torch.float32)


def _seeds(H, nfeat, R, seed):
    """Starting values of the accumulating outputs (CPU float32)."""
    g = torch.Generator().manual_seed(seed + 99991)
    return {"dh": torch.randn(R, H, generator=g), "dln": torch.randn(2 * H, generator=g),
            "dbi": torch.randn(3 * H, generator=g), "dbh": torch.randn(3 * H, generator=g),
            "dfeat": torch.randn(max(nfeat, 1), 3 * H, generator=g)}


def _padded(t, ld, dev="cuda", fill=CANARY, off=0):
    """Device buffer of (rows + 1) x ld floats (+ off leading floats) filled with `fill`, t copied into the first
    columns of its first rows; returns (buffer, pointer of element [0, 0])."""
    rows, w = t.shape
    buf = torch.full(((rows + 1) * ld + off,), fill, device=dev)
    view = buf[off:].view(rows + 1, ld)
    view[:rows, :w] = t.to(dev)
    return buf, buf.data_ptr() + 4 * off


def _launch(entry, H, R, nfeat, ldf, flags, layout, bias, inp, seeds):
    """One launch; returns the outputs on the CPU.  layout: 'dense', 'strided' (every ld wider than needed) or
    'misaligned' (dy one float into a buffer of ld H + 1: the vector body's alignment test fails)."""
    from marlsat import _lib

    L = _lib.lib
    g4, h, dy, sc, lb, feat = inp
    packed, assign = bool(flags & 4), bool(flags & 2)
    pad = layout == "strided"
    ldy, dyoff = (H + 1, 1) if layout == "misaligned" else (H + 4 * pad, 0)
    ldg, ldp, lddp = 4 * H + 8 * pad, H + 4 * pad, H + 4 * pad
    dyb, dyp = _padded(dy, ldy, off=dyoff)
    g4b, g4p = _padded(g4, ldg)
    hb, hp = _padded(h, ldp)
    scd = sc.cuda()
    nan = float("nan")
    if packed:
        lddi = lddh = 4 * H + 4 * pad
        Db = torch.full(((R + 1) * lddi,), CANARY, device="cuda")
        Db.view(R + 1, lddi)[:R, :4 * H] = nan
        Dhb, dGi_p, dGh_p = Db, Db.data_ptr(), Db.data_ptr() + 4 * H
    else:
        lddi, lddh = 3 * H + 4 * pad, 3 * H + 8 * pad
        Db = torch.full(((R + 1) * lddi,), CANARY, device="cuda")
        Db.view(R + 1, lddi)[:R, :3 * H] = nan
        Dhb = torch.full(((R + 1) * lddh,), CANARY, device="cuda")
        Dhb.view(R + 1, lddh)[:R, :3 * H] = nan
        dGi_p, dGh_p = Db.data_ptr(), Dhb.data_ptr()
    dh0 = torch.full((R, H), nan) if assign else seeds["dh"]
    dhb, dhp = _padded(dh0, lddp)
    dln = torch.full((2 * H,), nan, device="cuda") if not flags & 1 else seeds["dln"].cuda()
    dbi, dbh, dfeat = seeds["dbi"].cuda(), seeds["dbh"].cuda(), seeds["dfeat"].cuda()
    featb, featp = _padded(feat, max(ldf, 1), fill=nan)  # columns past nfeat are NaN: never read
    if nfeat:
        featb.view(R + 1, ldf)[:R, nfeat:] = nan
    nfl = int(L.msat_gru_ln_bwd_partial_floats(R, H))
    part = torch.full((nfl + 64,), CANARY, device="cuda")
    rexp = torch.full((R + 4,), -12345, dtype=torch.int32, device="cuda")
    a = [dyp, ldy, g4p, ldg, hp, ldp, scd.data_ptr(), dGi_p, lddi, dGh_p, lddh, dhp, lddp, dln.data_ptr(),
         dln.data_ptr() + 4 * H, dbi.data_ptr() if bias else None, dbh.data_ptr() + 8 * H if bias else None]
    fa = [featp if nfeat else None, ldf, nfeat, dfeat.data_ptr() if nfeat else None]
    tail = [part.data_ptr(), R, H, flags]
    s = _lib.stream_ptr()
    if entry == "g4":
        assert nfeat == 0
        rc = L.msat_gru_ln_bwd_g4(*a, *tail, s)
    elif entry == "g4f":
        rc = L.msat_gru_ln_bwd_g4f(*a, *fa, *tail, s)
    else:
        rc = L.msat_gru_ln_bwd_g4fe(*a, *fa, *tail, rexp.data_ptr(), s)
    _lib.check(rc, f"gru_ln_bwd_{entry}")
    torch.cuda.synchronize()  # every device tensor above is still referenced here
    out = {"D": Db.view(R + 1, lddi).cpu(), "Dh": Dhb.view(R + 1, lddh).cpu(), "dh": dhb.view(R + 1, lddp).cpu(),
           "dln": dln.cpu(), "dbi": dbi.cpu(), "dbh": dbh.cpu(), "dfeat": dfeat.cpu(), "part_tail": part[nfl:].cpu(),
           "rexp": rexp.cpu(), "wD": 4 * H if packed else 3 * H}
    # inputs unchanged (the kernel only reads them)
    assert torch.equal(dyb[dyoff:].view(R + 1, ldy)[:R, :H].cpu(), dy) and torch.equal(hb.view(R + 1, ldp)[:R, :H].cpu(), h)
    return out


def _canaries(out, R, H, packed, bias, nfeat, seeds, has_rexp):
    """Gap columns, the row past the last, b_hr / b_hz, the partials' tail and unrequested outputs: untouched."""
    w = out["wD"]
    assert bool((out["D"][:, w:] == CANARY).all()) and bool((out["D"][R] == CANARY).all()), "dGi gap"
    if not packed:
        assert bool((out["Dh"][:, 3 * H:] == CANARY).all()) and bool((out["Dh"][R] == CANARY).all()), "dGh gap"
    assert bool((out["dh"][:, H:] == CANARY).all()) and bool((out["dh"][R] == CANARY).all()), "dhprev gap"
    assert bool((out["part_tail"] == CANARY).all()), "partials past msat_gru_ln_bwd_partial_floats"
    assert torch.equal(out["dbh"][:2 * H], seeds["dbh"][:2 * H]), "dbh[:2H] (b_hr / b_hz do not exist)"
    if not bias:
        assert torch.equal(out["dbi"], seeds["dbi"]) and torch.equal(out["dbh"], seeds["dbh"])
    if not nfeat:
        assert torch.equal(out["dfeat"], seeds["dfeat"])
    assert bool((out["rexp"][R if has_rexp else 0:] == -12345).all()), "rexp past R"


def _compare(what, got, ref, yard, report):
    """Both bars on one tensor; appends (tensor, max err / E32, worst (err - 1e-5 |ref|) / E32) to report."""
    got, yard = got.double(), yard.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    if ref.numel() == 0:
        return
    err = (got - ref).abs()
    scale = float(ref.abs().max())
    assert float(err.max()) <= 1e-4 * scale + 1e-6, (what, float(err.max()), scale)
    e32 = float((yard - ref).abs().max())
    if scale > 0:
        assert e32 > 0, f"{what}: the float32 yardstick is exact here, choose another seed"
    f = FACTOR.get(what, GRAD_FACTOR)
    excess = float((err - 1e-5 * ref.abs()).max())
    report.append((what, float(err.max()) / max(e32, 1e-300), excess / max(e32, 1e-300)))
    bad = err > 1e-5 * ref.abs() + f * e32
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements over 1e-5 |ref| + {f} x E32 ({e32:.3g}); "
                                 f"max err {float(err.max()):.3g}, worst excess / E32 {excess / max(e32, 1e-300):.3g}")


def _check_values(out, ref, yard, seeds, R, H, nfeat, flags, bias, report):
    packed, assign = bool(flags & 4), bool(flags & 2)
    d = lambda t: t.double()
    if packed:
        _compare("packed", out["D"][:R, :4 * H], ref["packed"], yard["packed"], report)
    else:
        _compare("dGi", out["D"][:R, :3 * H], ref["dGi"], yard["dGi"], report)
        _compare("dGh", out["Dh"][:R, :3 * H], ref["dGh"], yard["dGh"], report)
    # accumulating outputs: reference + seed in float64, yardstick the float32 sum
    if assign:
        _compare("dh", out["dh"][:R, :H], ref["dh"], yard["dh"], report)
    else:
        _compare("dh", out["dh"][:R, :H], ref["dh"] + d(seeds["dh"]), seeds["dh"] + yard["dh"], report)
    if flags & 1:
        _compare("dln", out["dln"], ref["dln"] + d(seeds["dln"]), seeds["dln"] + yard["dln"], report)
    else:
        _compare("dln", out["dln"], ref["dln"], yard["dln"], report)  # assigned over NaN: none survives
    if bias:
        _compare("dbi", out["dbi"], ref["dbi"] + d(seeds["dbi"]), seeds["dbi"] + yard["dbi"], report)
        _compare("dbh_n", out["dbh"][2 * H:], ref["dbh_n"] + d(seeds["dbh"][2 * H:]),
                 seeds["dbh"][2 * H:] + yard["dbh_n"], report)
    if nfeat:
        _compare("dfeat", out["dfeat"], ref["dfeat"] + d(seeds["dfeat"]), seeds["dfeat"] + yard["dfeat"], report)


def _check_value_rows(out, inp, R, H, packed):
    """Saturated gates: exact zeros where the fp32 derivative vanishes; zero-dy rows: all-zero gate gradients."""
    g4 = inp[0]
    if packed:
        dan, dar, daz, danr = out["D"][:R, :4 * H].split(H, dim=1)
    else:
        dar, daz, dan = out["D"][:R, :3 * H].split(H, dim=1)
        danr = out["Dh"][:R, 2 * H:3 * H]
    zero_rows = torch.zeros(R, dtype=torch.bool)
    zero_rows[2::9] = True
    if R > CONST_ROW:
        zero_rows[11] = True
        zero_rows[CONST_ROW] = True  # h' constant: z = 1, every gate gradient is exactly 0 (dh is not)
        rp, zp, gin = g4[SAT_ROWS, :H], g4[SAT_ROWS, H:2 * H], g4[SAT_ROWS, 2 * H:3 * H]
        # s'(x) is 0 in fp32 for x = +40 (1 + e^-40 rounds to 1) and +-100; 1 - tanh^2 is 0 at +-20 and then
        # dan = 0 takes dar and dan r with it; z = 1 zeroes dan as well
        sat = lambda x: (x == 40) | (x.abs() == 100)
        n0 = (gin.abs() == 20) | (zp == 40) | (zp == 100)
        assert bool((dar[SAT_ROWS][sat(rp) | n0] == 0).all()), "dar at saturated r / n"
        assert bool((daz[SAT_ROWS][sat(zp)] == 0).all()), "daz at saturated z"
        assert bool((dan[SAT_ROWS][n0] == 0).all()) and bool((danr[SAT_ROWS][n0] == 0).all()), "dan at saturated n / z"
        assert bool((out["dh"][CONST_ROW, :H].abs() > 0).any())
    for t in (dar, daz, dan, danr):
        assert bool((t[zero_rows] == 0).all()), "zero-dy rows"
    return zero_rows


# entry, H, R, nfeat, ldf, flags, layout, bias
CASES = [
    # feature-less entry point, with and without the gate-bias outputs (NQ 6 / 2), unpacked and packed
    ("g4", 64, 77, 0, 0, 1, "dense", True),
    ("g4", 128, 5, 0, 0, 2, "strided", True),
    ("g4", 256, 4097, 0, 0, 3, "dense", True),
    ("g4", 128, 77, 0, 0, 0, "dense", False),
    ("g4", 64, 8195, 0, 0, 4 | 2, "strided", False),
    ("g4", 256, 77, 0, 0, 4 | 1, "dense", False),
    ("g4", 64, 0, 0, 0, 1, "dense", True),
    # g4f: unpacked rows with features, every nfeat / ldf pair
    ("g4f", 64, 4, 2, 4, 0, "dense", True),
    ("g4f", 256, 77, 2, 7, 3, "strided", True),
    ("g4f", 128, 1, 6, 8, 1, "dense", True),
    ("g4f", 64, 3, 6, 6, 2, "strided", True),
    ("g4f", 128, 4097, 6, 6, 0, "dense", True),
    ("g4f", 128, 0, 2, 4, 3, "dense", True),
    # g4fe, packed rows + rexp: the clause cell (nfeat 2, ldf 4) at every row count, every flags 0..3
    ("g4fe", 128, 0, 2, 4, 7, "dense", True),
    ("g4fe", 128, 1, 2, 4, 4, "dense", True),
    ("g4fe", 128, 3, 2, 4, 5, "strided", True),
    ("g4fe", 128, 4, 2, 4, 6, "dense", True),
    ("g4fe", 128, 5, 2, 4, 7, "strided", True),
    ("g4fe", 128, 77, 2, 4, 4, "strided", True),
    ("g4fe", 128, 4097, 2, 4, 7, "dense", True),
    ("g4fe", 128, 8195, 2, 4, 5, "dense", True),
    ("g4fe", 64, 77, 2, 7, 6, "dense", True),
    ("g4fe", 256, 5, 2, 4, 7, "dense", True),
    ("g4fe", 64, 5, 0, 0, 7, "dense", True),  # rexp without features
    # the var cell (nfeat 6): vector body (aligned) and scalar body (misaligned) at H 128 / 256
    ("g4fe", 128, 77, 6, 8, 7, "dense", True),
    ("g4fe", 128, 77, 6, 8, 7, "misaligned", True),
    ("g4fe", 256, 77, 6, 8, 5, "dense", True),
    ("g4fe", 256, 77, 6, 8, 6, "misaligned", True),
    ("g4fe", 128, 8195, 6, 8, 7, "strided", True),
    ("g4fe", 256, 4097, 6, 6, 4, "strided", True),
    ("g4fe", 128, 4097, 6, 8, 5, "misaligned", True),
    ("g4fe", 64, 8195, 6, 6, 7, "dense", True),
    # fp16x2 planes (bit 3): compared with the launch without bit 3
    ("g4fe", 128, 77, 6, 8, 15, "dense", True),
    ("g4fe", 128, 77, 6, 8, 15, "misaligned", True),
    ("g4fe", 256, 77, 6, 8, 13, "dense", True),
    ("g4fe", 256, 77, 6, 8, 14, "misaligned", True),
    ("g4fe", 256, 4097, 6, 6, 12, "strided", True),
    ("g4fe", 64, 77, 2, 7, 13, "strided", True),
    ("g4fe", 128, 8195, 2, 4, 15, "dense", True),
    ("g4fe", 128, 3, 6, 8, 15, "strided", True),
    ("g4fe", 64, 0, 6, 8, 15, "dense", True),
]


def _id(c):
    entry, H, R, nfeat, ldf, flags, layout, bias = c
    return f"{entry}-H{H}-R{R}-nf{nfeat}-ldf{ldf}-fl{flags}-{layout}" + ("" if bias else "-nobias")


def _seed_of(c):
    entry, H, R, nfeat, ldf, flags, layout, bias = c
    return 1000 * H + 7 * R + nfeat + 13 * ldf


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gru_ln_bwd_matches_float64(case):
    entry, H, R, nfeat, ldf, flags, layout, bias = case
    seed = _seed_of(case)
    inp, ref, yard = _case(R, H, nfeat, ldf, seed)
    seeds = _seeds(H, nfeat, R, seed)
    packed, planes = bool(flags & 4), bool(flags & 8)
    has_rexp = entry == "g4fe"
    out = _launch(entry, H, R, nfeat, ldf, flags & 7, layout, bias, inp, seeds)  # fp32 rows
    _canaries(out, R, H, packed, bias, nfeat, seeds, has_rexp)
    if R == 0:  # returns OK and writes nothing
        assert bool((out["D"] == CANARY).all()) and bool((out["dh"] == CANARY).all())
        for k in ("dbi", "dbh", "dfeat"):
            assert torch.equal(out[k], seeds[k]), k
        assert torch.equal(out["dln"], seeds["dln"]) if flags & 1 else bool(torch.isnan(out["dln"]).all())
        if planes:
            outp = _launch(entry, H, R, nfeat, ldf, flags, layout, bias, inp, seeds)
            assert bool((outp["D"] == CANARY).all())
        return
    report = []
    _check_values(out, ref, yard, seeds, R, H, nfeat, flags, bias, report)
    zero_rows = _check_value_rows(out, inp, R, H, packed)
    if has_rexp:
        rows = out["D"][:R, :4 * H].contiguous()
        rexp = out["rexp"][:R]
        assert torch.equal(rexp, row_exp(rows)), "rexp is not row_exp of the rows the launch wrote"
        assert bool((rexp[zero_rows] == KZERO).all()) and bool((rexp[~zero_rows] != KZERO).all())
    if planes:
        outp = _launch(entry, H, R, nfeat, ldf, flags, layout, bias, inp, seeds)
        _canaries(outp, R, H, packed, bias, nfeat, seeds, has_rexp)
        for k in ("dh", "dln", "dbi", "dbh", "dfeat", "rexp"):
            assert torch.equal(outp[k].view(torch.int32), out[k].view(torch.int32)), f"planes launch: {k} differs"
        got = outp["D"][:R, :4 * H].contiguous().view(torch.int16)
        want = host_planes(rows, rexp).view(torch.int16)
        assert torch.equal(got, want), "planes are not the fp16x2 split of the fp32 rows"
    print(f"gru bwd {_id(case)}: max err / E32, worst (err - 1e-5 |ref|) / E32:",
          [(w, round(a, 2), round(b, 2)) for w, a, b in report])


def test_cases_cover_every_dimension():
    """The case table spans what the kernel dispatches on (a guard against trimming it)."""
    col = lambda i: {c[i] for c in CASES}
    assert col(0) == {"g4", "g4f", "g4fe"} and col(1) == {64, 128, 256}
    assert col(2) == {0, 1, 3, 4, 5, 77, 4097, 8195}
    assert {(c[3], c[4]) for c in CASES} >= {(0, 0), (2, 4), (2, 7), (6, 8), (6, 6)}
    assert {c[5] & 3 for c in CASES} == {0, 1, 2, 3} and {c[5] >> 2 for c in CASES} == {0, 1, 3}
    assert {(c[5] & 4, c[7]) for c in CASES} >= {(0, False), (4, False)}
    for H in (128, 256):  # nfeat 6: vector and scalar body, each with and without planes
        assert {(c[6] == "misaligned", bool(c[5] & 8)) for c in CASES if c[1] == H and c[3] == 6} >= {
            (False, False), (True, False), (False, True), (True, True)}
