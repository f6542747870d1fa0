"""CPU: the fused GRU + LayerNorm forward's host side and the inputs of its placement tests.

* every MSAT_REQUIRE of msat_gru_ln_fused_fwd / _x3r / _h2r and of the two transposed splitters returns -1 with
  its message before anything is launched (dummy non-null pointers, never dereferenced); R == 0 is OK with
  NULL pointers;
* the case tables of tests/gru_placement.py name every factor tests/test_gru_fused_placement_gpu.py promises;
* the float32 restatement on the CPU alone meets every bar of that file on the chosen inputs, so that a
  failing GPU case means the kernel and not the inputs."""
import pytest
import torch

import gru_placement as gr

A16 = 0x10000  # a 16-byte aligned dummy address


def _refused(rc, msg):
    from marlsat import _lib

    assert rc == -1
    assert msg in _lib.lib.msat_last_error().decode(), _lib.lib.msat_last_error().decode()


def _args(bad):
    a = dict(x0=A16, ld0=128, w0=128, x1=A16, ld1=8, w1=8, x2=None, ld2=0, w2=0, hprev=A16, ldp=128, wi=A16, bi=A16,
             wh=A16, bh=A16, sc=A16, lb=A16, out=A16, ldo=128, g4=A16, ldg=512, R=5, H=128, kxp=160, wi3=A16, wh3=A16,
             flags=A16, wbad=A16)
    a.update(bad)
    return a


def _call(entry, bad):
    from marlsat import _lib

    a = _args(bad)
    segs = [a["x0"], a["ld0"], a["w0"], a["x1"], a["ld1"], a["w1"], a["x2"], a["ld2"], a["w2"], a["hprev"], a["ldp"]]
    tail = [a["out"], a["ldo"], a["g4"], a["ldg"], a["R"], a["H"]]
    if entry == "plain":
        return _lib.lib.msat_gru_ln_fused_fwd(*segs, a["wi"], a["bi"], a["wh"], a["bh"], a["sc"], a["lb"], *tail, None)
    if entry == "x3r":
        return _lib.lib.msat_gru_ln_fused_fwd_x3r(*segs, a["wi"], a["kxp"], a["bi"], a["wh"], a["bh"], a["sc"],
                                                  a["lb"], *tail, None)
    return _lib.lib.msat_gru_ln_fused_fwd_h2r(*segs, a["wi"], a["wh"], a["wi3"], a["wh3"], a["kxp"], a["bi"], a["bh"],
                                              a["sc"], a["lb"], *tail, a["flags"], a["wbad"], None)


# refusals the three entry points share (the register-A forms word some of them differently)
COMMON = [
    (dict(R=-1), "R < 0", "R < 0"),
    (dict(bi=None), "NULL pointer", "NULL pointer"),
    (dict(out=None), "NULL pointer", "NULL pointer"),
    (dict(ldo=127), "bad dims", "bad dims"),
    (dict(ldp=124), "bad dims", "bad dims"),
    (dict(ldg=508), "bad dims", "bad dims"),
    (dict(w1=6), "segment 1 width 6 must be a multiple of 4", "segment 1 width 6 must be a multiple of 4"),
    (dict(w0=-4), "segment 0 width -4 must be a multiple of 4", "segment 0 width -4 must be a multiple of 4"),
    (dict(ld1=4), "segment 1 must be 16-byte aligned", "segment 1 must be 16-byte aligned"),
    (dict(ld0=130), "segment 0 must be 16-byte aligned", "segment 0 must be 16-byte aligned"),
    (dict(x1=A16 + 4), "segment 1 must be 16-byte aligned", "segment 1 must be 16-byte aligned"),
    (dict(x2=None, ld2=4, w2=4), "segment 2 must be 16-byte aligned", "segment 2 must be 16-byte aligned"),
    (dict(w0=0), "empty input", "empty input"),
    (dict(hprev=A16 + 4), "hprev / weights must be 16-byte aligned", "hprev / weight planes must be 16-byte aligned"),
    (dict(ldp=130), "hprev / weights must be 16-byte aligned", "hprev / weight planes must be 16-byte aligned"),
    (dict(wi=A16 + 8), "hprev / weights must be 16-byte aligned", "hprev / weight planes must be 16-byte aligned"),
    (dict(wh=A16 + 4), "hprev / weights must be 16-byte aligned", "hprev / weight planes must be 16-byte aligned"),
]


@pytest.mark.parametrize("entry", ["plain", "x3r", "h2r"])
@pytest.mark.parametrize("bad,msg_plain,msg_r", COMMON, ids=[str(b) for b, _, _ in COMMON])
def test_shared_refusals(entry, bad, msg_plain, msg_r):
    _refused(_call(entry, bad), msg_plain if entry == "plain" else msg_r)


@pytest.mark.parametrize("H", [0, 32, 96, 512])
def test_fp32_kernel_width_refused(H):
    _refused(_call("plain", dict(H=H, ldo=512, ldp=512, ldg=2048)), "gru_ln_fused: H must be 64, 128 or 256")


KXP_MSG = "kxp must be >= Kx and a multiple of 32"
OUT_MSG = "out / g4 rows must be 16-byte aligned"


@pytest.mark.parametrize("entry", ["x3r", "h2r"])
@pytest.mark.parametrize("bad,msg", [
    (dict(H=64), "H must be 128 (got 64)"), (dict(H=256, ldo=256, ldp=256, ldg=1024), "H must be 128 (got 256)"),
    (dict(kxp=136), KXP_MSG), (dict(kxp=128), KXP_MSG), (dict(out=A16 + 4), OUT_MSG), (dict(ldo=130), OUT_MSG),
    (dict(g4=A16 + 8), OUT_MSG), (dict(ldg=514), OUT_MSG),
], ids=str)
def test_register_a_refusals(entry, bad, msg):
    _refused(_call(entry, bad), "gru_ln_fused_fwd_x3r/h2r: " + msg)


@pytest.mark.parametrize("bad,msg", [
    (dict(flags=None), "NULL flags"), (dict(wbad=None), "NULL flags"), (dict(wi3=None), "bf16x3 planes"),
    (dict(wh3=None), "bf16x3 planes"), (dict(wi3=A16 + 8), "bf16x3 planes"), (dict(wh3=A16 + 2), "bf16x3 planes"),
], ids=str)
def test_h2r_refusals(bad, msg):
    _refused(_call("h2r", bad), "gru_ln_fused_fwd_h2r: " + msg)


def test_empty_batch_is_ok_with_null_pointers():
    """R == 0 returns OK before any pointer is looked at (R < 0 is still refused); so does the bf16 splitter at
    K == 0 or N == 0."""
    from marlsat import _lib

    for entry in ("plain", "x3r", "h2r"):
        none = dict(x0=None, x1=None, hprev=None, wi=None, bi=None, wh=None, bh=None, sc=None, lb=None, out=None,
                    g4=None, wi3=None, wh3=None, flags=None, wbad=None, R=0)
        assert _call(entry, none) == 0
        _refused(_call(entry, dict(none, R=-1)), "R < 0")
    assert _lib.lib.msat_split_bf16x3_t(None, 0, 4, 4, 32, None, None) == 0
    assert _lib.lib.msat_split_bf16x3_t(None, 4, 0, 4, 32, None, None) == 0


@pytest.mark.parametrize("bad", [dict(W=None), dict(planes=None), dict(ldw=380), dict(Kp=128), dict(K=-1), dict(N=-4)],
                         ids=str)
def test_split_bf16x3_t_refusals(bad):
    from marlsat import _lib

    a = dict(W=A16, K=136, N=384, ldw=384, Kp=160, planes=A16)
    a.update(bad)
    _refused(_lib.lib.msat_split_bf16x3_t(a["W"], a["K"], a["N"], a["ldw"], a["Kp"], a["planes"], None),
             "bad split_bf16x3_t args")


@pytest.mark.parametrize("bad", [dict(W=None), dict(planes=None), dict(bad=None), dict(ldw=380), dict(Kp=128),
                                 dict(K=0), dict(N=0), dict(K=-1)], ids=str)
def test_split_f16x2_t_refusals(bad):
    from marlsat import _lib

    a = dict(W=A16, K=136, N=384, ldw=384, Kp=160, planes=A16, bad=A16)
    a.update(bad)
    _refused(_lib.lib.msat_split_f16x2_t(a["W"], a["K"], a["N"], a["ldw"], a["Kp"], a["planes"], a["bad"], None),
             "bad split_f16x2_t args")


# ----------------------------------------------------------------------------------------------------------
# the tables

@pytest.mark.parametrize("group", sorted(gr.FACTORS))
def test_case_tables_name_every_factor(group):
    cases = gr.TABLES[group]
    got = {t for c in cases for t in c.tags}
    assert set(gr.FACTORS[group]) <= got, sorted(set(gr.FACTORS[group]) - got)
    names = [c.name for c in cases]
    assert len(names) == len(set(names)), "duplicate case names"


def test_tile_edge_table_is_the_full_product():
    got = {(c.layout, c.H, c.R, c.tags[1]) for c in gr.TILE_EDGE_CASES}
    want = {(lay, H, R, k) for lay, H in gr.LAYOUTS for R in gr.TILE_EDGE_ROWS for k in ("var8", "clause4")}
    assert got == want and len(gr.TILE_EDGE_CASES) == len(want)
    for c in gr.TILE_EDGE_CASES:  # the kinds are what the fused-order encoder passes
        assert c.widths == ((c.H, 8) if "var8" in c.tags else (2 * c.H, 4))
        assert c.segs[0][1] == (gr.Placement(0, c.H) if "var8" in c.tags else gr.P0)
    huge = {(c.R, c.tags[1]) for c in gr.TILE_EDGE_HUGE_CASES if c.layout == "h2r" and c.fill == "huge"}
    assert huge == {(R, k) for R in gr.TILE_EDGE_ROWS for k in ("var8", "clause4")}


def test_tags_say_what_the_case_does():
    """A tag is a claim about the case's numbers: restate each from the numbers."""
    for c in gr.PLACEMENT_CASES + gr.SEGMENT_CASES + gr.PADDING_CASES:
        H = c.H
        if c.layout != "plain":  # what the register-A forms refuse is never in a table
            assert c.out.off % 4 == 0 and c.out.pad % 4 == 0 and c.g4.off % 4 == 0 and c.g4.pad % 4 == 0
        for w, p in c.segs:
            assert w % 4 == 0 and p.off % 4 == 0 and p.pad % 4 == 0
        assert c.hprev.off % 4 == 0 and c.hprev.pad % 4 == 0 and c.kxp % 32 == 0 and c.kxp >= c.Kx
        t = set(c.tags)
        if "base" in t:
            assert all(p == gr.P0 for _, p in c.segs) and (c.hprev, c.out, c.g4) == (gr.P0,) * 3
            assert (c.bi, c.bh, c.sc, c.lb, c.kxp_extra) == (0,) * 5
        if "out-ld2H@H" in t:
            assert c.out == gr.Placement(H, H)
        if "hprev-ld2H@0" in t:
            assert c.hprev == gr.Placement(0, H)
        if "ldo%4" in t:
            assert (H + c.out.pad) % 4 != 0
        if "ldg%4" in t:
            assert (4 * H + c.g4.pad) % 4 != 0
        if "feat-ld8-w4" in t:
            assert c.segs[1] == (4, gr.Placement(0, 4))
        if "boundary@4" in t:
            assert c.widths[0] == 4
        if "three-segments" in t:
            assert len(c.segs) == 3 and c.widths == (H // 2, H // 2, 8)
        if "boundary-in-32-step-and-16-slab" in t:
            b0, b1 = c.widths[0], c.widths[0] + c.widths[1]
            assert b0 % 32 and b0 % 16 and b1 % 32 and b1 % 16 and (c.Kx, c.kxp) == (108, 128)
        if "Kx-quad-past-32" in t:
            assert c.Kx % 32 == 4 and c.widths[1] == 4
        if "one-segment-2H" in t:
            assert c.widths == (2 * H,)
        if "kxp+32" in t:
            assert c.kxp == (c.Kx + 31) // 32 * 32 + 32
        if "padline-200" in t:
            assert c.h_row0 == 200.0 and c.kxp > c.Kx and 200.0 * 2 ** 7 < 2 ** 15
        if "fill-huge" in t:
            assert c.fill == "huge" and gr.HUGE * 2 ** 7 >= 2 ** 15  # a leaked guard value would raise the flag
    for c in gr.PADDING_CASES:
        assert any(t.startswith("fill-") for t in c.tags)
    # (d) reruns every segment layout and the base placement of every kernel with both fills
    rerun = {(c.layout, c.H, c.widths, c.kxp_extra, c.fill) for c in gr.PADDING_CASES if c.h_row0 is None}
    for c in gr.SEGMENT_CASES + [gr.base_case(lay, H) for lay, H in gr.LAYOUTS]:
        for fill in ("nan", "huge"):
            assert (c.layout, c.H, c.widths, c.kxp_extra, fill) in rerun


def test_gate_table_is_the_full_product():
    assert len(set(gr.GATE_CASES)) == len(gr.GATE_CASES) == len(gr.LAYOUTS) * 3 * len(gr.GATE_M) * 2
    assert set(gr.GATE_M) == {20.0, 89.0, 104.0, 1.0e4}
    g = gr.tanh_cut_grid(64)
    for s in (1.0, -1.0):
        for k in range(-3, 4):
            assert float(torch.tensor(s * (gr.TANH_CUT + k * 2.0 ** -24), dtype=torch.float32)) in g.tolist()
    assert len(set(g.tolist())) == 64  # distinct floats: an ulp at 0.625 is 2^-24


# ----------------------------------------------------------------------------------------------------------
# the float32 restatement alone meets every bar on the chosen inputs

def _f32_meets_bars(d, tape=True, out=True):
    ref, tp, ab = gr.reference(d)
    r32, t32, _ = gr.reference(d, torch.float32)
    assert bool(torch.isfinite(r32).all()) and bool(torch.isfinite(t32).all())
    if out:
        err = (r32.double() - ref).abs()
        assert bool((err <= gr.out_bar(ref)).all()), float((err / gr.out_bar(ref)).max())
    if tape:
        terr = (t32.double() - tp).abs()
        assert bool((terr <= gr.tape_bar(ab)).all()), float((terr / gr.tape_bar(ab)).max())
    return ref, r32


def test_float32_restatement_meets_the_bars_on_every_table_case():
    seen = set()
    for c in (gr.TILE_EDGE_CASES + gr.PLACEMENT_CASES + gr.SEGMENT_CASES + gr.PADDING_CASES
              + gr.PADLINE_FLAG_CASES):
        key = (c.H, c.R, c.widths, c.h_row0)
        if key not in seen:
            seen.add(key)
            _f32_meets_bars(gr.case_data(c))


def test_float32_restatement_meets_the_bars_at_the_gate_limits():
    seen = set()
    for _, H, R, gate, m, sign in gr.GATE_CASES:
        if (H, R, gate, m, sign) not in seen:
            seen.add((H, R, gate, m, sign))
            _f32_meets_bars(gr.gate_limit_data(H, R, gate, m, sign))
    for lay, H in gr.LAYOUTS:
        R = gr.ragged_rows(lay)
        d = gr.zero_data(H, R)
        ref, r32 = _f32_meets_bars(d)
        assert torch.equal(r32, d.lb.expand(R, H)) and torch.equal(ref, d.lb.double().expand(R, H))
        _f32_meets_bars(gr.z_saturated_data(H, R))
        _f32_meets_bars(gr.tanh_cut_data(H, R))
        for c in gr.CONST_ROWS:
            d = gr.z_saturated_data(H, R, h_const=c)
            ref, r32 = _f32_meets_bars(d)
            assert torch.equal(ref, d.lb.double().expand(R, H))  # every partial sum exact: variance 0
        for c in gr.NEAR_CONST:  # measured against the float32 restatement's own error, which must exist
            d = gr.z_saturated_data(H, R, near=c)
            ref, r32 = _f32_meets_bars(d, out=False)
            e32 = float((r32.double() - ref).abs().max())
            print(f"near-constant rows c={c} H={H}: E32 = {e32:.3g}")
            assert e32 == e32 and e32 < float("inf")
