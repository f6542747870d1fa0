"""GPU: msat_assign_loss (the assignment predictor's per-variable two-class cross-entropy, its gradient, the
arg-max assignment and that assignment's satisfaction check) against a NumPy float64 restatement on the same fp32
inputs.

Bars.  Exact: pred, sample_correct, sample_unsat, sample_solved and the four counting sums.  dlogits and sample_nll:
within 2^-23 |ref| (one fp32 rounding of an fp64 value is 2^-24; the same again for the device's exp / log1p: the
bar tests/test_single_ppo_loss_gpu.py holds its fp64-evaluated rows to).  sums[0]: within S V 2^-53 sums[0] of the
float64 sum (every term is >= 0: the bound of any summation order).  Every dlogits row sums to exactly 0.

``minibatch`` is MB = 5 in every case, whatever S (the kernel takes any; S = 1 and 3 are then micro-batches of a
minibatch of 5).  The reason is the planted +80 gap: its gradient is e^-80 / (minibatch V) = 1.8e-35 / (minibatch V),
and the 2^-23 relative bar is a statement about fp32 *normal* results (>= 1.18e-38), so minibatch V must stay below
1535; V goes up to 257.

Logits, labels and outputs sit at addresses that are no multiple of 16 bytes, with guards around every output."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (63, 65), (64, 64), (65, 130), (130, 218), (257, 7))  # (V, C)
SS = (1, 3, 130)  # one wave of a workgroup; three of its four; 33 workgroups with a half-filled last one
# past the launch's cap of 8192 workgroups x 4 samples: the first workgroup takes a second trip of the sample loop
# (and of the two barriers in it) with two of its four waves live
S_PAST_CAP = 8192 * 4 + 2
CASES = [(V, C, S) for S in SS for V, C in SHAPES] + [(3, 2, S_PAST_CAP)]
N = 3
MB = 5
ULP = 2.0 ** -23
INIT = np.array([0.0, 3.0, 7.0, 11.0, 13.0])  # sums[0] starts at 0: the device's total is then its sum alone
OFF, GUARD = 3, 5
LIT_NULL, LIT_ABSENT = 0xFFFF, 0xFFFE
KINDS = ("tie", "gap_pos", "gap_neg", "inf_pos", "inf_neg", "nan0", "nan1", "label2", "label255")


# ------------------------------------------------------------------ inputs ----
def _clauses(V, C, rng):
    """(N, C, 3) int32: random 3-literal clauses, then (room permitting) a literal 0, a clause that is two real
    literals and a literal 0, and a variable twice in a clause with both signs."""
    cl = rng.integers(1, V + 1, (N, C, 3)) * rng.choice([-1, 1], (N, C, 3))
    for n in range(N):
        cl[n, 0 % C, 1] = 0  # literal 0 among real ones
        if C > 1:
            cl[n, 1, 2] = 0  # "2-wide" in a 3-wide pool: MSAT_LIT_NULL in slot 2, MSAT_LIT_ABSENT in slot 3
        if C > 2:
            v = int(rng.integers(1, V + 1))
            cl[n, 2] = (v, -v, v)  # both signs of one variable: always true
        if C > 3:
            cl[n, 3] = 0  # an all-zero clause: never true
    return cl.astype(np.int32)


def _problem_idx(S, rng):
    """Repeats, one value below 0 and one >= N (clamped to 0 and N - 1); S = 1 alternates the two."""
    p = rng.integers(0, N, S).astype(np.int32)
    p[0] = -2
    p[-1] = N + 4 if S > 1 else p[-1]
    if S > 2:
        p[1] = p[2] if S > 3 else 1
    return p


def _kinds_of(V, C, S):
    """{kind: flat row index}: all of them where S * V >= len(KINDS), else a rotation over the cases."""
    n = S * V
    if n >= len(KINDS):
        step = n // len(KINDS)
        return {k: i * step + (i % min(step, V)) for i, k in enumerate(KINDS)}
    start = (7 * S + C) % len(KINDS)
    return {KINDS[(start + i) % len(KINDS)]: i for i in range(n)}


def _inputs(V, C, S):
    rng = np.random.default_rng(100000 * V + 100 * C + S)
    lg = (3.0 * rng.standard_normal((S * V, 2))).astype(np.float32)
    lab = rng.integers(0, 2, S * V).astype(np.uint8)
    kinds = _kinds_of(V, C, S)
    for k, r in kinds.items():
        if k == "tie":
            lg[r] = np.float32(0.37)
        elif k == "gap_pos":  # the label's logit 80 above the other: p_other = e^-80
            lg[r, lab[r]], lg[r, 1 - lab[r]] = np.float32(41.5), np.float32(-38.5)
        elif k == "gap_neg":  # 80 below: nll = 80
            lg[r, lab[r]], lg[r, 1 - lab[r]] = np.float32(-38.5), np.float32(41.5)
        elif k == "inf_pos":
            lg[r, 1] = np.float32("inf")
        elif k == "inf_neg":
            lg[r, 1] = np.float32("-inf")
        elif k == "nan0":
            lg[r, 0] = np.float32("nan")
        elif k == "nan1":
            lg[r, 1] = np.float32("nan")
        elif k == "label2":
            lab[r] = 2
        elif k == "label255":
            lab[r] = 255
    return lg, lab, _clauses(V, C, rng), _problem_idx(S, rng), kinds


# --------------------------------------------------------------- reference ----
def _unpack(packed):
    return packed.view(np.uint16).astype(np.int64)


def ref_unsat(pred, codes, pidx):
    """Clauses each sample's assignment leaves false, by msat_walksat's rule on the library's own codes."""
    S = pred.shape[0]
    Np = codes.shape[0]
    cd = codes[np.clip(np.asarray(pidx, np.int64), 0, Np - 1)]  # (S, C, 4)
    real = cd < LIT_ABSENT
    x = pred[np.arange(S)[:, None, None], np.where(real, cd >> 1, 0)]
    true = real & (((x ^ cd) & 1) == 1)
    return (~true.any(2)).sum(1).astype(np.int32)


def reference(lg, lab, S, V, minibatch, codes, pidx):
    l = lg.astype(np.float64)
    with np.errstate(invalid="ignore"):
        pred = (lg[:, 1] > lg[:, 0]).astype(np.uint8)
    valid = (lab <= 1) & np.isfinite(lg).all(1)
    lb = np.where(valid, lab, 0).astype(np.int64)
    r = np.arange(S * V)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(valid, l[r, lb] - l[r, 1 - lb], 0.0)
        nll = np.where(valid, np.maximum(-d, 0.0) + np.log1p(np.exp(-np.abs(d))), 0.0)
        e = np.exp(-np.abs(d))
        p_other = np.where(d >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    g = np.where(valid, p_other / (minibatch * V), 0.0)
    dl = np.zeros((S * V, 2))
    dl[r, lb] = -g
    dl[r, 1 - lb] = g
    correct = (valid & (pred == lab)).reshape(S, V).sum(1).astype(np.int32)
    unsat = ref_unsat(pred.reshape(S, V), codes, pidx)
    return {"pred": pred.reshape(S, V), "valid": valid, "nll": nll, "dlogits": dl,
            "sample_nll": nll.reshape(S, V).sum(1), "correct": correct, "unsat": unsat,
            "solved": (unsat == 0).astype(np.uint8)}


# ------------------------------------------------------------------ device ----
def _guarded(n, dtype, fill):
    buf = torch.full((OFF + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[OFF:OFF + n]


def _at_odd_offset(a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.empty(OFF + t.numel(), dtype=t.dtype, device="cuda")
    buf[OFF:] = t.cuda()
    return buf[OFF:]


def run(lg, lab, S, V, minibatch, dpool, pidx, sums_d, predict_only=False):
    """One call.  -> dict of host arrays (dlogits / sample_nll / correct None in predict-only mode)."""
    from marlsat import _lib

    lg_d = _at_odd_offset(lg)
    assert lg_d.data_ptr() % 16 != 0
    lab_d = None if predict_only else _at_odd_offset(lab)
    pidx_d = torch.from_numpy(pidx).cuda()
    specs = {"dlogits": (2 * S * V, torch.float32, -77.25), "pred": (S * V, torch.uint8, 99),
             "sample_nll": (S, torch.float32, -77.25), "correct": (S, torch.int32, -777),
             "unsat": (S, torch.int32, -777), "solved": (S, torch.uint8, 99)}
    skip = ("dlogits", "sample_nll", "correct") if predict_only else ()
    bufs = {k: _guarded(*v) for k, v in specs.items() if k not in skip}
    p = lambda k: bufs[k][1].data_ptr() if k in bufs else None
    N_, C = dpool.packed.shape[:2]
    _lib.check(_lib.lib.msat_assign_loss(
        lg_d.data_ptr(), S, V, _lib.ptr(lab_d), minibatch, dpool.packed.data_ptr(), N_, C, pidx_d.data_ptr(),
        p("dlogits"), p("pred"), p("sample_nll"), p("correct"), p("unsat"), p("solved"), _lib.ptr(sums_d),
        _lib.stream_ptr()), "msat_assign_loss")
    torch.cuda.synchronize()
    out = {}
    for k, (buf, v) in bufs.items():  # the guards stay as they were
        fill, n = specs[k][2], v.numel()
        assert bool((buf[:OFF] == fill).all()) and bool((buf[OFF + n:] == fill).all()), k
        out[k] = v.cpu().numpy()
    return out


def _within(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref != 0, err / np.abs(ref), np.where(err > 0, np.inf, 0.0))
    print(f"  {what}: max err / |ref| {rel.max() if rel.size else 0.0:.3g} (bar {ULP:.3g})")
    bad = err > ULP * np.abs(ref)
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], ref[bad][:4])


def _pool(V, C, cl):
    from marlsat import SATEnv

    return SATEnv(V, C, max_steps=4, vars_per_agent=V).make_pool(cl)


def test_small_cases_cover_every_planted_row():
    seen = set()
    for V, C in SHAPES:
        for S in SS:
            k = _kinds_of(V, C, S)
            assert len(set(k.values())) == len(k) and max(k.values()) < S * V
            seen |= set(k)
            if S * V >= len(KINDS):
                assert set(k) == set(KINDS)
    assert seen == set(KINDS)
    assert MB * max(V for V, _ in SHAPES) < 1535  # the +80 gap's gradient stays an fp32 normal


@pytest.mark.parametrize("V,C,S", CASES)
def test_assign_loss_matches_float64(V, C, S):
    lg, lab, cl, pidx, kinds = _inputs(V, C, S)
    dpool = _pool(V, C, cl)
    codes = _unpack(dpool.packed.cpu().numpy())
    assert (codes[:, :, 3] == LIT_ABSENT).all() and (codes[:, 0, 1] == LIT_NULL).all()
    ref = reference(lg, lab, S, V, MB, codes, pidx)
    sums_d = torch.from_numpy(INIT.copy()).cuda()
    out = run(lg, lab, S, V, MB, dpool, pidx, sums_d)
    print(f"assign_loss V={V} C={C} S={S} kinds={sorted(kinds)} invalid rows {int((~ref['valid']).sum())} "
          f"unsat {out['unsat'][:6]}")
    # exact outputs
    assert np.array_equal(out["pred"].reshape(S, V), ref["pred"])
    assert np.array_equal(out["correct"], ref["correct"])
    assert np.array_equal(out["unsat"], ref["unsat"])
    assert np.array_equal(out["solved"], ref["solved"])
    dl = out["dlogits"].reshape(S * V, 2)
    assert np.isfinite(dl).all() and np.isfinite(out["sample_nll"]).all()
    inv = ~ref["valid"]
    assert inv.sum() == sum(k in kinds for k in ("inf_pos", "inf_neg", "nan0", "nan1", "label2", "label255"))
    assert (dl[inv].view(np.int32) == 0).all()  # a zero row, +0 both
    assert ((dl[:, 0] + dl[:, 1]).view(np.int32) & 0x7FFFFFFF == 0).all()  # every row sums to exactly 0
    assert (dl[:, 0] == -dl[:, 1]).all()
    _within(dl, ref["dlogits"], "dlogits")
    _within(out["sample_nll"], ref["sample_nll"], "sample_nll")
    if "gap_pos" in kinds:
        r = kinds["gap_pos"]
        assert 0 < abs(dl[r, 0]) and abs(dl[r, 0]) >= np.finfo(np.float32).tiny  # a normal, not flushed
    sums = sums_d.cpu().numpy()
    total = ref["nll"].sum()
    err = abs((sums[0] - INIT[0]) - total)
    bound = S * V * 2.0 ** -53 * total
    print(f"  sums[0]: {sums[0]!r} against {total!r}: err {err:.3g}, S V 2^-53 sums[0] = {bound:.3g}")
    assert err <= bound, (err, bound)
    assert sums[1] == INIT[1] + ref["correct"].sum()
    assert sums[2] == INIT[2] + ref["valid"].sum()
    assert sums[3] == INIT[3] + inv.sum()
    assert sums[4] == INIT[4] + ref["solved"].sum()

    # two identical calls: bitwise equal everywhere
    sums_2 = torch.from_numpy(INIT.copy()).cuda()
    again = run(lg, lab, S, V, MB, dpool, pidx, sums_2)
    for k in out:
        assert np.array_equal(out[k].view(np.uint8), again[k].view(np.uint8)), k
    assert np.array_equal(sums_2.cpu().numpy().view(np.int64), sums.view(np.int64))

    # predict only: the same pred / unsat / solved, sums[0..3] untouched, sums[4] accumulated
    sums_p = torch.from_numpy(INIT.copy()).cuda()
    po = run(lg, None, S, V, MB, dpool, pidx, sums_p, predict_only=True)
    for k in ("pred", "unsat", "solved"):
        assert np.array_equal(po[k], out[k]), k
    sp = sums_p.cpu().numpy()
    assert np.array_equal(sp[:4].view(np.int64), INIT[:4].view(np.int64)) and sp[4] == INIT[4] + ref["solved"].sum()
    run(lg, None, S, V, MB, dpool, pidx, None, predict_only=True)  # sums NULL: nothing accumulated, no fault

    if S < 2:
        return
    # a batch cut into two calls at the same minibatch: bitwise the one-call rows
    two = torch.from_numpy(INIT.copy()).cuda()
    h = S // 2
    parts = [run(lg[a * V:b * V], lab[a * V:b * V], b - a, V, MB, dpool, pidx[a:b], two) for a, b in ((0, h), (h, S))]
    for k in out:
        cat = np.concatenate([p[k] for p in parts])
        assert np.array_equal(cat.view(np.uint8), out[k].view(np.uint8)), k
    t2 = two.cpu().numpy()
    assert np.array_equal(t2[1:], sums[1:])
    # each half within its own bound, and one more rounding where the second call adds to the first's total
    assert abs(t2[0] - total) <= bound + 2.0 ** -53 * total


def test_two_wide_pool_has_absent_slots():
    """A pool of 2-literal clauses: slots 2 and 3 are MSAT_LIT_ABSENT, inert whatever the assignment."""
    V, C, S = 9, 11, 4
    rng = np.random.default_rng(5)
    cl = (rng.integers(1, V + 1, (N, C, 2)) * rng.choice([-1, 1], (N, C, 2))).astype(np.int32)
    dpool = _pool(V, C, cl)
    codes = _unpack(dpool.packed.cpu().numpy())
    assert (codes[:, :, 2:] == LIT_ABSENT).all()
    lg = rng.standard_normal((S * V, 2)).astype(np.float32)
    pidx = np.array([0, 2, 1, 2], np.int32)
    out = run(lg, None, S, V, 1, dpool, pidx, None, predict_only=True)
    pred = (lg[:, 1] > lg[:, 0]).astype(np.uint8).reshape(S, V)
    x = pred[np.arange(S)[:, None, None], np.abs(cl[pidx]) - 1]
    want = (~((x == 1) == (cl[pidx] > 0)).any(2)).sum(1)  # straight from the signed literals
    assert np.array_equal(out["unsat"], want) and want.sum() > 0
    assert np.array_equal(out["unsat"], ref_unsat(pred, codes, pidx))


def test_planted_solution_is_solved_and_its_neighbour_is_not():
    """Cannot pass vacuously: logits of +-5 towards an instance's planted solution satisfy it; negating one
    variable of a clause that solution satisfies through that variable alone leaves a false clause."""
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses, generate_sat_solution

    V, C, seed = 20, 91, 4242
    cl = generate_sat_clauses(V, C, 3, seed)
    sol = generate_sat_solution(V, seed).astype(np.uint8)
    lit_true = (sol[np.abs(cl) - 1] == 1) == (cl > 0)
    assert lit_true.any(1).all()
    crit = np.flatnonzero(lit_true.sum(1) == 1)
    assert crit.size, "no unit-critical clause in this instance"
    v = abs(int(cl[crit[0]][lit_true[crit[0]]][0])) - 1
    flipped = sol.copy()
    flipped[v] ^= 1
    dpool = _pool(V, C, cl[None])
    lab = np.concatenate([sol, sol])
    lg = np.zeros((2 * V, 2), np.float32)
    for s, x in enumerate((sol, flipped)):
        lg[s * V + np.arange(V), x] = 5.0
        lg[s * V + np.arange(V), 1 - x] = -5.0
    sums_d = torch.zeros(5, dtype=torch.float64, device="cuda")
    out = run(lg, lab, 2, V, 2, dpool, np.zeros(2, np.int32), sums_d)
    assert out["unsat"][0] == 0 and out["solved"][0] == 1 and out["correct"][0] == V
    assert out["unsat"][1] >= 1 and out["solved"][1] == 0 and out["correct"][1] == V - 1
    assert np.array_equal(out["pred"].reshape(2, V), np.stack([sol, flipped]))
    s = sums_d.cpu().numpy()
    assert s[1] == 2 * V - 1 and s[2] == 2 * V and s[3] == 0 and s[4] == 1


def test_empty_batch_and_argument_errors():
    from marlsat import _lib

    L = _lib.lib
    st = _lib.stream_ptr()
    f = torch.zeros(32, device="cuda")
    i = torch.zeros(8, dtype=torch.int32, device="cuda")
    u = torch.zeros(32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(32, dtype=torch.int16, device="cuda")
    s = torch.from_numpy(INIT.copy()).cuda()
    good = dict(logits=f.data_ptr(), S=2, V=2, labels=u.data_ptr(), mb=2, lits=w.data_ptr(), N=1, C=1,
                pidx=i.data_ptr(), dl=f.data_ptr(), pred=u.data_ptr(), nll=f.data_ptr(), cor=i.data_ptr(),
                uns=i.data_ptr(), sol=u.data_ptr(), sums=s.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        return L.msat_assign_loss(a["logits"], a["S"], a["V"], a["labels"], a["mb"], a["lits"], a["N"], a["C"],
                                  a["pidx"], a["dl"], a["pred"], a["nll"], a["cor"], a["uns"], a["sol"], a["sums"], st)

    assert call(S=0) == 0 and call(S=0, **{k: None for k in good if k not in ("S", "V", "mb", "N", "C")}) == 0
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), INIT)
    for kw, needle in ((dict(S=-1), "S -1"), (dict(V=0), "V 0"), (dict(V=32001), "V 32001"),
                       (dict(C=0), "num_clauses 0"), (dict(N=0), "num_problems 0"), (dict(mb=0), "minibatch 0"),
                       (dict(dl=None), "labels and dlogits"), (dict(labels=None), "labels and dlogits")):
        assert call(**kw) == -1, kw
        assert needle in L.msat_last_error().decode(), (kw, L.msat_last_error())
    for k in ("logits", "lits", "pidx", "pred", "nll", "cor", "uns", "sol", "sums"):
        assert call(**{k: None}) == -1 and "NULL" in L.msat_last_error().decode(), k
