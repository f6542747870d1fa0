"""GPU: msat_ppo_single_loss (the single-agent PPO loss, single_rl_learner.py:118-158) against float64 evaluated on
the same fp32 inputs (tests/single_oracle.py).

The kernel evaluates a row in fp64 and rounds each output once, so every output element must lie within
2^-23 * |reference| (half an ulp for the rounding, the same again for the device's exp / log).  Rows whose float64
ratio lies within 1e-6 of a clip edge are left out of the dlogits comparison (the surrogate's gradient jumps there);
the inputs are seeded so that the reference alone marks at most 1 row in 64, and never a dedicated row.  sums are
the fp64 sums of the device's own fp32 row terms on top of the caller's values (1e-12 relative), the invalid count
exact.  Inputs and outputs sit at float offsets that are no multiple of 16 bytes, with guard floats around every
output."""
import numpy as np
import pytest
import torch

import single_oracle as so

pytestmark = pytest.mark.gpu

VS = (1, 2, 63, 64, 65, 129, 257, 1024)  # one lane; two; 64 = the lanes, one below, one above; 3 and 5 rounds; 16
SS = (1, 3, 130)  # one wave of a workgroup; three of its four; 33 workgroups with a half-filled last one
# past the launch's cap of 8192 workgroups x 4 rows: the first workgroup's first three waves take a second row
S_PAST_CAP = 8192 * 4 + 3
CASES = [(V, S) for S in SS for V in VS] + [(2, S_PAST_CAP)]
CLIP_EPS, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5
ULP = 2.0 ** -23
INIT = np.array([0.5, 3.0, 7.0, 11.0])
OFF, GUARD = 3, 5  # floats before an array (12 bytes: not 16-byte aligned) and after it
KINDS = ("one_pos", "one_neg", "one_zero", "hi_pos", "hi_neg", "lo_pos", "lo_neg", "dominant", "equal", "inv_neg",
         "inv_above")


def _kinds_of(V, S):
    """The dedicated rows of a case: all of them at S = 130; the small cases rotate through them so that every
    kind is met at S = 1 and at S = 3 over the V values."""
    if S >= len(KINDS):
        return {k: i for i, k in enumerate(KINDS)}
    start = (VS.index(V) * (4 if S == 3 else 3)) % len(KINDS)
    return {KINDS[(start + i) % len(KINDS)]: i for i in range(S)}


def _inputs(V, S):
    """fp32 inputs with the dedicated rows in place, apart from the 'one_*' rows' old_logp (the kernel's own
    log-probability, filled in from a first call)."""
    rng = np.random.default_rng(1000 * V + S)
    lg = (3.0 * rng.standard_normal((S, V))).astype(np.float32)
    act = rng.integers(0, V, S).astype(np.int32)
    adv = rng.standard_normal(S).astype(np.float32)
    value = rng.standard_normal(S).astype(np.float32)
    tg = rng.standard_normal(S).astype(np.float32)
    kinds = _kinds_of(V, S)
    for k, r in kinds.items():
        if k.endswith("_pos"):
            adv[r] = np.float32(0.7)
        elif k.endswith("_neg") and k != "inv_neg":
            adv[r] = np.float32(-0.7)
        elif k == "one_zero":
            adv[r] = np.float32(0.0)
        elif k == "dominant":  # every other probability underflows to 0 in float64: p log p at p = 0 contributes 0
            act[r] = V // 2
            lg[r, V // 2] = np.float32(800.0)
        elif k == "equal":
            lg[r] = np.float32(0.37)
            adv[r] = np.float32(0.9)  # away from 0: the entropy gradient of equal logits is 0 but for rounding
        elif k == "inv_neg":
            act[r] = -1
        elif k == "inv_above":
            act[r] = V
    for k in ("inv_neg", "inv_above"):  # nothing of an invalid row is read: poison it
        if k in kinds:
            lg[kinds[k]] = np.float32("nan")
            adv[kinds[k]] = value[kinds[k]] = tg[kinds[k]] = np.float32("nan")
    lp = so.single_loss(np.nan_to_num(lg), act, np.zeros(S), np.zeros(S), np.zeros(S), np.zeros(S), CLIP_EPS,
                        ENT_COEF, VF_COEF, S)["lp"]
    old = (lp + 0.3 * rng.standard_normal(S)).astype(np.float32)  # ratios on both sides of both clip edges
    for k, r in kinds.items():
        if k.startswith("hi_"):
            old[r] = np.float32(lp[r] - np.log(3.0))  # ratio 3
        elif k.startswith("lo_"):
            old[r] = np.float32(lp[r] + np.log(3.0))  # ratio 1/3
        elif k in ("dominant", "equal"):
            old[r] = np.float32(lp[r] - 0.05)
        elif k.startswith("inv_"):
            old[r] = np.float32("nan")
    return lg, act, old, adv, value, tg, kinds


def _guarded(n, fill=-77.25):
    buf = torch.full((OFF + n + GUARD,), fill, device="cuda")
    return buf, buf[OFF:OFF + n]


def _at_odd_offset(a):
    """The array on the device at a float address that is no multiple of 16 bytes."""
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.empty(OFF + t.numel(), dtype=t.dtype, device="cuda")
    buf[OFF:] = t.cuda()
    v = buf[OFF:]
    assert v.data_ptr() % 16 != 0
    return v


def _run(lg, act, old, adv, value, tg, S, V, minibatch, sums_d):
    from marlsat import _lib

    d = [_at_odd_offset(a) for a in (lg, act, old, adv, value, tg)]
    bufs = [_guarded(S * V), _guarded(S), _guarded(3 * S)]
    _lib.check(_lib.lib.msat_ppo_single_loss(d[0].data_ptr(), S, V, *(t.data_ptr() for t in d[1:]), CLIP_EPS, ENT_COEF,
                                             VF_COEF, minibatch, *(v.data_ptr() for _, v in bufs),
                                             sums_d.data_ptr(), _lib.stream_ptr()), "msat_ppo_single_loss")
    torch.cuda.synchronize()
    for buf, v in bufs:  # the guard floats stay as they were
        n = v.numel()
        assert bool((buf[:OFF] == -77.25).all()) and bool((buf[OFF + n:] == -77.25).all())
    dl, dv, rt = (v.cpu().numpy() for _, v in bufs)
    return dl.reshape(S, V), dv, rt.reshape(S, 3)


def _within(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > ULP * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref != 0, err / np.abs(ref), np.where(err > 0, np.inf, 0.0))
    print(f"  {what}: max err / |ref| {rel.max() if rel.size else 0.0:.3g} (bar {ULP:.3g})")
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], ref[bad][:4])


def test_small_cases_cover_every_dedicated_row():
    seen = set()
    for V in VS:
        seen |= set(_kinds_of(V, 3))
        assert len(_kinds_of(V, 1)) == 1 and len(_kinds_of(V, 3)) == 3
        assert set(_kinds_of(V, 130)) == set(KINDS)
    assert seen == set(KINDS)


@pytest.mark.parametrize("V,S", CASES)
def test_single_loss_matches_float64(V, S):
    lg, act, old, adv, value, tg, kinds = _inputs(V, S)
    # the 'ratio exactly 1' rows: old_logp = the kernel's own log-probability.  A first call with old_logp = 0
    # and adv = 1 has ratio = p[a] <= 1, below the upper clip edge, so its actor term is -p[a].
    first = _run(lg, act, np.zeros(S, np.float32), np.ones(S, np.float32), value, tg, S, V, S,
                 torch.zeros(4, dtype=torch.float64, device="cuda"))
    for k, r in kinds.items():
        if k.startswith("one_"):
            old[r] = np.float32(np.log(-np.float64(first[2][r, 0])))
    ref = so.single_loss(lg, act, old, adv, value, tg, CLIP_EPS, ENT_COEF, VF_COEF, S)
    valid = ref["valid"]
    near = so.near_kink(ref["ratio"], CLIP_EPS, valid)
    dedicated = np.zeros(S, bool)
    dedicated[list(kinds.values())] = True
    assert near.sum() <= S // 64 and not (near & dedicated).any(), (near.sum(), S)
    for k, r in kinds.items():  # the dedicated rows are what they claim to be
        if k.startswith("one_"):
            assert abs(ref["ratio"][r] - 1.0) < 1e-6
        elif k.startswith("hi_"):
            assert ref["ratio"][r] > 2.9
        elif k.startswith("lo_"):
            assert ref["ratio"][r] < 0.34
        elif k == "dominant" and V > 1:
            assert ref["terms"][r, 2] == 0.0
    sums_d = torch.from_numpy(INIT.copy()).cuda()
    dl, dv, rt = _run(lg, act, old, adv, value, tg, S, V, S, sums_d)
    print(f"single_loss V={V} S={S} kinds={sorted(kinds)} near-kink rows left out: {int(near.sum())}")
    assert np.isfinite(dl).all() and np.isfinite(dv).all() and np.isfinite(rt).all()
    _within(dl[~near], ref["dlogits"][~near], "dlogits")
    _within(dv, ref["dvalue"], "dvalue")
    _within(rt, ref["terms"], "row terms")
    inv = ~valid
    assert inv.sum() == sum(k in kinds for k in ("inv_neg", "inv_above"))
    assert (dl[inv].view(np.int32) == 0).all() and (dv[inv].view(np.int32) == 0).all()
    assert (rt[inv].view(np.int32) == 0).all()
    sums = sums_d.cpu().numpy()
    np.testing.assert_allclose(sums[:3], INIT[:3] + rt.astype(np.float64).sum(0), rtol=1e-12, atol=0)
    assert sums[3] == INIT[3] + inv.sum()
    if S < 2:
        return
    # micro-batches: two calls over the halves with the whole batch's `minibatch` add up to the same gradient
    two = torch.from_numpy(INIT.copy()).cuda()
    h = S // 2
    parts = [_run(lg[a:b], act[a:b], old[a:b], adv[a:b], value[a:b], tg[a:b], b - a, V, S, two)
             for a, b in ((0, h), (h, S))]
    dl2, dv2, rt2 = (np.concatenate([p[i] for p in parts]) for i in range(3))
    _within(dl2[~near], ref["dlogits"][~near], "dlogits, two halves")
    _within(dv2, ref["dvalue"], "dvalue, two halves")
    assert np.array_equal(dl2.view(np.int32), dl.view(np.int32)) and np.array_equal(rt2.view(np.int32),
                                                                                  rt.view(np.int32))
    np.testing.assert_allclose(two.cpu().numpy(), sums, rtol=1e-12, atol=0)


def test_empty_batch_and_argument_errors():
    from marlsat import _lib

    L = _lib.lib
    st = _lib.stream_ptr()
    f = torch.zeros(8, device="cuda")
    i = torch.zeros(8, dtype=torch.int32, device="cuda")
    s = torch.from_numpy(INIT.copy()).cuda()
    p, ip, sp = f.data_ptr(), i.data_ptr(), s.data_ptr()

    def call(S=2, V=2, mb=2, eps=0.2, ptrs=None):
        a = ptrs if ptrs is not None else [p, ip, p, p, p, p, p, p, p, sp]
        return L.msat_ppo_single_loss(a[0], S, V, a[1], a[2], a[3], a[4], a[5], eps, 0.01, 0.5, mb, a[6], a[7], a[8],
                                      a[9], st)

    assert call(S=0) == 0 and call(S=0, ptrs=[None] * 10) == 0  # no launch, nothing dereferenced
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), INIT)
    for kw, needle in ((dict(S=-1), "S -1"), (dict(V=0), "V 0"), (dict(mb=0), "minibatch 0"),
                       (dict(eps=0.0), "clip_eps"), (dict(eps=-0.1), "clip_eps"), (dict(eps=float("nan")), "clip_eps"),
                       (dict(eps=float("inf")), "clip_eps")):
        assert call(**kw) == -1, kw
        assert needle in L.msat_last_error().decode(), (kw, L.msat_last_error())
    for k in range(10):
        a = [p, ip, p, p, p, p, p, p, p, sp]
        a[k] = None
        assert call(ptrs=a) == -1 and "NULL" in L.msat_last_error().decode(), k
