"""GPU: msat_bc_loss (joint cross-entropy of the BC labels, its gradient, accuracy and the valid / invalid row
counts) against torch float64 on the same fp32 logits.  Bars as tests/test_heads_gpu.py holds msat_ppo_loss to:
dlogits and row terms within 1e-5 of each tensor's largest reference magnitude, sums = the fp64 sum of the
device's own fp32 row terms (1e-12 relative, on top of non-zero initial values), the mean loss within 1e-5
relative (atol 1e-7) of the reference, counts exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (S, A, M): R = 9 is no multiple of the 4 waves per workgroup; W = 2; W = 64 = the lanes; W = 65 crosses the
# lane loop; W = 131 takes three lane rounds; R = 32800 > 4 * 8192 (the grid cap): the grid-stride loop runs
CASES = [(3, 3, 4), (2, 2, 1), (2, 3, 63), (2, 3, 64), (1, 2, 130), (8200, 4, 3)]
INIT = np.array([0.5, 3.0, 7.0, 11.0])
SPECIALS = ("var", "noop", "tie_low", "tie_high", "neg", "above", "masked")
STARTS = [0, 3, 6, 2, 1, 0]  # per case: the first special its rows receive (every case keeps a valid row)


def _sizes(A, M):
    """Agent i owns base + (i < rem) variable slots (the largest owns M); M = 1 has no padded slot."""
    base, rem = (M, 0) if M == 1 else (M - 1, max(1, A // 2))
    return base, rem, np.array([base + (i < rem) for i in range(A)])


def _make(S, A, M, case_no):
    """fp32 logits (R, W) with -inf at padded slots and labels (R,) covering SPECIALS (as many as R rows allow,
    rotated by the case number so that the small cases cover all of them between them)."""
    rng = np.random.default_rng(100 + case_no)
    R, W = S * A, M + 1
    base, rem, n = _sizes(A, M)
    own = np.tile(n, S)  # (R,)
    lg = (3.0 * rng.standard_normal((R, W))).astype(np.float32)
    slot = np.arange(W)[None, :]
    lg[(slot >= own[:, None]) & (slot < M)] = -np.inf
    # default labels: a uniformly drawn own variable or the no-op
    pick = rng.integers(0, own + 1)
    lab = np.where(pick == own, M, pick).astype(np.int32)
    kinds = {}
    order = [SPECIALS[(STARTS[case_no] + k) % len(SPECIALS)] for k in range(len(SPECIALS))]
    rows = list(rng.permutation(R))
    for kind in order:
        if kind == "masked":
            cand = [r for r in rows if own[r] < M]
        else:
            cand = rows
        if not cand:
            continue
        r = cand[0]
        rows.remove(r)
        kinds[kind] = r
        if kind == "var":
            lab[r] = own[r] - 1
        elif kind == "noop":
            lab[r] = M
        elif kind in ("tie_low", "tie_high"):  # two maximal logits: slot 0 and the no-op
            lg[r, 0] = lg[r, M] = np.float32(lg[r][np.isfinite(lg[r])].max() + 1.0)
            lab[r] = 0 if kind == "tie_low" else M
        elif kind == "neg":
            lab[r] = -1
        elif kind == "above":
            lab[r] = M + 1
        elif kind == "masked":
            lab[r] = M - 1
    return lg, lab, kinds


def _reference(lg, lab, A, M, minibatch):
    """float64: dlogits, row terms (R, 2), valid mask."""
    L = torch.from_numpy(lg).double()
    y = torch.from_numpy(lab).long()
    R, W = L.shape
    inside = (y >= 0) & (y <= M)
    yc = y.clamp(0, M)
    valid = inside & torch.isfinite(L.gather(1, yc[:, None])[:, 0])
    lsm = torch.log_softmax(L, -1)
    nll = torch.where(valid, -lsm.gather(1, yc[:, None])[:, 0], torch.zeros(R, dtype=torch.float64))
    onehot = torch.zeros_like(L).scatter_(1, yc[:, None], 1.0)
    d = (torch.softmax(L, -1) - onehot) / (minibatch * A)
    d = torch.where(valid[:, None], d, torch.zeros_like(d))
    mx = L.max(-1, keepdim=True).values
    first = torch.where(L == mx, torch.arange(W)[None, :].expand(R, W), torch.full((R, W), W)).min(-1).values
    correct = (valid & (first == yc)).double()
    return d.numpy(), torch.stack([nll, correct], 1).numpy(), valid.numpy()


def _run(lg_d, lab_d, S, A, M, minibatch, sums_d):
    from marlsat import _lib

    R = S * A
    dl = torch.full((R, M + 1), float("nan"), device="cuda")
    rt = torch.full((2 * R,), float("nan"), device="cuda")
    _lib.check(_lib.lib.msat_bc_loss(lg_d.data_ptr(), S, A, M, lab_d.data_ptr(), minibatch, dl.data_ptr(),
                                     rt.data_ptr(), sums_d.data_ptr(), _lib.stream_ptr()), "msat_bc_loss")
    torch.cuda.synchronize()
    return dl, rt.reshape(R, 2)


@pytest.fixture(scope="module")
def cases():
    """Inputs and float64 references, computed once per case and left unchanged."""
    out = {}
    for no, (S, A, M) in enumerate(CASES):
        lg, lab, kinds = _make(S, A, M, no)
        out[(S, A, M)] = (lg, lab, kinds) + _reference(lg, lab, A, M, S)
    return out


def test_cases_cover_every_label_kind(cases):
    seen = set()
    for lg, lab, kinds, *_ in cases.values():
        seen |= set(kinds)
    assert seen == set(SPECIALS)
    assert set(cases[(8200, 4, 3)][2]) == set(SPECIALS) == set(cases[(3, 3, 4)][2])


@pytest.mark.parametrize("S,A,M", CASES)
def test_bc_loss_matches_float64(S, A, M, cases):
    lg, lab, kinds, d_ref, rt_ref, valid = cases[(S, A, M)]
    R = S * A
    lg_d, lab_d = torch.from_numpy(lg).cuda(), torch.from_numpy(lab).cuda()
    sums_d = torch.from_numpy(INIT.copy()).cuda()
    dl, rt = _run(lg_d, lab_d, S, A, M, S, sums_d)
    dl_h, rt_h, sums = dl.cpu().numpy(), rt.cpu().numpy(), sums_d.cpu().numpy()
    assert np.isfinite(dl_h).all() and np.isfinite(rt_h).all()
    e_d = np.abs(dl_h - d_ref).max() / np.abs(d_ref).max()
    e_n = np.abs(rt_h[:, 0] - rt_ref[:, 0]).max() / np.abs(rt_ref[:, 0]).max()
    print(f"bc_loss S={S} A={A} M={M}: dlogits err / max|ref| {e_d:.3g}, nll err / max|ref| {e_n:.3g}")
    assert e_d <= 1e-5 and e_n <= 1e-5
    assert np.abs(rt_h[:, 1] - rt_ref[:, 1]).max() <= 1e-5 * max(rt_ref[:, 1].max(), 1e-12)
    # invalid rows: nothing but zeros, bitwise; -inf slots of valid rows: zero gradient
    inv = torch.from_numpy(~valid).cuda()
    assert int(inv.sum()) == sum(k in kinds for k in ("neg", "above", "masked"))
    assert bool((dl[inv].view(torch.int32) == 0).all()) and bool((rt[inv].view(torch.int32) == 0).all())
    assert (dl_h[~np.isfinite(lg)] == 0).all()
    # the tie rows: accuracy follows the lowest index
    if "tie_low" in kinds:
        assert rt_h[kinds["tie_low"], 1] == 1.0
    if "tie_high" in kinds:
        assert rt_h[kinds["tie_high"], 1] == 0.0
    # sums: the device's own row terms in fp64, on top of the caller's values; exact counts
    own = INIT[:2] + rt_h.astype(np.float64).sum(0)
    np.testing.assert_allclose(sums[:2], own, rtol=1e-12, atol=0)
    assert sums[2] == INIT[2] + valid.sum() and sums[3] == INIT[3] + (~valid).sum()
    assert sums[1] - INIT[1] == rt_ref[:, 1].sum()
    np.testing.assert_allclose((sums[0] - INIT[0]) / R, rt_ref[:, 0].sum() / R, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("S,A,M", [c for c in CASES if c[0] >= 2])
def test_two_half_calls_equal_one_call(S, A, M, cases):
    """Micro-batches: two calls over the two halves with the whole batch's ``minibatch`` write the same dlogits
    rows (bitwise) and accumulate the same sums."""
    lg, lab, *_ = cases[(S, A, M)]
    lg_d, lab_d = torch.from_numpy(lg).cuda(), torch.from_numpy(lab).cuda()
    one = torch.from_numpy(INIT.copy()).cuda()
    dl, rt = _run(lg_d, lab_d, S, A, M, S, one)
    two = torch.from_numpy(INIT.copy()).cuda()
    h = S // 2
    lo = _run(lg_d[:h * A].contiguous(), lab_d[:h * A].contiguous(), h, A, M, S, two)
    hi = _run(lg_d[h * A:].contiguous(), lab_d[h * A:].contiguous(), S - h, A, M, S, two)
    assert torch.equal(torch.cat([lo[0], hi[0]]), dl) and torch.equal(torch.cat([lo[1], hi[1]]), rt)
    np.testing.assert_allclose(two.cpu().numpy(), one.cpu().numpy(), rtol=1e-12, atol=0)
