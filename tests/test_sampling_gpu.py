"""GPU: categorical sampling (distrax.Categorical sample / log_prob, learner:397-403) by the
Gumbel-max kernel -- empirical frequencies vs softmax, masked (-inf) actions never drawn,
log-probs exact, greedy = first argmax (jnp.argmax ties), counter-based reproducibility."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sample(logits, greedy, seed, counter):
    from marlsat import _lib

    R, W = logits.shape
    act = torch.empty(R, dtype=torch.int32, device="cuda")
    lp = torch.empty(R, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib.msat_sample_actions(logits.data_ptr(), R, W, 1 if greedy else 0, seed, counter,
                                            act.data_ptr(), lp.data_ptr(), _lib.stream_ptr()), "sample")
    torch.cuda.synchronize()
    return act, lp


@pytest.mark.parametrize("W", [2, 9, 11, 70])
def test_gumbel_sampling_statistics(W):
    R = 200000
    g = torch.Generator(device="cuda").manual_seed(W)
    row = torch.randn(W, device="cuda", generator=g) * 1.5
    masked = W // 2 if W > 2 else -1  # a masked action (W = 2 keeps both: two outcomes needed below)
    if masked >= 0:
        row[masked] = float("-inf")
    logits = row.expand(R, W).contiguous()
    act, lp = _sample(logits, False, 1234, 7)
    a = act.long().cpu()
    assert int(a.min()) >= 0 and int(a.max()) < W and not bool((a == masked).any())
    p = torch.softmax(row.double().cpu(), 0)
    freq = torch.bincount(a, minlength=W).double() / R
    sigma = (p * (1 - p) / R).sqrt()
    assert bool(((freq - p).abs() <= 5 * sigma + 1e-12).all()), (freq, p)
    ref_lp = torch.log_softmax(row.double(), 0)[act.long()].float()
    assert torch.allclose(lp, ref_lp, rtol=0, atol=2e-6)
    act2, _ = _sample(logits, False, 1234, 7)
    act3, _ = _sample(logits, False, 1234, 8)
    assert torch.equal(act, act2) and not torch.equal(act, act3)


def test_greedy_argmax_first_tie_and_masks():
    lg = torch.tensor([[0.5, 2.0, 2.0, -1.0], [float("-inf"), -3.0, -3.0, float("-inf")],
                       [float("-inf")] * 3 + [0.0], [7.0, 7.0, 7.0, 7.0]], device="cuda")
    act, lp = _sample(lg, True, 0, 0)
    assert act.tolist() == [1, 1, 3, 0]
    assert torch.allclose(lp, torch.log_softmax(lg.double(), 1).gather(1, act.long()[:, None])[:, 0].float())


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("R", [1, 2, 3, 5])  # one to four waves of the first block busy, then a second block
@pytest.mark.parametrize("W", [1, 64, 65, 129])  # one lane, a full wave, a second and a third trip of the j += 64 loops
def test_row_widths_and_row_counts(W, R, greedy):
    rng = np.random.default_rng(W * 10 + R)
    lg = (rng.standard_normal((R, W)) * 2).astype(np.float32)
    if W > 1:
        lg[rng.random((R, W)) < 0.3] = float("-inf")
        lg[np.arange(R), rng.integers(0, W, R)] = 0.25  # a live entry in every row
    logits = torch.from_numpy(lg).cuda()
    act, lp = _sample(logits, greedy, 99, 5)
    a = act.long().cpu()
    assert int(a.min()) >= 0 and int(a.max()) < W
    assert bool(torch.isfinite(logits.cpu().gather(1, a[:, None])).all())  # never a masked action
    ref = torch.log_softmax(torch.from_numpy(lg).double(), 1)
    assert torch.allclose(lp.cpu().double(), ref.gather(1, a[:, None])[:, 0], rtol=0, atol=2e-6)
    if greedy:
        assert a.tolist() == np.argmax(lg, 1).tolist()  # the first maximum


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("W", [2, 11])
def test_row_without_a_finite_logit(W, greedy):
    """A mode-1 padded variable slot (W = 2), and the same at W = 11: some action inside the row, and
    log-prob exactly 0 (the PPO loss skips the slot; a NaN here would poison the joint ratio)."""
    lg = torch.randn(3, W, device="cuda")
    lg[1] = float("-inf")
    act, lp = _sample(lg, greedy, 5, 1)
    assert 0 <= int(act[1]) < W
    assert float(lp[1]) == 0.0 and not bool(torch.signbit(lp[1]))
    assert bool(torch.isfinite(lp).all()) and int(act.min()) >= 0 and int(act.max()) < W


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("greedy", [True, False])
def test_rows_past_the_grid_cap_equal_the_two_pieces(greedy):
    """R = 32773, W = 3: five rows past the launch's cap of 8192 workgroups x 4 rows, so the first two workgroups
    take a second trip of the row loop (one of them with a single live wave).  The whole-batch call is bitwise the
    concatenation of the rows [0, 32768) -- one trip exactly -- and [32768, R) sampled as a piece of their own:
    msat_sample_actions_from with row_offset 32768 for the sampled draw; the greedy pick draws no noise and takes
    no row offset (msat_sample_actions_from has no greedy form), so its pieces are plain greedy calls, and it is
    also the first maximum of every row."""
    from marlsat import _lib

    R, W, CUT, SEED, COUNTER = 32773, 3, 8192 * 4, 0x1234_5678_9ABC_DEF1, (7 << 32) + 5
    rng = np.random.default_rng(R)
    lg = (rng.standard_normal((R, W)) * 2).astype(np.float32)
    lg[rng.random((R, W)) < 0.3] = -np.inf
    lg[np.arange(R), rng.integers(0, W, R)] = 0.25  # a live entry in every row ...
    lg[CUT + 1] = -np.inf  # ... but one of the second trip's: log-prob 0
    lg[CUT + 2] = 0.5  # and a three-way tie there

    def call(fn, rows, *mid):
        n = rows.shape[0]
        act = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        lp = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(getattr(_lib.lib, fn)(rows.data_ptr(), n, W, *mid, SEED, COUNTER, act.data_ptr(), lp.data_ptr(),
                                         _lib.stream_ptr()), fn)
        torch.cuda.synchronize()
        return act.cpu().numpy(), lp.cpu().numpy()

    d = torch.from_numpy(lg).cuda()
    head, tail = d[:CUT].contiguous(), d[CUT:].contiguous()
    whole = call("msat_sample_actions", d, 1 if greedy else 0)
    if greedy:
        pieces = [call("msat_sample_actions", head, 1), call("msat_sample_actions", tail, 1)]
        assert np.array_equal(whole[0], np.argmax(lg, 1))
    else:
        pieces = [call("msat_sample_actions_from", head, 0, 1.0), call("msat_sample_actions_from", tail, CUT, 1.0)]
        assert _same_bits(call("msat_sample_actions_from", d, 0, 1.0), whole)
    cat = tuple(np.concatenate([p[i] for p in pieces]) for i in range(2))
    assert _same_bits(cat, whole), np.flatnonzero(cat[0] != whole[0])[:8]
    a, lp = whole
    assert a.min() >= 0 and a.max() < W and lp[CUT + 1] == 0.0
    live = np.isfinite(lg).any(1)
    assert np.isfinite(lg[live, a[live]]).all()  # never a masked action
    ref = torch.log_softmax(torch.from_numpy(lg[live]).double(), 1).numpy()
    assert np.abs(lp[live] - ref[np.arange(live.sum()), a[live]]).max() <= 2e-6  # this file's bar for log-probs
