"""GPU: Gumbel-max sampling at a temperature (msat_sample_actions_t, include/marlsat_net.h).

The yardstick is the existing kernel on identical inputs: msat_sample_actions_t(logits, inv_t) must give, bit for
bit, the action and the log-prob of msat_sample_actions(greedy = 0) on the logits multiplied by inv_t in fp32 on
the host, so no tolerance appears.  Shapes: W in {1, 2, 11, 64, 65, 129} (one lane, a full wave, a second and a
third trip of the lane loops) x R in {1, 5} (one wave; a second workgroup), -inf masks and an all -inf row, inverse
temperatures 1.0, 0.5, 2.0 and 1 / 0.3.  msat_sample_actions_from, the same kernel for a piece of a larger batch,
is held to: pieces of any size sample what the whole batch samples.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, COUNTER = 0x1234_5678_9ABC_DEF1, (7 << 32) + 5  # both Philox counter words and both key words in use


def _call(fn, logits, *mid, seed=SEED, counter=COUNTER):
    from marlsat import _lib

    R, W = logits.shape
    act = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((R,), float("nan"), dtype=torch.float32, device="cuda")
    rc = getattr(_lib.lib, fn)(logits.data_ptr(), R, W, *mid, seed, counter, act.data_ptr(), lp.data_ptr(),
                               _lib.stream_ptr())
    _lib.check(rc, fn)
    torch.cuda.synchronize()
    return act.cpu().numpy(), lp.cpu().numpy()


def _logits(R, W, seed):
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((R, W)) * 3).astype(np.float32)
    if W > 1:
        lg[rng.random((R, W)) < 0.3] = -np.inf
        lg[np.arange(R), rng.integers(0, W, R)] = 0.25  # a live entry in every row ...
    if R > 1:
        lg[R // 2] = -np.inf  # ... but one: a row with no finite logit (a mode-1 padded slot)
    return lg


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("inv_t", [1.0, 0.5, 2.0, 1 / 0.3])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("W", [1, 2, 11, 64, 65, 129])
def test_tempered_equals_plain_kernel_on_premultiplied_logits(W, R, inv_t):
    lg = _logits(R, W, W * 10 + R)
    it32 = np.float32(inv_t)  # what the C-ABI's float argument holds
    got = _call("msat_sample_actions_t", torch.from_numpy(lg).cuda(), float(it32))
    pre = (lg * it32).astype(np.float32)  # one fp32 rounding per logit, on the host
    want = _call("msat_sample_actions", torch.from_numpy(pre).cuda(), 0)
    assert _same_bits(got, want), (got, want)
    if R > 1:  # the row with no finite logit: log-prob 0
        assert got[1][R // 2] == 0.0 and not np.isfinite(pre[R // 2]).any()
    live = np.isfinite(pre).any(axis=1)
    assert np.isfinite(pre[live, got[0][live]]).all()  # never a masked action
    if inv_t == 1.0:
        assert _same_bits(got, _call("msat_sample_actions", torch.from_numpy(lg).cuda(), 0))


@pytest.mark.parametrize("inv_t", [0.0, -2.0, float("nan"), float("inf"), float("-inf")])
def test_bad_inverse_temperature_is_ebadarg(inv_t):
    from marlsat import _lib

    lg = torch.zeros((2, 4), device="cuda")
    act = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    lp = torch.zeros(2, device="cuda")
    rc = _lib.lib.msat_sample_actions_t(lg.data_ptr(), 2, 4, inv_t, 1, 2, act.data_ptr(), lp.data_ptr(),
                                        _lib.stream_ptr())
    assert rc == -1 and "inv_temperature" in _lib.lib.msat_last_error().decode()
    torch.cuda.synchronize()
    assert act.tolist() == [-7, -7]  # nothing was launched


@pytest.mark.parametrize("inv_t", [1.0, 1 / 0.7])
def test_pieces_of_a_batch_sample_what_the_whole_batch_samples(inv_t):
    R, W = 9, 11
    lg = torch.from_numpy(_logits(R, W, 3)).cuda()
    whole = _call("msat_sample_actions_t", lg, inv_t)
    assert _same_bits(_call("msat_sample_actions_from", lg, 0, inv_t), whole)
    for cut in (1, 4, 8):
        a = _call("msat_sample_actions_from", lg[:cut].contiguous(), 0, inv_t)
        b = _call("msat_sample_actions_from", lg[cut:].contiguous(), cut, inv_t)
        assert _same_bits((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), whole), cut
    shifted = _call("msat_sample_actions_from", lg, 1, inv_t)
    assert not np.array_equal(shifted[0], whole[0])  # another row offset: other streams


def test_learner_policy_temperature_takes_the_new_entry_point():
    """learner.policy(temperature=t) samples msat_sample_actions_t(logits, 1 / t) with the old call's counters;
    temperature 1.0 and greedy calls are the old calls (same outputs as without the keyword)."""
    from marlsat import SATEnv, _lib
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.random import Key
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    env = SATEnv(20, 91, max_steps=8, vars_per_agent=10)
    pool = env.make_pool(generate_problem_pool(20, 91, 5, size_id=0))
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, 20, device="cuda", seed=4)
    lr = MAPPOLearner(dict(NUM_ENVS=5, NUM_STEPS=1, MINIBATCH_SIZE=5), env, net, pool)
    _, st = env.reset_from_pool(pool, 5, Key(3, 0), problem_idx=np.arange(5), with_obs=False)
    key = Key(11, 2)
    a0, l0, _ = lr.policy(st, key, critic=False)
    a1, l1, _ = lr.policy(st, key, critic=False, temperature=1.0)
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
    g0, _, _ = lr.policy(st, key, greedy=True, critic=False)
    g1, _, _ = lr.policy(st, key, greedy=True, critic=False, temperature=0.5)
    assert torch.equal(g0, g1)
    at, lt, _ = lr.policy(st, key, critic=False, temperature=0.5)
    logits, _, _ = net.forward(lr._batch(st.problem_idx, st.variable_assignments), critic=False)
    W = env.max_vars_per_agent + 1
    want = _call("msat_sample_actions_t", logits.reshape(-1, W).contiguous(), 2.0, seed=key.seed,
                 counter=key.counter << 16)
    assert np.array_equal(at.cpu().numpy().reshape(-1), want[0])
    assert np.array_equal(lt.cpu().numpy().reshape(-1).view(np.uint32), want[1].view(np.uint32))
    with pytest.raises(ValueError, match="temperature"):
        lr.policy(st, key, critic=False, temperature=0.0)
