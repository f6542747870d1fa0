"""GPU: msat_pool_generate (include/marlsat.h) against tests/pool_generate_replay.py, the NumPy restatement of the
header's draw on oracle.rng.philox4x32_10: clauses, planted assignments and attempts bit for bit, the retry and the
exhausted path included; prefix stability, two calls agreeing, rejection off; ProblemPool.generate on top of it."""
import functools

import numpy as np
import pytest
import torch

import pool_generate_replay as replay

pytestmark = pytest.mark.gpu

SEED, COUNTER = 77, (3 << 32) | 5


@functools.lru_cache(maxsize=None)
def _replay(N, V, C, K, reject=True, max_attempts=64):
    out = replay.generate(N, V, C, K, SEED, COUNTER, reject, max_attempts)
    for a in out:
        a.setflags(write=False)
    return out


def _device(N, V, C, K, reject=True, max_attempts=64, seed=SEED, counter=COUNTER):
    from marlsat import _lib

    cl = torch.full((N, C, K), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    pl = torch.full((N, V), 0xEE, dtype=torch.uint8, device="cuda")
    at = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.msat_pool_generate(N, V, C, K, seed, counter, int(reject), max_attempts, cl.data_ptr(),
                                           pl.data_ptr(), at.data_ptr(), _lib.stream_ptr(cl.device)),
               "msat_pool_generate")
    return cl.cpu().numpy(), pl.cpu().numpy(), at.cpu().numpy()


def _same(got, want):
    for what, g, w in zip(("clauses", "planted", "attempts"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=what)


@pytest.mark.parametrize("N,V,C,K", [(64, 20, 20, 3), (64, 12, 20, 2), (4, 129, 300, 3), (4, 200, 860, 3),
                                     (2, 257, 300, 3), (2, 600, 1800, 3)])
def test_generator_equals_replay_bit_for_bit(N, V, C, K):
    want = _replay(N, V, C, K)
    if (V, C) in ((20, 20), (12, 20)):
        # the retry path must be exercised: a uniform-subset simulation gives 57 % / 29 % of instances at least
        # one retry; asserted on the replay first, so that a failure below names the kernel
        assert (want[2] > 0).sum() >= N // 4 and (want[2] >= 0).all()
    got = _device(N, V, C, K)
    _same(got, want)
    if (V, C) in ((20, 20), (12, 20)):
        assert (got[2] > 0).sum() >= N // 4 and (got[2] >= 0).all()


def test_exhausted_attempts_are_minus_one_and_generate_raises():
    """(6, 6, 1) with four attempts: six unit clauses rarely cover six variables, so most rows exhaust their
    attempts; the rows that must are taken from the replay, and the outputs hold the last attempt."""
    from marlsat import ProblemPool

    want = _replay(32, 6, 6, 1, True, 4)
    assert (want[2] == -1).any()
    _same(_device(32, 6, 6, 1, True, 4), want)
    with pytest.raises(RuntimeError, match="4 attempts"):
        ProblemPool.generate((6, 6, 1), 32, 5, max_attempts=4)


def test_rejection_off_is_attempt_zero():
    got = _device(64, 20, 20, 3, reject=False)
    assert (got[2] == 0).all()
    _same(got, _replay(64, 20, 20, 3, False))


def test_prefix_stability_and_repeatability():
    a = _device(64, 20, 20, 3)
    b = _device(128, 20, 20, 3)
    _same(tuple(x[:64] for x in b), a)
    _same(_device(128, 20, 20, 3), b)
    other = _device(64, 20, 20, 3, counter=COUNTER + 1)
    assert not np.array_equal(other[0], a[0])
    other = _device(64, 20, 20, 3, seed=SEED + (1 << 32))  # the high half of the seed is part of the key
    assert not np.array_equal(other[0], a[0])


def test_problem_pool_generate():
    from marlsat import ProblemPool, SATEnv
    from marlsat.random import Key

    env = SATEnv(20, 91, max_steps=8, vars_per_agent=10)
    pool = ProblemPool.generate(env, 8, Key(SEED, COUNTER))
    want = replay.generate(8, 20, 91, 3, SEED, COUNTER)
    np.testing.assert_array_equal(pool.clauses.cpu().numpy(), want[0])
    np.testing.assert_array_equal(pool.planted.cpu().numpy(), want[1])
    np.testing.assert_array_equal(pool.attempts.cpu().numpy(), want[2])
    assert (pool.num_problems, pool.num_clauses, pool.clause_width, pool.num_vars) == (8, 91, 3, 20)
    # everything behind the pool works unchanged: the planted assignment solves its instance in the env
    for n in range(8):
        _, nun = env._calculate_satisfaction_explicit(pool.planted[n].cpu().numpy(), pool.clauses[n].cpu().numpy())
        assert int(nun) == 0
    assert pool.static_var_features().shape == (8, 20, 3)
    two = ProblemPool.generate((12, 20, 2), 4, 3)
    assert tuple(two.clauses.shape) == (4, 20, 2) and (two.attempts >= 0).all()
    with pytest.raises(RuntimeError, match="clause_width"):
        ProblemPool.generate((12, 20, 4), 4, 3)
    with pytest.raises(RuntimeError, match="never be accepted"):
        ProblemPool.generate((20, 6, 3), 4, 3)
