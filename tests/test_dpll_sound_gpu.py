"""GPU: the verdicts of msat_dpll held against the independent host solver (tests/dpll_independent.py), not against
the replay: on the uf20 / uf50 / uf100 pools of dpll_cases.SOUND as single searches, under 16 cubes, through
decide_pool, and on four meaning-preserving rewrites of the uf50 pool.  Every model goes through the env's clause
check.  The independent verdicts are computed once per session (dpll_cases.shared_verdicts); the pools' mix and the
agreement of the solver's two branching rules are asserted before anything is compared."""
import numpy as np
import pytest

from dpll_cases import SOUND, rewrites, satisfied, sound_pool, sound_verdicts
from dpll_replay import SAT, UNKNOWN, combine
from test_dpll_gpu import BIG, device_run, verify_models

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(SOUND))
def test_kernel_status_equals_the_independent_verdict(name):
    truth = sound_verdicts(name)
    pool, V, N = sound_pool(name)
    st, x, nodes, _, _ = device_run(pool, V, np.arange(N))
    assert (st != UNKNOWN).all() and (nodes < BIG).all()
    assert np.array_equal(st, truth), np.flatnonzero(st != truth)
    verify_models(pool, V, np.arange(N), st, x)


@pytest.mark.parametrize("name", sorted(SOUND))
def test_sixteen_cubes_combine_to_the_independent_verdict(name):
    truth = sound_verdicts(name)
    pool, V, N = sound_pool(name)
    pidx, cubes = np.repeat(np.arange(N), 16), np.tile(np.arange(16), N)
    st, x, _, _, _ = device_run(pool, V, pidx, cubes, 4)
    assert (st != UNKNOWN).all()
    verdict = np.array([combine(st[n * 16:(n + 1) * 16]) for n in range(N)])
    assert np.array_equal(verdict, truth), np.flatnonzero(verdict != truth)
    verify_models(pool, V, pidx, st, x)


def test_decide_pool_against_the_independent_verdict():
    from marlsat import SATEnv
    from marlsat.solvers import decide_pool

    truth = sound_verdicts("uf50")
    pool, V, N = sound_pool("uf50")
    env = SATEnv(V, pool.shape[1], max_steps=1, vars_per_agent=10)
    got = decide_pool(env.make_pool(pool))  # the defaults: 4096 nodes, 16 cubes from round 1 on
    assert np.array_equal(got["status"], truth), np.flatnonzero(got["status"] != truth)
    verify_models(pool, V, np.arange(N), got["status"], got["solution"])
    # budgets that leave some instances open: a decided status is the verdict, the rest are UNKNOWN, never wrong
    got = decide_pool(env.make_pool(pool), max_nodes=8, cube_bits=4, max_rounds=3)
    decided = got["status"] != UNKNOWN
    assert decided.any() and np.array_equal(got["status"][decided], truth[decided])
    assert set(got["status"][~decided].tolist()) <= {UNKNOWN}
    verify_models(pool, V, np.arange(N), got["status"], got["solution"])
    # one round of 8 nodes decides only the shortest searches, and those rightly
    got = decide_pool(env.make_pool(pool), max_nodes=8, cube_bits=4, max_rounds=1)
    decided = got["status"] != UNKNOWN
    assert not decided.all() and np.array_equal(got["status"][decided], truth[decided])


@pytest.mark.parametrize("kind", ["renamed", "polarity", "permuted", "duplicated"])
def test_rewritten_instances_keep_their_verdict(kind):
    """Renaming, polarity flips, row and slot permutations and duplicated clauses leave satisfiability as it was (by
    construction); the kernel's status on the rewrite is the independent verdict of the original."""
    truth = sound_verdicts("uf50")
    pool, V, N = sound_pool("uf50")
    new, flip = rewrites(pool, V, 50)[kind]
    st, x, _, _, _ = device_run(new, V, np.arange(N))
    assert np.array_equal(st, truth), np.flatnonzero(st != truth)
    verify_models(new, V, np.arange(N), st, x)
    if kind == "permuted":  # no step of the algorithm depends on the order of the rows or of a row's slots
        same = device_run(pool, V, np.arange(N))
        assert all(np.array_equal(a, b) for a, b in zip((st, x), same[:2]))
    if flip is not None:
        for n in np.flatnonzero(truth == SAT):
            assert satisfied(x[n] ^ flip[n], pool[n]).all(), n  # mapped back: a model of the original clauses
