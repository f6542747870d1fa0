"""CPU: the verdicts of the DPLL replay (tests/dpll_replay.py, the yardstick of the GPU tests) held against a solver
that shares neither code nor search shape with it (tests/dpll_independent.py), past the 14 variables brute force
reaches.  First the independent solver's own soundness (brute force for V <= 14, two branching rules that must
agree, every model checked), then the replay on the uf20 / uf50 / uf100 pools of dpll_cases.SOUND as single
searches, under 16 cubes and on four meaning-preserving rewrites, and the deep-backtracking instances whose counts
are derived by hand in dpll_cases.chain / chain_two_pops."""
import numpy as np
import pytest

import dpll_independent as indep
from dpll_cases import (HAND_MADE, SOUND, brute_force_sat, chain, chain_two_pops, hand_made, pigeonhole, random_pool,
                        rewrites, satisfied, shared_replay, sound_pool, sound_verdicts)
from dpll_replay import SAT, UNKNOWN, UNSAT, combine, replay_one

BIG = 200000
# every random pool of tests/test_dpll_cpu.py with V <= 14
SMALL = [(12, 80, 6, 1), (14, 60, 10, 2), (7, 63, 4, 3), (7, 64, 4, 4), (7, 65, 4, 5), (10, 43, 12, 6), (5, 20, 8, 7),
         (3, 6, 8, 8), (12, 52, 3, 21), (12, 52, 4, 22), (7, 30, 3, 9), (12, 56, 5, 32)]


def sound_replay(name):
    pool, V, N = sound_pool(name)
    return shared_replay(("sound", name), pool, V, np.arange(N), max_nodes=BIG)


# ---------------------------------------------------- the independent solver's own soundness ----
def test_statuses_are_the_replay_s_codes():
    assert (indep.SAT, indep.UNSAT) == (SAT, UNSAT)


@pytest.mark.parametrize("rule", indep.RULES)
@pytest.mark.parametrize("V,C,N,seed", SMALL)
def test_independent_equals_brute_force_on_random_pools(V, C, N, seed, rule):
    pool = random_pool(V, C, N, seed)
    for n in range(N):
        status, x = indep.decide(pool[n], V, rule)  # decide() checks the model
        assert status == (SAT if brute_force_sat(pool[n], V) else UNSAT), n
        assert (x is None) == (status == UNSAT)


@pytest.mark.parametrize("rule", indep.RULES)
def test_independent_equals_brute_force_on_hand_made_cases(rule):
    for name in sorted(HAND_MADE):
        pool, V, status, _ = hand_made(name)
        assert indep.decide(pool[0], V, rule)[0] == status == (SAT if brute_force_sat(pool[0], V) else UNSAT), name
    pool, V = pigeonhole(4, 3)
    assert indep.decide(pool[0], V, rule)[0] == UNSAT
    assert indep.decide(np.zeros((2, 3), np.int32), 3, rule)[0] == UNSAT  # the empty clause
    assert indep.decide(np.array([[1, -1, 0], [2, -2, 2]], np.int32), 2, rule)[0] == SAT  # tautologies only


def test_normalise_rewrites_by_meaning():
    got = indep.normalise(np.array([[1, 1, -2], [3, -3, 4], [0, 5, -6], [0, 0, 7], [0, 0, 0], [9, 9, 9], [-9, 0, -9],
                                    [-2, 1, 1], [7, 0, 0]], np.int32))
    assert got.tolist() == [[0, 0, 0], [-9, 0, 0], [7, 0, 0], [9, 0, 0], [1, -2, 0], [5, -6, 0]]


@pytest.mark.parametrize("name", sorted(SOUND))
def test_pools_hold_both_verdicts_and_the_two_rules_agree(name):
    truth = sound_verdicts(name)  # asserts both
    _, _, N = sound_pool(name)
    assert truth.shape == (N,) and set(truth.tolist()) == {SAT, UNSAT}
    if name == "uf20":
        assert ((truth == SAT).sum(), (truth == UNSAT).sum()) == (8, 8)
    if name == "uf50":
        assert ((truth == SAT).sum(), (truth == UNSAT).sum()) == (17, 15)


# ----------------------------------------------------------------- the replay's verdicts ----
@pytest.mark.parametrize("name", sorted(SOUND))
def test_replay_status_equals_the_independent_verdict(name):
    truth = sound_verdicts(name)
    pool, V, N = sound_pool(name)
    status, x = sound_replay(name)[:2]
    assert (status != UNKNOWN).all()
    assert np.array_equal(status, truth), np.flatnonzero(status != truth)
    for n in range(N):
        assert satisfied(x[n], pool[n]).all() if status[n] == SAT else not x[n].any()


def test_uf50_pool_backtracks_deeper_than_brute_force_reaches():
    """The uf50 pool exercises what V <= 14 does not: one conflict that pops three or more closed entries, and a flip
    at level 6 or deeper."""
    pool, V, N = sound_pool("uf50")
    ref = sound_replay("uf50")
    pops = flip = level = 0
    for n in range(N):
        stats = {}
        got = replay_one(pool[n], V, 0, 0, BIG, stats)
        assert got[0] == ref[0][n] and got[2] == ref[2][n]  # the outputs do not depend on stats
        assert len(stats["flips"]) == got[3] - (got[0] == UNSAT)  # every conflict but an UNSAT search's last flips
        pops, flip, level = max(pops, stats["max_pops"]), max(flip, stats["deepest_flip"]), max(level,
                                                                                               stats["max_level"])
    print(f"uf50: most pops {pops}, deepest flip {flip}, deepest level {level}")
    assert pops >= 3 and flip >= 6 and level >= flip


@pytest.mark.parametrize("name", ["uf20", "uf50"])
def test_sixteen_cubes_combine_to_the_independent_verdict(name):
    truth = sound_verdicts(name)
    pool, V, N = sound_pool(name)
    N = min(N, 16)
    st, x, _, _, _ = shared_replay(("sound16", name), pool, V, np.repeat(np.arange(N), 16),
                                   np.tile(np.arange(16), N), 4, BIG)
    assert (st != UNKNOWN).all()
    for n in range(N):
        assert combine(st[n * 16:(n + 1) * 16]) == truth[n], n
    for s in np.flatnonzero(st == SAT):
        assert satisfied(x[s], pool[s // 16]).all()


@pytest.mark.parametrize("kind", ["renamed", "polarity", "permuted", "duplicated"])
def test_replay_on_rewritten_instances(kind):
    """Satisfiability survives the rewrite (checked with the independent solver too); the search does not, except
    under the permutation, which must leave all five outputs as they were."""
    truth = sound_verdicts("uf50")
    pool, V, N = sound_pool("uf50")
    new, flip = rewrites(pool, V, 50)[kind]
    assert new.shape[0] == N and not np.array_equal(new[:, :pool.shape[1]], pool)
    assert np.array_equal(indep.verdicts(new, V, "occur"), truth)
    ref = shared_replay(("rewrite", kind), new, V, np.arange(N), max_nodes=BIG)
    assert np.array_equal(ref[0], truth), np.flatnonzero(ref[0] != truth)
    if kind == "permuted":  # no step of the header depends on the order of the rows or of a row's slots
        assert all(np.array_equal(a, b) for a, b in zip(ref, sound_replay("uf50")))
    else:
        assert not np.array_equal(ref[2], sound_replay("uf50")[2])  # other searches
    if flip is not None:
        for n in np.flatnonzero(truth == SAT):
            assert satisfied(ref[1][n] ^ flip[n], pool[n]).all(), n  # mapped back: a model of the original


# ------------------------------------------------------------------- levels past 255 ----
def test_chain_flips_at_level_300():
    cl, V = chain(300)
    assert cl.shape == (1, 601, 3) and V == 601
    stats = {}
    status, x, nodes, conflicts, props = replay_one(cl[0], V, 0, 0, BIG, stats)
    assert (status, nodes, conflicts, props) == (SAT, 301, 1, 1)
    want = np.zeros(V, np.uint8)
    want[0:597:2] = 1  # the odd variables below p
    want[599] = 1      # q; p (index 598) and r (600) stay 0
    assert np.array_equal(x, want) and satisfied(x, cl[0]).all()
    assert stats == {"max_level": 300, "deepest_flip": 300, "max_pops": 0, "flips": [(300, 300)]}
    assert indep.decide(cl[0], V)[0] == SAT
    # 30 closed levels: the all-ones cube is the same path; cube 0 sets the even variables of the first 30 pairs
    assert replay_one(cl[0], V, 2 ** 30 - 1, 30, BIG)[2:] == (301, 1, 1)
    status, x0, nodes, conflicts, props = replay_one(cl[0], V, 0, 30, BIG, stats)
    assert (status, nodes, conflicts, props) == (SAT, 301, 1, 31) and stats["deepest_flip"] == 300
    want[0:60:2], want[1:60:2] = 0, 1
    assert np.array_equal(x0, want)


def test_chain_pops_level_300_and_flips_299():
    cl, V = chain_two_pops(298)
    assert cl.shape == (1, 1198, 3) and V == 601
    stats = {}
    status, x, nodes, conflicts, props = replay_one(cl[0], V, 0, 0, BIG, stats)
    assert (status, nodes, conflicts, props) == (SAT, 302, 2, 1)
    assert stats == {"max_level": 300, "deepest_flip": 300, "max_pops": 1, "flips": [(300, 300), (300, 299)]}
    want = np.zeros(V, np.uint8)
    want[0:596:2] = 1  # the odd variables of the pairs
    want[597] = 1      # a2; a, b, c, d stay 0
    assert np.array_equal(x, want) and satisfied(x, cl[0]).all()
    assert indep.decide(cl[0], V, "occur")[0] == SAT
