"""GPU: msat_dpll at its own edges.  Every case goes through test_dpll_gpu.check_case: all five outputs bitwise
against the host replay, guard rows, the env's clause check on every model.  Where V <= 14 the status is also held
against brute force, and where it is cheap against the independent solver (tests/dpll_independent.py).

The edges: the trip counts of the 64-wide variable loops (V around 64 and 128), the clause passes up to the 64 KiB
LDS bound 8 C + 14 V + ceil16(V), search levels past 255 (the chain instances of dpll_cases, derived by hand), 30 cube
bits, 8192 samples, the ends of the node budget, the irregular pools of tests/irregular_pools.py, and the larger of
these again under libmarlsat_debug.so, whose index checks then cover LDS offsets at the bound and levels and stack
entries past 255."""
import ctypes
import os

import numpy as np
import pytest

import dpll_independent as indep
import irregular_pools
from dpll_cases import (brute_force_sat, chain, chain_two_pops, hand_made, random_pool, shared_replay, sound_pool,
                        sound_verdicts)
from dpll_replay import SAT, UNKNOWN, UNSAT, replay_one
from test_dpll_gpu import BIG, check_case

pytestmark = pytest.mark.gpu


def lds_bytes(V, C):
    return 8 * C + 14 * V + (V + 15) // 16 * 16


def shared_case(key, pool, V, pidx, cubes=None, cube_bits=0, lib=None):
    """check_case against a replay computed once per session."""
    ref = shared_replay(("edge",) + tuple(key), pool, V, pidx, cubes, cube_bits, BIG)
    return check_case(pool, V, pidx, cubes, cube_bits, ref=ref, lib=lib)


# ------------------------------------------------------------ variable-loop trips ----
def trip_pool(V):
    return random_pool(V, max(1, round(4.3 * V)), 4, 1000 + V)


@pytest.mark.parametrize("V", [63, 64, 65, 128, 129])
def test_variable_loop_trips(V):
    """One, two and three trips of the `base += 64` loops and their ballots, a partial last trip on either side."""
    pool = trip_pool(V)
    ref = shared_case(("trip", V), pool, V, np.arange(4))
    assert (ref[0] != UNKNOWN).all()
    if V <= 65:  # the independent solver is cheap here
        assert np.array_equal(ref[0], indep.verdicts(pool, V, "occur"))


@pytest.mark.parametrize("name", ["x", "not x", "x and not x"])
def test_one_variable(name):
    pool, V, status, nodes = hand_made(name)
    assert V == 1
    ref = check_case(pool, V, [0, 0, 0], [0, 1, 0], 1)
    assert (ref[0] == status).all() and (ref[2] == nodes).all()
    assert status == (SAT if brute_force_sat(pool[0], V) else UNSAT)


# ------------------------------------------------------ clause passes, the LDS bound ----
@pytest.mark.parametrize("C", [1, 128, 129, 640])
def test_clause_passes(C):
    """One pass with one clause, two full passes, two and one clause, ten passes; against brute force as well."""
    pool = random_pool(12, C, 4, 40 + C)
    ref = check_case(pool, 12, np.arange(4))
    for n in range(4):
        assert ref[0][n] == (SAT if brute_force_sat(pool[n], 12) else UNSAT)


def test_127_clause_passes_at_the_lds_bound():
    V, C = 64, 8072
    assert lds_bytes(V, C) == 65536
    pool = random_pool(V, C, 2, 5)
    ref = shared_case(("lds", V, C), pool, V, [0, 1, 1, 0])
    assert (ref[0] == UNSAT).all() and (ref[2] == 6).all()
    assert indep.verdicts(pool, V).tolist() == [UNSAT, UNSAT]


def test_200_variables_at_the_lds_bound():
    V, C = 200, 7816
    assert lds_bytes(V, C) == 65536
    pool = random_pool(V, C, 1, 6)
    ref = check_case(pool, V, [0, 0], [1, 2], 2)
    assert (ref[0] == UNSAT).all()
    ref = check_case(pool, V, [0])
    assert ref[0][0] == UNSAT and ref[2][0] == 12
    assert indep.verdicts(pool, V).tolist() == [UNSAT]


def test_one_variable_and_the_most_clauses():
    """V = 1, C = 8188: 128 passes, the one conflicting row in the last pass's last lanes."""
    V, C = 1, 8188
    assert lds_bytes(V, C) == 65534 and lds_bytes(V, C + 1) > 65536
    pool = np.zeros((1, C, 3), np.int32)
    pool[0, :, 0] = 1
    pool[0, -1, 0] = -1
    ref = check_case(pool, V, [0, 0])
    assert (ref[0] == UNSAT).all() and not ref[2].any() and (ref[3] == 1).all() and not ref[4].any()
    sat = pool.copy()
    sat[0, -1, 0] = 1  # without the last row: a model
    ref = check_case(sat, V, [0])
    assert ref[0][0] == SAT and ref[1][0, 0] == 1 and (ref[2][0], ref[3][0], ref[4][0]) == (0, 0, 1)


def test_one_clause_and_the_most_variables():
    """V = 4368, C = 1: 69 trips of every variable loop, the last of 16 lanes; 65536 - 8 bytes of LDS."""
    V, C = 4368, 1
    assert lds_bytes(V, C) == 65536 - 8 and lds_bytes(V + 1, C) > 65536
    pool = np.array([[[V, 0, 0]]], np.int32)
    ref = check_case(pool, V, [0, 0])
    assert (ref[0] == SAT).all() and not ref[2].any() and not ref[3].any() and (ref[4] == 1).all()
    assert np.array_equal(np.flatnonzero(ref[1][0]), [V - 1])
    pool = np.array([[[-1, V, 0]]], np.int32)  # one decision over 4368 candidates: the lowest index wins the tie
    ref = check_case(pool, V, [0])
    assert ref[0][0] == SAT and (ref[2][0], ref[3][0], ref[4][0]) == (1, 0, 0) and not ref[1][0].any()


# ------------------------------------------------------------------ levels past 255 ----
def test_chain_flips_at_level_300():
    """The counts and the model are derived in dpll_cases.chain and pinned for the replay in
    tests/test_dpll_sound_cpu.py; here the kernel's 16-bit levels and its stack hold entries up to 300."""
    cl, V = chain(300)
    stats = {}
    assert replay_one(cl[0], V, 0, 0, BIG, stats)[2:] == (301, 1, 1)
    assert stats["max_level"] == 300 and stats["flips"] == [(300, 300)]  # a flip at level 300
    ref = shared_case(("chain",), cl, V, [0])
    assert (ref[0][0], ref[2][0], ref[3][0], ref[4][0]) == (SAT, 301, 1, 1)
    want = np.zeros(V, np.uint8)
    want[0:597:2] = 1
    want[599] = 1
    assert np.array_equal(ref[1][0], want)
    # 30 closed levels: cube 2^30 - 1 walks the same path, cube 0 sets the even variables of the first 30 pairs
    ref = shared_case(("chain", 30), cl, V, [0, 0], [2 ** 30 - 1, 0], 30)
    assert ref[0].tolist() == [SAT, SAT] and ref[2].tolist() == [301, 301] and ref[3].tolist() == [1, 1]
    assert ref[4].tolist() == [1, 31]
    assert np.array_equal(ref[1][0], want)
    want[0:60:2], want[1:60:2] = 0, 1
    assert np.array_equal(ref[1][1], want)


def test_chain_pops_level_300_and_flips_299():
    cl, V = chain_two_pops(298)
    stats = {}
    assert replay_one(cl[0], V, 0, 0, BIG, stats)[2:] == (302, 2, 1)
    assert stats == {"max_level": 300, "deepest_flip": 300, "max_pops": 1, "flips": [(300, 300), (300, 299)]}
    ref = shared_case(("chain2",), cl, V, [0])
    assert (ref[0][0], ref[2][0], ref[3][0], ref[4][0]) == (SAT, 302, 2, 1)
    assert ref[1][0, 597] == 1 and not ref[1][0, [596, 598, 599, 600]].any()


# --------------------------------------------------------------------- sample count ----
def test_8192_samples():
    """A grid of 8192 waves over the uf20 pool: all 64 (instance, cube) pairs of 2 cube bits, visited with a stride
    coprime to 64; the replay runs once per pair."""
    pool, V, N = sound_pool("uf20")
    assert N == 16
    pair = (np.arange(8192) * 37 + 11) % 64
    assert len(set(pair[:64].tolist())) == 64
    once = shared_replay(("edge", "pairs"), pool, V, np.arange(64) % 16, np.arange(64) // 16, 2, BIG)
    ref = tuple(r[pair] for r in once)
    check_case(pool, V, pair % 16, pair // 16, 2, ref=ref)  # the guard rows past sample 8191 are checked there


# --------------------------------------------------------------------- budget ends ----
def test_largest_node_budget():
    pool, V, N = sound_pool("uf20")
    ref = shared_replay(("edge", "uf20"), pool, V, np.arange(N), None, 0, BIG)
    assert (ref[2] < BIG).all()  # so that the replay under 2^31 - 1 is this one
    check_case(pool, V, np.arange(N), max_nodes=2 ** 31 - 1, ref=ref)
    assert np.array_equal(ref[0], sound_verdicts("uf20"))


@pytest.mark.parametrize("want", [SAT, UNSAT])
def test_exact_node_budget(want):
    """A budget of exactly the sample's node count decides it; one node less does not."""
    pool, V, N = sound_pool("uf20")
    full = shared_replay(("edge", "uf20"), pool, V, np.arange(N), None, 0, BIG)
    n = int(np.flatnonzero((full[0] == want) & (full[2] >= 2))[0])
    nodes = int(full[2][n])
    ref = check_case(pool, V, [n], max_nodes=nodes)
    assert all(np.array_equal(r[0], f[n]) for r, f in zip(ref, full)) and ref[0][0] == want
    ref = check_case(pool, V, [n], max_nodes=nodes - 1)
    assert ref[0][0] == UNKNOWN and ref[2][0] == nodes - 1 and not ref[1].any()


# ------------------------------------------------------------------ irregular pools ----
IRREGULAR = ["quirks23", "k2", "k1", "solo", "wide257", "wide513k2", "wide600"]


def searched_pool(name):
    """The pool `name` (N, C, K), and after it every instance that holds an all-zero clause again with that clause
    overwritten by the row before it: the all-zero clause ends a search at level 0, and the copy is what sends the
    literal-0, duplicate and tautology rows (past row 255 in the wide pools) and the variable in 70 clauses through
    propagation and branching."""
    p = irregular_pools.get(name)
    extra = []
    for n in range(p.pool.shape[0]):
        zero = np.flatnonzero(~p.pool[n].any(axis=1))
        if len(zero):
            assert p.names[n] == "quirk-rows" and len(zero) == 1 and zero[0] > 0
            cl = p.pool[n].copy()
            cl[zero[0]] = cl[zero[0] - 1]
            extra.append(cl)
    pool = np.concatenate([p.pool, np.stack(extra)]) if extra else p.pool
    return p, pool.astype(np.int32)


@pytest.mark.parametrize("name", IRREGULAR)
def test_irregular_pools(name):
    p, pool = searched_pool(name)
    N = pool.shape[0]
    single = shared_case(("irr", name, 0), pool, p.V, np.arange(N))
    cubed = shared_case(("irr", name, 2), pool, p.V, np.repeat(np.arange(N), 4), np.tile(np.arange(4), N), 2)
    truth = indep.verdicts(pool, p.V, "occur")
    assert np.array_equal(single[0], truth)
    for n in range(N):
        iso = irregular_pools.isolated_vars(pool[n], p.V)
        for st, x in [(single[0][n], single[1][n])] + [(cubed[0][4 * n + q], cubed[1][4 * n + q]) for q in range(4)]:
            assert st != UNKNOWN
            assert not x[iso].any()  # a variable in no clause is never assigned: its model byte is 0
        assert (SAT in cubed[0][4 * n:4 * n + 4]) == (truth[n] == SAT)  # the cube rule
        if not pool[n].any(axis=1).all():  # an all-zero clause ("quirk-rows"): a conflict before any decision
            assert single[0][n] == UNSAT and single[2][n] == 0 and (cubed[0][4 * n:4 * n + 4] == UNSAT).all()
            assert not cubed[2][4 * n:4 * n + 4].any()
    if name in ("wide257", "wide600"):  # the copies without the all-zero clause do search; in the other pools the
        assert single[2][len(p.names):].all()  # quirk rows still hold opposite units (a conflict of the first pass)


# -------------------------------------------------------------------- debug library ----
def test_debug_library_at_the_edges():
    """libmarlsat_debug.so (MSAT_DCHECK on every global and LDS index) on the chain, the 65536-byte shape, V = 65,
    quirks23 and wide513k2: the replay's outputs, and no index check trips."""
    from conftest import ROOT
    from marlsat import _lib

    path = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    if not os.path.exists(path):
        status = os.path.join(os.path.dirname(path), "debug_build_status.json")
        if os.path.exists(status):
            pytest.fail("libmarlsat_debug.so missing although a build ran: " + open(status).read())
        pytest.skip("libmarlsat_debug.so not built (make -C marl-sat_amd debug)")
    dbg = ctypes.CDLL(path)
    dbg.msat_dpll.restype = ctypes.c_int32
    dbg.msat_dpll.argtypes = _lib.lib.msat_dpll.argtypes
    dbg.msat_last_error.restype = ctypes.c_char_p
    cl, V = chain(300)
    shared_case(("chain",), cl, V, [0], lib=dbg)
    shared_case(("chain", 30), cl, V, [0, 0], [2 ** 30 - 1, 0], 30, lib=dbg)
    cl, V = chain_two_pops(298)
    shared_case(("chain2",), cl, V, [0], lib=dbg)
    shared_case(("lds", 64, 8072), random_pool(64, 8072, 2, 5), 64, [0, 1, 1, 0], lib=dbg)
    shared_case(("trip", 65), trip_pool(65), 65, np.arange(4), lib=dbg)
    for name in ("quirks23", "wide513k2"):
        p, pool = searched_pool(name)
        N = pool.shape[0]
        shared_case(("irr", name, 0), pool, p.V, np.arange(N), lib=dbg)
        shared_case(("irr", name, 2), pool, p.V, np.repeat(np.arange(N), 4), np.tile(np.arange(4), N), 2, lib=dbg)
