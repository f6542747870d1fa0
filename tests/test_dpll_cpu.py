"""CPU tests of the DPLL feature's host side.  The NumPy replay (tests/dpll_replay.py, the yardstick of the GPU
tests) is held against ground truth that shares nothing with it: brute-force enumeration of all 2^V assignments
for V <= 14 gives the status, and every returned model goes through a clause check of its own.  Then the cube
rule, the node budget, the argument checks and LDS plan of msat_dpll (no GPU work is launched by these calls), the
CLI parser and the bc_training key."""
import os

import numpy as np
import pytest

from dpll_cases import HAND_MADE, brute_force_sat, hand_made, pigeonhole, random_pool, satisfied
from dpll_replay import SAT, UNKNOWN, UNSAT, combine, replay
from oracle.sat_env import OracleSATEnv

BIG = 200000


def check_against_brute_force(pool, V, res):
    status, x = res[0], res[1]
    for n in range(pool.shape[0]):
        assert status[n] == (SAT if brute_force_sat(pool[n], V) else UNSAT), n
        if status[n] == SAT:
            assert satisfied(x[n], pool[n]).all(), n
        else:
            assert not x[n].any()
    sat = status == SAT
    if sat.any():
        _, nun = OracleSATEnv.satisfaction(x[sat].astype(np.int32), pool[sat])
        assert (np.asarray(nun) == 0).all()


@pytest.mark.parametrize("V,C,N,seed", [(12, 80, 6, 1), (14, 60, 10, 2), (7, 63, 4, 3), (7, 64, 4, 4), (7, 65, 4, 5),
                                        (10, 43, 12, 6), (5, 20, 8, 7), (3, 6, 8, 8)])
def test_replay_status_equals_brute_force(V, C, N, seed):
    pool = random_pool(V, C, N, seed)
    res = replay(pool, V, np.arange(N), max_nodes=BIG)
    assert (res[0] != UNKNOWN).all()
    check_against_brute_force(pool, V, res)


def test_random_pools_mix_sat_and_unsat():
    """The pools the GPU tests share hold both verdicts (otherwise they would test one path only)."""
    for V, C, N, seed in [(14, 60, 10, 2), (10, 43, 12, 6)]:
        st = replay(random_pool(V, C, N, seed), V, np.arange(N), max_nodes=BIG)[0]
        assert (st == SAT).any() and (st == UNSAT).any(), (V, C)


def test_pigeonhole_is_unsat():
    pool, V = pigeonhole(4, 3)
    assert pool.shape == (1, 22, 3) and V == 12 and not brute_force_sat(pool[0], V)
    st, x, nodes, conflicts, _ = replay(pool, V, [0], max_nodes=BIG)
    assert st[0] == UNSAT and not x.any() and 0 < nodes[0] <= 64 and conflicts[0] >= 1


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_cases(name):
    pool, V, status, nodes = hand_made(name)
    res = replay(pool, V, [0], max_nodes=BIG)
    assert res[0][0] == status
    if nodes is not None:
        assert res[2][0] == nodes
    check_against_brute_force(pool, V, res)
    if name == "all-NULL clause":
        assert res[2][0] == 0 and res[3][0] == 1 and res[4][0] == 0  # a conflict of the first pass at level 0
    if name == "contradicting units of one pass":
        # pass 1 assigns x1 = 0 and x3 = 0; pass 2 has the units x2 (from x1 v x2) and -x2 (from -x2 v x3): conflict
        assert res[3][0] == 1 and res[4][0] == 2


@pytest.mark.parametrize("V,C,N,seed", [(14, 60, 10, 2), (12, 80, 4, 1), (10, 43, 12, 6)])
@pytest.mark.parametrize("bits", [1, 2, 3])
def test_cube_rule_combines_to_the_single_search_verdict(V, C, N, seed, bits):
    pool = random_pool(V, C, N, seed)
    single = replay(pool, V, np.arange(N), max_nodes=BIG)
    K = 1 << bits
    pidx, cubes = np.repeat(np.arange(N), K), np.tile(np.arange(K), N)
    st, x, nodes, _, _ = replay(pool, V, pidx, cubes, bits, BIG)
    for n in range(N):
        assert combine(st[n * K:(n + 1) * K]) == single[0][n], n
    for s in np.flatnonzero(st == SAT):
        assert satisfied(x[s], pool[pidx[s]]).all()
    assert (st != UNKNOWN).all()


def test_cube_zero_bits_ignores_the_cube_word():
    pool = random_pool(10, 43, 4, 6)
    a = replay(pool, 10, np.arange(4), None, 0, BIG)
    b = replay(pool, 10, np.arange(4), [5, 1, 7, 3], 0, BIG)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_node_budget():
    V, C, N = 14, 60, 10
    pool = random_pool(V, C, N, 2)
    full = replay(pool, V, np.arange(N), max_nodes=BIG)
    for budget in (0, 1, 3):
        st, x, nodes, _, _ = replay(pool, V, np.arange(N), max_nodes=budget)
        more = full[2] > budget
        assert more.any()
        assert (st[more] == UNKNOWN).all() and (nodes[more] == budget).all() and not x[more].any()
        for k in range(5):  # a search that fits the budget is the full search
            assert np.array_equal(replay(pool, V, np.arange(N), max_nodes=budget)[k][~more], full[k][~more])


def test_problem_idx_is_clamped():
    pool = random_pool(7, 30, 3, 9)
    pidx = np.array([-5, 0, 2, 3, 2 ** 31 - 1, -2 ** 31])
    a = replay(pool, 7, pidx, max_nodes=BIG)
    b = replay(pool, 7, np.clip(pidx, 0, 2), max_nodes=BIG)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------ the C-ABI ----
_ARGS = dict(lits=8, N=1, V=20, C=91, pidx=8, cube=None, S=2, bits=0, max_nodes=10, status=8, out=8, nodes=8,
             conflicts=8, props=8)


def _call(**kw):
    from marlsat import _lib

    a = dict(_ARGS)
    a.update(kw)
    rc = _lib.lib.msat_dpll(a["lits"], a["N"], a["V"], a["C"], a["pidx"], a["cube"], a["S"], a["bits"],
                            a["max_nodes"], a["status"], a["out"], a["nodes"], a["conflicts"], a["props"], None)
    return rc, _lib.lib.msat_last_error().decode()


@pytest.mark.parametrize("bad,msg", [
    (dict(lits=None), "NULL"),
    (dict(pidx=None), "NULL"),
    (dict(status=None), "NULL"),
    (dict(out=None), "NULL"),
    (dict(nodes=None), "NULL"),
    (dict(conflicts=None), "NULL"),
    (dict(props=None), "NULL"),
    (dict(V=0), "num_vars 0"),
    (dict(V=32001), "num_vars 32001"),
    (dict(C=0), "num_clauses 0"),
    (dict(N=0), "num_problems 0"),
    (dict(S=-1), "num_samples -1"),
    (dict(max_nodes=-1), "max_nodes -1"),
    (dict(bits=-1), "cube_bits -1"),
    (dict(bits=31), "cube_bits 31"),
    (dict(V=1, C=8189), "LDS"),      # 8 * 8189 + 14 + 16 = 65542 > 65536
    (dict(V=4369, C=1), "LDS"),      # 8 + 14 * 4369 + 4384 = 65558
    (dict(V=32000, C=1), "LDS"),
])
def test_dpll_bad_arguments(bad, msg):
    rc, err = _call(**bad)  # pointers are never dereferenced: validation fails first
    assert rc == -1
    assert msg in err and "dpll" in err


def test_dpll_lds_plan_and_empty_batch():
    from marlsat import _lib

    # num_samples == 0 is a no-op that launches nothing and needs no pointers; the plan is still checked
    none = dict(S=0, lits=None, pidx=None, status=None, out=None, nodes=None, conflicts=None, props=None)
    assert _call(**none)[0] == 0
    assert _call(V=1, C=8188, **none)[0] == 0    # 65504 + 14 + 16 = 65534
    assert _call(V=4368, C=1, **none)[0] == 0    # 8 + 61152 + 4368 = 65528
    assert _call(V=300, C=1290, **none)[0] == 0
    assert _call(V=1, C=8189, **none)[0] == -1
    assert "msat_dpll" in _lib.EXPORTED
    assert _lib.lib.msat_version() == 3  # an additive entry point


def test_cli_parser_complete_flags():
    from marlsat.utils.sat_solver import build_parser

    a = build_parser().parse_args(["--cnf-dir", "D", "--sol-dir", "O"])
    assert a.complete is False
    a = build_parser().parse_args(["--cnf-dir", "D", "--sol-dir", "O", "--complete", "--max-nodes", "77",
                                   "--cube-bits", "2"])
    assert a.complete is True and a.max_nodes == 77 and a.cube_bits == 2


def test_bc_settings_solve_missing_complete_defaults_off():
    from marlsat.runners.behavioral_cloning import bc_settings
    from marlsat.runners.mappo_runner import load_config

    assert bc_settings({})["SOLVE_MISSING_COMPLETE"] is False
    path = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")
    assert bc_settings(load_config(path))["SOLVE_MISSING_COMPLETE"] is False
    assert bc_settings(load_config(path, ["bc_training.SOLVE_MISSING_COMPLETE=true"]))["SOLVE_MISSING_COMPLETE"] is True


def test_dpll_host_glue_under_asan():
    """tests/dpll_host_check.cpp against the library's AddressSanitizer objects (marl-sat_amd/Makefile `debug`): the
    argument checks and the LDS plan, as a stand-alone program with nothing preloaded, with no ASan report.  Skips
    only where no build ran."""
    import json
    import subprocess

    from conftest import ROOT

    binary = os.path.join(ROOT, "marl-sat_amd", "build", "asan", "dpll_host_check")
    status = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "debug_build_status.json")
    if not os.path.exists(binary):
        if os.path.exists(status):
            pytest.fail(f"dpll_host_check missing: build()'s 'make debug' exited "
                        f"{json.load(open(status)).get('make_debug_rc')}")
        pytest.skip("dpll_host_check not built (make -C marl-sat_amd debug; __graft_entry__.build() does)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dpll_host_check: ok" in r.stdout and "AddressSanitizer" not in r.stderr
