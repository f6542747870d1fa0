"""CPU tests of the WalkSAT feature's host side: the NumPy replay (tests/walksat_replay.py, the yardstick of the
GPU tests) against the oracle's clause truth, the argument checks of msat_walksat (no GPU work is launched by
these calls), the .sol writer / load_expert_data round trip, the CLI parser and the bc_training key."""
import os

import numpy as np
import pytest

from oracle.sat_env import OracleSATEnv
from walksat_replay import clause_status, noise_p32, replay


def test_replay_solutions_satisfy_under_the_oracle():
    """Every assignment the replay reports solved satisfies its formula under oracle.sat_env's clause truth, the
    unsolved ones report the oracle's unsatisfied count; the uf20 counts are those of the algorithm as
    include/marlsat.h states it (64 / 64 solved within 33 flips at noise 0.5)."""
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    V, C, N, R = 20, 91, 16, 4
    pool = generate_problem_pool(V, C, N, size_id=0)
    pidx = np.arange(N * R) // R
    x, solved, flips, nun = replay(pool, V, pidx, 2000, noise_p32(0.5), 1234, 7)
    assert solved.all() and flips.max() == 33
    _, o_nun = OracleSATEnv.satisfaction(x.astype(np.int32), pool[pidx])
    assert (np.asarray(o_nun) == 0).all() and (nun == 0).all()
    # a budget too small for most runs: the unsolved path reports flips == max_flips and the oracle's count
    x, solved, flips, nun = replay(pool, V, pidx, 3, noise_p32(0.5), 1234, 7)
    assert (solved == 0).any()
    status, o_nun = OracleSATEnv.satisfaction(x.astype(np.int32), pool[pidx])
    assert np.array_equal(np.asarray(o_nun), nun)
    assert np.array_equal(solved == 1, nun == 0) and (flips[solved == 0] == 3).all()
    for s in range(len(pidx)):
        assert np.array_equal(clause_status(x[s], pool[pidx[s]]), np.asarray(status[s]).astype(bool))


def test_replay_literal_edges():
    """Null literals are false and no candidates; a clause of zeros is never satisfied and never flips."""
    x, solved, flips, nun = replay(np.array([[[0, 0, 0], [1, 2, 0]]], np.int32), 2, [0], 5, noise_p32(0.5), 1, 2,
                                   init_assign=np.array([[0, 0]], np.uint8))
    assert solved[0] == 0 and flips[0] == 5 and nun[0] >= 1
    x, solved, flips, nun = replay(np.array([[[1], [-1]]], np.int32), 1, [0], 7, noise_p32(0.5), 1, 2,
                                   init_assign=np.array([[1]], np.uint8))
    assert solved[0] == 0 and flips[0] == 7 and nun[0] == 1 and x[0, 0] == 0  # seven flips of the one variable
    # x v x v -y from (0, 1): flipping x satisfies at once; break counts see the duplicated variable once
    x, solved, flips, nun = replay(np.array([[[1, 1, -2]]], np.int32), 2, [0], 7, 0, 1, 2,
                                   init_assign=np.array([[0, 1]], np.uint8))
    assert solved[0] == 1 and flips[0] == 1 and list(x[0]) == [1, 1]


_ARGS = dict(lits=8, N=1, V=20, C=91, pidx=8, S=2, init=None, max_flips=10, noise=0, seed=1, counter=2, form=0,
             out=8, solved=8, flips=8, nun=8)


def _call(**kw):
    from marlsat import _lib

    a = dict(_ARGS)
    a.update(kw)
    rc = _lib.lib.msat_walksat(a["lits"], a["N"], a["V"], a["C"], a["pidx"], a["S"], a["init"], a["max_flips"],
                               a["noise"], a["seed"], a["counter"], a["form"], a["out"], a["solved"], a["flips"],
                               a["nun"], None)
    return rc, _lib.lib.msat_last_error().decode()


@pytest.mark.parametrize("bad,msg", [
    (dict(lits=None), "NULL"),
    (dict(pidx=None), "NULL"),
    (dict(out=None), "NULL"),
    (dict(solved=None), "NULL"),
    (dict(flips=None), "NULL"),
    (dict(nun=None), "NULL"),
    (dict(V=0), "num_vars 0"),
    (dict(V=32001), "num_vars 32001"),
    (dict(C=0), "num_clauses 0"),
    (dict(N=0), "num_problems 0"),
    (dict(max_flips=-1), "max_flips -1"),
    (dict(S=-1), "num_samples -1"),
    (dict(form=-1), "form -1"),
    (dict(form=99), "form 99"),
    (dict(form=1, C=129), "form 1 holds num_clauses <= 128"),
    (dict(form=2, C=257), "form 2 holds num_clauses <= 256"),
    (dict(form=3, C=513), "form 3 holds num_clauses <= 512"),
    (dict(form=4, C=1024), "form 4 holds num_clauses <= 1023"),
    (dict(C=8200), "LDS"),          # 8 * 8200 + 32 > 65536: no form holds it
    (dict(V=32000, C=4200), "LDS"),
    (dict(form=6, V=3000, C=3000), "form 6 needs"),  # fits the other forms, not the occurrence lists
])
def test_walksat_bad_arguments(bad, msg):
    rc, err = _call(**bad)  # pointers are never dereferenced: validation fails first
    assert rc == -1
    assert msg in err and "walksat" in err


def test_walksat_forms_and_empty_batch():
    from marlsat import _lib
    from marlsat.solvers.walksat import walksat_forms

    assert _lib.lib.msat_walksat_forms() >= 1 and walksat_forms() == _lib.lib.msat_walksat_forms()
    # num_samples == 0 is a no-op that launches nothing and needs no pointers
    rc, _ = _call(S=0, lits=None, pidx=None, out=None, solved=None, flips=None, nun=None)
    assert rc == 0
    assert _lib.lib.msat_version() == 3  # additive entry points


def test_noise_threshold():
    from marlsat.solvers.walksat import noise_p32 as lib_noise_p32

    assert lib_noise_p32(0.0) == 0 and lib_noise_p32(0.5) == 1 << 31 and lib_noise_p32(1.0) == 2 ** 32 - 1
    for p in (0.0, 0.1, 0.5, 0.57, 1.0):
        assert lib_noise_p32(p) == noise_p32(p)
    with pytest.raises(ValueError):
        lib_noise_p32(1.5)


def test_sol_writer_round_trips_through_load_expert_data(tmp_path):
    from marlsat.runners.behavioral_cloning import load_expert_data
    from marlsat.utils.data_parser import parse_sol, write_cnf
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses, generate_sat_solution
    from marlsat.utils.sat_solver import sol_path, write_sol

    cnf, sol = tmp_path / "cnf", tmp_path / "sol"
    cnf.mkdir()
    sol.mkdir()
    want = {}
    for i, (V, C) in enumerate([(20, 91), (12, 40)]):
        name = f"p{i}.cnf"
        write_cnf(str(cnf / name), V, generate_sat_clauses(V, C, seed=i))
        want[name] = generate_sat_solution(V, i)
        assert sol_path(str(sol), name) == str(sol / f"p{i}.sol")
        write_sol(sol_path(str(sol), name), want[name].astype(np.uint8))
    text = open(sol / "p0.sol").read()
    assert text == " ".join(str(int(v)) for v in want["p0.cnf"]) + "\n" and set(text.split()) <= {"0", "1"}
    assert np.array_equal(parse_sol(str(sol / "p1.sol")), want["p1.cnf"])
    experts = load_expert_data(str(cnf), str(sol))
    assert [e["name"] for e in experts] == sorted(want)
    for e in experts:
        assert np.array_equal(e["expert_solution"], want[e["name"]])
        _, nun = OracleSATEnv.satisfaction(e["expert_solution"][None].astype(np.int32), e["problem_clauses"][None])
        assert int(nun[0]) == 0


def test_cli_parser():
    from marlsat.utils.sat_solver import build_parser

    a = build_parser().parse_args(["--cnf-dir", "D", "--sol-dir", "O"])
    assert (a.cnf_dir, a.sol_dir, a.tries, a.max_flips, a.max_rounds, a.noise, a.seed) == \
        ("D", "O", 8, 100_000, 4, 0.5, 0)
    a = build_parser().parse_args(["--cnf-dir", "D", "--sol-dir", "O", "--tries", "3", "--max-flips", "50",
                                   "--max-rounds", "2", "--noise", "0.25", "--seed", "9"])
    assert (a.tries, a.max_flips, a.max_rounds, a.noise, a.seed) == (3, 50, 2, 0.25, 9)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--cnf-dir", "D"])


def test_bc_settings_solve_missing_experts_defaults_off():
    from marlsat.runners.behavioral_cloning import bc_settings
    from marlsat.runners.mappo_runner import load_config

    assert bc_settings({})["SOLVE_MISSING_EXPERTS"] is False
    path = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")
    assert bc_settings(load_config(path))["SOLVE_MISSING_EXPERTS"] is False
    assert bc_settings(load_config(path, ["bc_training.SOLVE_MISSING_EXPERTS=true"]))["SOLVE_MISSING_EXPERTS"] is True


def test_walksat_host_glue_under_asan():
    """tests/walksat_host_check.cpp against the library's AddressSanitizer objects (marl-sat_amd/Makefile `debug`):
    the argument checks and the LDS plans of every form, with no ASan report.  Skips only where no build ran."""
    import json
    import subprocess

    from conftest import ROOT

    binary = os.path.join(ROOT, "marl-sat_amd", "build", "asan", "walksat_host_check")
    status = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "debug_build_status.json")
    if not os.path.exists(binary):
        if os.path.exists(status):
            pytest.fail(f"walksat_host_check missing: build()'s 'make debug' exited "
                        f"{json.load(open(status)).get('make_debug_rc')}")
        pytest.skip("walksat_host_check not built (make -C marl-sat_amd debug; __graft_entry__.build() does)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "walksat_host_check: ok" in r.stdout and "AddressSanitizer" not in r.stderr
