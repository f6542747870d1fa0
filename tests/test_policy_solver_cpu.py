"""Host side of the policy solver (no GPU): argument validation, the key schedule, the round plan, the report
helpers and the new entry points' argument checks through the C-ABI's error channel."""
import ctypes
import json

import numpy as np
import pytest


def _ok_args(**kw):
    d = dict(tries=8, rounds=2, max_steps=16, env_max_steps=16, temperature=1.0, finish="walksat", finish_tries=8,
             finish_flips=1000, noise=0.5, max_batch=4096)
    d.update(kw)
    return d


def test_solve_args_accepted():
    from marlsat.solvers.policy import check_solve_args

    check_solve_args(**_ok_args())
    check_solve_args(**_ok_args(rounds=0, finish="none", finish_flips=0, max_batch=8, temperature=0.3, noise=0.0))


@pytest.mark.parametrize("bad,msg", [
    (dict(tries=0), "tries"),
    (dict(rounds=-1), "rounds"),
    (dict(max_steps=None), "max_steps"),
    (dict(max_steps=0), "max_steps"),
    (dict(max_steps=17), "max_steps"),
    (dict(temperature=0.0), "temperature"),
    (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("inf")), "temperature"),
    (dict(temperature=float("nan")), "temperature"),
    (dict(finish="cdcl"), "finish"),
    (dict(finish_tries=0), "finish_tries"),
    (dict(finish_flips=-1), "finish_flips"),
    (dict(noise=1.5), "noise"),
    (dict(max_batch=7), "max_batch"),
])
def test_solve_args_rejected(bad, msg):
    from marlsat.solvers.policy import check_solve_args

    with pytest.raises(ValueError, match=msg):
        check_solve_args(**_ok_args(**bad))


def test_key_schedule_is_evaluate_policys():
    """runners/mappo_runner.py evaluate_policy: k_reset, k_run = split(key); per step k_run, k_act = split(k_run)."""
    from marlsat.random import Key, split
    from marlsat.solvers.policy import search_keys

    key = Key(21, 4)
    k_reset, k_run = split(key, 2)
    want = []
    for _ in range(5):
        k_run, k_act = split(k_run, 2)
        want.append(k_act)
    got_reset, got = search_keys(key, 5)
    assert got_reset == k_reset and got == want
    assert search_keys((21, 4), 5) == (k_reset, want)  # a (seed, counter) tuple, as evaluate_policy takes
    assert search_keys(key, 0) == (k_reset, [])
    assert len({(k.seed, k.counter) for k in want + [k_reset]}) == 6
    assert search_keys(Key(21, 5), 5)[1] != want  # another counter: another schedule


def test_round_plan():
    from marlsat.solvers.policy import round_plan

    assert round_plan(3, 8, True) == [(True, 1), (False, 8), (False, 8)]
    assert round_plan(2, 3, False) == [(False, 3), (False, 3)]
    assert round_plan(0, 3, True) == []


def _result():
    i32 = lambda *v: np.array(v, dtype=np.int32)
    return {"solved": np.array([True, True, False, True]), "by": np.array([1, 2, 0, 1], dtype=np.int8),
            "solution": np.zeros((4, 3), np.uint8), "round": i32(0, 1, 1, 1), "try": i32(0, 2, 1, 0),
            "steps": i32(4, -1, -1, 10), "flips": i32(6, 30, 28, 12), "finish_flips": i32(-1, 77, -1, -1),
            "best_unsat": i32(0, 2, 1, 0), "best_solution": np.zeros((4, 3), np.uint8)}


def test_report_schema():
    from marlsat.utils.policy_solver import INSTANCE_FIELDS, group_report, instance_report

    res = _result()
    e = instance_report("a.cnf", res, 1)
    assert tuple(e) == INSTANCE_FIELDS
    assert e == {"name": "a.cnf", "solved": True, "by": "walksat", "round": 1, "try": 2, "steps": -1, "flips": 30,
                 "finish_flips": 77, "best_unsat": 2}
    base = {"solved": np.array([True, True, True, False]), "flips": np.array([10, 30, 20, -1], dtype=np.int32)}
    g = group_report(3, 9, ["a", "b", "c", "d"], res, base)
    assert (g["num_vars"], g["num_clauses"], g["instances"]) == (3, 9, 4)
    assert (g["solved_by_policy"], g["solved_by_walksat"], g["unsolved"]) == (2, 1, 1)
    assert g["solve_rate_policy"] == 0.5 and g["solve_rate_with_finish"] == 0.75
    assert g["median_policy_steps"] == 7.0 and g["median_policy_flips"] == 9.0 and g["median_finish_flips"] == 77.0
    assert g["baseline_walksat"] == {"solve_rate": 0.75, "median_flips": 20.0}
    assert [r["name"] for r in g["results"]] == ["a", "b", "c", "d"]
    assert json.loads(json.dumps(g)) == g  # plain JSON types throughout
    none = dict(res, by=np.zeros(4, np.int8), solved=np.zeros(4, bool))
    g0 = group_report(3, 9, ["a", "b", "c", "d"], none)
    assert g0["median_policy_steps"] is None and g0["solve_rate_policy"] == 0.0 and "baseline_walksat" not in g0


def test_missing_checkpoint_is_an_error(tmp_path):
    from marlsat.utils.policy_solver import find_checkpoint

    with pytest.raises(FileNotFoundError, match="no checkpoint"):
        find_checkpoint(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="no checkpoint"):
        find_checkpoint(str(tmp_path / "absent"))


def test_cli_arguments():
    from marlsat.utils.policy_solver import build_parser

    a = build_parser().parse_args(["--checkpoint", "c", "--cnf-dir", "d", "--sol-dir", "o", "network.GNN_HIDDEN_DIM=64"])
    assert (a.tries, a.rounds, a.max_steps, a.temperature, a.finish, a.finish_tries, a.finish_flips, a.noise,
            a.seed) == (8, 2, None, 1.0, "walksat", 8, 100_000, 0.5, 0)
    assert not a.no_greedy_round and not a.baseline_walksat and a.report is None
    assert a.overrides == ["network.GNN_HIDDEN_DIM=64"]
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--checkpoint", "c", "--cnf-dir", "d", "--sol-dir", "o", "--finish", "cdcl"])


@pytest.mark.parametrize("inv_t", [0.0, -1.0, float("nan"), float("inf")])
def test_sample_actions_t_rejects_bad_inverse_temperature(inv_t):
    """Checked before any pointer is touched or a launch is made."""
    from marlsat import _lib

    L = _lib.lib
    assert L.msat_sample_actions_t(8, 1, 4, inv_t, 0, 0, 8, 8, None) == -1
    assert "inv_temperature" in L.msat_last_error().decode()
    assert L.msat_sample_actions_from(8, 1, 4, 0, inv_t, 0, 0, 8, 8, None) == -1
    assert L.msat_sample_actions_from(8, 1, 4, -1, 1.0, 0, 0, 8, 8, None) == -1
    assert "rows" in L.msat_last_error().decode()
    assert L.msat_sample_actions_t(None, 0, 4, 1.0, 0, 0, None, None, None) == 0  # no rows: no launch


def test_track_and_pick_reject_bad_arguments():
    from marlsat import _lib

    L = _lib.lib
    st = _lib.SolveStateC(8, 8, 8, 8, 8, 8, 8)  # never dereferenced: validation fails first
    assert L.msat_solve_track_init(-1, 4, 8, 8, ctypes.byref(st), None) == -1
    assert L.msat_solve_track_init(2, 0, 8, 8, ctypes.byref(st), None) == -1
    assert L.msat_solve_track_init(2, 4, None, 8, ctypes.byref(st), None) == -1
    assert "NULL" in L.msat_last_error().decode()
    assert L.msat_solve_track(2, 4, 0, 8, 8, 8, ctypes.byref(st), None) == -1
    assert "step" in L.msat_last_error().decode()
    assert L.msat_solve_track(2, 4, 1, 8, 8, 8, None, None) == -1
    no_word = _lib.SolveStateC(8, 8, 8, 8, 8, 8, None)
    assert L.msat_solve_track(2, 4, 1, 8, 8, 8, ctypes.byref(no_word), None) == -1
    assert "unsolved" in L.msat_last_error().decode()
    no_best = _lib.SolveStateC(8, None, 8, 8, 8, 8, 8)
    assert L.msat_solve_track(2, 4, 1, 8, 8, 8, ctypes.byref(no_best), None) == -1
    assert L.msat_solve_pick(2, 0, 4, ctypes.byref(st), 8, 8, 8, 8, 8, 8, 8, None) == -1
    assert "tries" in L.msat_last_error().decode()
    assert L.msat_solve_pick(1 << 20, 1 << 20, 4, ctypes.byref(st), 8, 8, 8, 8, 8, 8, 8, None) == -1
    assert L.msat_solve_pick(2, 3, 4, ctypes.byref(st), 8, 8, 8, None, 8, 8, 8, None) == -1
    assert L.msat_solve_pick(0, 3, 4, None, None, None, None, None, None, None, None, None) == 0


def test_learner_policy_keeps_its_signature():
    """The new keywords come last and default to the old behaviour (temperature 1.0, no row offset)."""
    import inspect

    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner

    p = inspect.signature(MAPPOLearner.policy).parameters
    assert list(p)[:5] == ["self", "st", "key", "greedy", "critic"]
    assert p["temperature"].default == 1.0 and p["row_offset"].default is None
