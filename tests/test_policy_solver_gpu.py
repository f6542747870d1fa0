"""GPU: the policy solver (marlsat/solvers/policy.py, marlsat/utils/policy_solver.py).

  * policy_search(greedy=True) against evaluate_policy, bit for bit, for both action modes at
    test_evaluate_policy_replays_on_oracle's shapes, with and without the early exit;
  * a sampled search (temperature 0.7) replayed on the oracle env from its traced reset assignment and actions:
    every field of the device record, bit-exact;
  * solve_pool_with_policy on 6 planted uf20-91 instances with a randomly initialised network: everything solved
    and verified, finish="none" leaves honest best-so-far records, max_batch changes nothing;
  * the CLI on a generated directory with a second group of another num_vars.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")
SHAPES = {0: (20, 91, 10, 24), 1: (12, 40, 3, 24)}  # V, C, vars_per_agent, T
N = 10


def _setup(mode):
    from marlsat import SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    V, C, vpa, T = SHAPES[mode]
    clauses = generate_problem_pool(V, C, N, size_id=3)
    env = SATEnv(V, C, max_steps=T, vars_per_agent=vpa, action_mode=mode)
    pool = env.make_pool(clauses)
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, mode, V, device="cuda", seed=6)
    lr = MAPPOLearner(dict(NUM_ENVS=N, NUM_STEPS=1, MINIBATCH_SIZE=N), env, net, pool)
    return clauses, env, pool, lr


@pytest.mark.parametrize("mode", [0, 1])
def test_greedy_search_equals_evaluate_policy(mode):
    from marlsat.random import Key
    from marlsat.runners.mappo_runner import evaluate_policy
    from marlsat.solvers.policy import policy_search

    clauses, env, pool, lr = _setup(mode)
    T = SHAPES[mode][3]
    probs = np.arange(N)[::-1].copy()
    key = Key(21, 4)
    tr_e, tr_s = [], []
    want = evaluate_policy(key, lr, pool, probs, T, early_exit=False, trace=tr_e)
    # the two differ by design only where the reset assignment already satisfies the formula
    _, nun0 = env._calculate_satisfaction_explicit(tr_e[0].cpu().numpy(), clauses[probs])
    assert (nun0.cpu().numpy() > 0).all()
    rec = policy_search(lr, pool, probs, T, key, greedy=True, early_exit=False, trace=tr_s)
    assert rec.steps_run == T and len(tr_s) == len(tr_e) == T + 1
    for a, b in zip(tr_s, tr_e):
        assert torch.equal(a, b)
    for g, w in zip(rec.as_evaluation(T), want):
        np.testing.assert_array_equal(g, w)
    early = policy_search(lr, pool, probs, T, key, greedy=True, early_exit=True)
    for k in ("first_solve", "best_unsat", "best_step", "best_x", "flips"):
        assert torch.equal(getattr(early, k), getattr(rec, k)), k
    for g, w in zip(early.as_evaluation(T), evaluate_policy(key, lr, pool, probs, T, early_exit=True)):
        np.testing.assert_array_equal(g, w)
    with pytest.raises(ValueError, match="max_steps"):
        policy_search(lr, pool, probs, T + 1, key)


def test_early_exit_stops_and_changes_no_output():
    """Instances whose reset assignment is the planted solution: every row is solved at init, so the loop stops at
    its first look (step 16) and the record is the init record."""
    from marlsat import SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.random import Key
    from marlsat.solvers.policy import policy_search
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool, generate_sat_solution

    V, C = 20, 91
    clauses = generate_problem_pool(V, C, 4, size_id=3)
    sol = np.stack([generate_sat_solution(V, 3000 + i) for i in range(4)]).astype(np.uint8)
    env = SATEnv(V, C, max_steps=40, vars_per_agent=10)
    _, nun = env._calculate_satisfaction_explicit(sol, clauses)
    assert (nun.cpu().numpy() == 0).all()
    pool = env.make_pool(clauses)
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, V, device="cuda", seed=6)
    lr = MAPPOLearner(dict(NUM_ENVS=4, NUM_STEPS=1, MINIBATCH_SIZE=4), env, net, pool)
    a = policy_search(lr, pool, np.arange(4), 40, Key(1, 0), assignments=sol)
    b = policy_search(lr, pool, np.arange(4), 40, Key(1, 0), assignments=sol, early_exit=False)
    assert a.steps_run == 16 and b.steps_run == 40
    for rec in (a, b):
        assert rec.first_solve.tolist() == [0] * 4 and rec.flips.tolist() == [0] * 4
        assert rec.best_step.tolist() == [0] * 4 and int(rec.unsolved.item()) == 0
        np.testing.assert_array_equal(rec.best_x.cpu().numpy(), sol)


@pytest.mark.parametrize("mode", [0, 1])
def test_sampled_search_replays_on_oracle(mode):
    from marlsat.random import Key, split
    from marlsat.solvers.policy import policy_search
    from oracle.rng import reset_draws
    from oracle.sat_env import OracleSATEnv

    clauses, env, pool, lr = _setup(mode)
    V, C, vpa, T = SHAPES[mode]
    probs = np.arange(N)[::-1].copy()
    key = Key(21, 4)
    trace = []
    rec = policy_search(lr, pool, probs, T, key, greedy=False, temperature=0.7, early_exit=False, trace=trace)
    k_reset, _ = split(key, 2)
    _, x0 = reset_draws(k_reset.seed, k_reset.counter, N, V, N)
    np.testing.assert_array_equal(trace[0].cpu().numpy(), x0)
    ora = OracleSATEnv(V, C, T, vars_per_agent=vpa, action_mode=mode)
    _, ost = ora.reset(clauses[probs], x0.astype(np.int32))
    first = np.where(ost.num_unsatisfied == 0, 0, -1).astype(np.int32)
    best_unsat = ost.num_unsatisfied.astype(np.int32).copy()
    best_step = np.zeros(N, np.int32)
    best_x = x0.astype(np.uint8).copy()
    flips = np.zeros(N, np.int32)
    prev = x0.astype(np.uint8).copy()
    for t in range(1, T + 1):
        _, ost, _, _, info = ora.step(ost, trace[t].cpu().numpy())
        x = ost.variable_assignments.astype(np.uint8)
        live = first < 0
        flips[live] += (prev[live] ^ x[live]).sum(axis=1).astype(np.int32)
        prev[live] = x[live]
        solved = np.asarray(info["solved"], bool)
        nun = np.asarray(info["num_unsatisfied"], np.int32)
        better = live & (solved | (nun < best_unsat))
        best_unsat[better] = np.where(solved, 0, nun)[better]
        best_step[better] = t
        best_x[better] = x[better]
        first[live & solved] = t
    got = {k: getattr(rec, k).cpu().numpy() for k in ("first_solve", "best_unsat", "best_step", "best_x", "flips")}
    np.testing.assert_array_equal(got["first_solve"], first)
    np.testing.assert_array_equal(got["best_unsat"], best_unsat)
    np.testing.assert_array_equal(got["best_step"], best_step)
    np.testing.assert_array_equal(got["best_x"], best_x)
    np.testing.assert_array_equal(got["flips"], flips)
    assert flips.max() > 0
    solved, steps, sol = rec.as_evaluation(T)
    np.testing.assert_array_equal(sol, best_x * (first >= 0)[:, None])
    assert int(rec.unsolved.item()) == (first < 0).sum()
    # sampled means sampled: not the greedy actions; reproducible from the key; another counter differs
    greedy = []
    policy_search(lr, pool, probs, T, key, greedy=True, early_exit=False, trace=greedy)
    assert not all(torch.equal(a, b) for a, b in zip(trace[1:], greedy[1:]))
    again, other = [], []
    rec2 = policy_search(lr, pool, probs, T, key, greedy=False, temperature=0.7, early_exit=False, trace=again)
    assert all(torch.equal(a, b) for a, b in zip(trace, again))
    for k in got:
        assert torch.equal(getattr(rec2, k), getattr(rec, k)), k
    policy_search(lr, pool, probs, T, Key(21, 5), greedy=False, temperature=0.7, early_exit=False, trace=other)
    assert not all(torch.equal(a, b) for a, b in zip(trace, other))


@pytest.fixture(scope="module")
def pool6():
    from marlsat import SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    clauses = generate_problem_pool(20, 91, 6, size_id=0)
    env = SATEnv(20, 91, max_steps=16, vars_per_agent=10)
    pool = env.make_pool(clauses)
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, 20, device="cuda", seed=4)
    lr = MAPPOLearner(dict(NUM_ENVS=18, NUM_STEPS=1, MINIBATCH_SIZE=18), env, net, pool)
    return clauses, env, pool, lr


def test_pool_solve_with_walksat_finish(pool6):
    from marlsat.random import Key
    from marlsat.solvers.policy import solve_pool_with_policy
    from oracle.sat_env import OracleSATEnv

    clauses, env, pool, lr = pool6
    kw = dict(tries=3, rounds=2, max_steps=16, finish_tries=8, finish_flips=20_000, noise=0.5, key=Key(5, 0))
    res = solve_pool_with_policy(lr, pool, **kw)
    assert res["solved"].all()
    assert set(res["by"].tolist()) <= {1, 2}
    _, nun = OracleSATEnv.satisfaction(res["solution"].astype(np.int32), clauses)
    assert (nun == 0).all()
    pol, ws = res["by"] == 1, res["by"] == 2
    assert (res["steps"][pol] >= 0).all() and (res["steps"][pol] <= 16).all() and (res["finish_flips"][pol] == -1).all()
    assert (res["steps"][ws] == -1).all() and (res["finish_flips"][ws] >= 0).all() and (res["best_unsat"][ws] > 0).all()
    assert (res["round"] >= 0).all() and (res["round"] <= 1).all()
    assert (res["try"][res["round"] == 0] == 0).all() and (res["try"] < 3).all()
    np.testing.assert_array_equal(res["best_solution"][pol], res["solution"][pol])

    none = solve_pool_with_policy(lr, pool, **dict(kw, finish="none"))
    np.testing.assert_array_equal(none["solved"], pol)  # the same policy rounds, nothing after them
    missed = ~none["solved"]
    assert (none["by"][missed] == 0).all() and not none["solution"][missed].any()
    assert (none["best_unsat"][missed] > 0).all()
    _, nun_best = OracleSATEnv.satisfaction(none["best_solution"].astype(np.int32), clauses)
    np.testing.assert_array_equal(nun_best, none["best_unsat"])
    for k in ("round", "try", "steps", "flips", "best_unsat", "best_solution"):
        np.testing.assert_array_equal(none[k], res[k], err_msg=k)

    for mb in (4, 7):  # one instance per slab; two
        slabs = solve_pool_with_policy(lr, pool, **dict(kw, max_batch=mb))
        for k in res:
            np.testing.assert_array_equal(slabs[k], res[k], err_msg=f"max_batch={mb} {k}")
    sampled_first = solve_pool_with_policy(lr, pool, **dict(kw, greedy_round=False, finish="none", rounds=1))
    assert (sampled_first["round"] == 0).all() and sampled_first["try"].max() <= 2

    with pytest.raises(ValueError, match="max_steps"):
        solve_pool_with_policy(lr, pool, **dict(kw, max_steps=17))
    with pytest.raises(ValueError, match="another pool"):
        solve_pool_with_policy(lr, env.make_pool(clauses), **kw)


def test_cli_on_a_directory_with_a_foreign_group(tmp_path, capsys):
    from marlsat import SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.runners.behavioral_cloning import load_expert_data
    from marlsat.runners.mappo_runner import verify_solutions_file
    from marlsat.utils import checkpoints as ck
    from marlsat.utils.generate_cnf_dataset import generate_cnf_dataset_sat
    from marlsat.utils.policy_solver import SOLUTIONS_FILE, main

    data, out, run_dir = tmp_path / "data", tmp_path / "out", tmp_path / "run"
    generate_cnf_dataset_sat(5, 20, 91, str(data), seed=5)
    generate_cnf_dataset_sat(2, 12, 40, str(data), seed=6)  # another num_vars: uf12-001.cnf, uf12-002.cnf
    env = SATEnv(20, 91, max_steps=16, vars_per_agent=10)
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, 20, device="cuda", seed=4)
    ck.save_checkpoint(str(run_dir / "checkpoints"), ck.train_state_dict(net), 0, "latest_model_")
    ov = ["environment.NUM_VARS=20", "environment.NUM_CLAUSES=91", "environment.VARS_PER_AGENT=10",
          "environment.MAX_STEPS=16", "network.GNN_HIDDEN_DIM=64", "network.GNN_NUM_MESSAGE_PASSING_STEPS=2"]
    common = ["--config", CFG, "--cnf-dir", str(data), "--sol-dir", str(out), "--tries", "3", "--rounds", "2",
              "--finish-flips", "20000", "--max-batch", "64"]
    report = tmp_path / "report.json"
    rc = main(common + ["--checkpoint", str(run_dir), "--report", str(report), "--baseline-walksat"] + ov)
    rep = json.loads(report.read_text())
    assert rc == (1 if rep["unsolved"] else 0) and rc == 0
    assert [(s["num_vars"], sorted(s["names"])) for s in rep["skipped"]] == [(12, ["uf12-001.cnf", "uf12-002.cnf"])]
    assert "NUM_VARS" in rep["skipped"][0]["reason"]
    (g,) = rep["groups"]
    assert (g["num_vars"], g["num_clauses"], g["instances"]) == (20, 91, 5)
    assert g["solve_rate_with_finish"] == 1.0 and g["solved_by_policy"] + g["solved_by_walksat"] == 5
    assert g["baseline_walksat"]["solve_rate"] == 1.0 and g["baseline_walksat"]["median_flips"] >= 0
    assert sorted(r["name"] for r in g["results"]) == [f"uf20-{i:03d}.cnf" for i in range(1, 6)]
    assert all(r["by"] in ("policy", "walksat") for r in g["results"])
    experts = load_expert_data(str(data), str(out))
    assert sorted(e["name"] for e in experts) == [f"uf20-{i:03d}.cnf" for i in range(1, 6)]
    for e in experts:
        _, nun = env._calculate_satisfaction_explicit(e["expert_solution"].astype(np.uint8), e["problem_clauses"])
        assert int(nun) == 0
    counts = verify_solutions_file(str(out / SOLUTIONS_FILE), str(data))
    assert counts == {"verified": 5, "failed": 0, "skipped": 0}

    # no finish and a single greedy 1-step try: whatever stays unsolved sets the exit status and gets no file
    out2 = tmp_path / "out2"
    rc2 = main(["--config", CFG, "--cnf-dir", str(data), "--sol-dir", str(out2), "--checkpoint", str(run_dir),
                "--rounds", "1", "--max-steps", "1", "--finish", "none", "--report", str(report)] + ov)
    rep2 = json.loads(report.read_text())
    assert rc2 == (1 if rep2["unsolved"] else 0)
    assert len(rep2["unsolved"]) >= 1  # a random network's one greedy step does not solve five uf20 formulas
    have = sorted(f for f in os.listdir(out2) if f.endswith(".sol"))
    assert have == sorted(n[:-4] + ".sol" for n in (f"uf20-{i:03d}.cnf" for i in range(1, 6)) if n not in rep2["unsolved"])
    counts2 = verify_solutions_file(str(out2 / SOLUTIONS_FILE), str(data))
    assert counts2["failed"] == 0 and counts2["skipped"] == len(rep2["unsolved"])

    # a missing checkpoint is an error, not a random network
    out3 = tmp_path / "out3"
    rc3 = main(["--config", CFG, "--cnf-dir", str(data), "--sol-dir", str(out3), "--checkpoint",
                str(tmp_path / "nowhere")] + ov)
    assert rc3 == 2 and "no checkpoint" in capsys.readouterr().err
    assert not os.path.exists(out3)
