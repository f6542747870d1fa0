"""GPU: the assignment predictor's runner (runners/bc_runner.py) end to end on planted uf20-91 files, and the
predictor as WalkSAT's start (solvers/walksat.solve_pool(init_assignments=...), utils/sat_solver --init-model)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

CONFIG = os.path.join(ROOT, "configs", "ASSIGN_BC_CONFIG.yaml")
LINE = re.compile(r"Epoch (\d{3}) \| Train Loss: ([\d.]+), Train Var-Acc: ([\d.]+), Train Sol-Acc: ([\d.]+) \| "
                  r"Val Loss: ([\d.]+), Val Var-Acc: ([\d.]+), Val Sol-Acc: ([\d.]+)")


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Two epochs on 10 planted uf20-91 files: (run result, cnf dir, sol dir)."""
    from marlsat.runners.bc_runner import load_config, run
    from marlsat.utils.generate_cnf_dataset import generate_cnf_dataset_sat

    tmp = tmp_path_factory.mktemp("assign")
    cnf, sol = str(tmp / "uf20-91"), str(tmp / "uf20-91-answer")
    generate_cnf_dataset_sat(10, 20, 91, cnf, seed=5, sol_dir=sol)
    lines = []
    res = run(load_config(CONFIG, [f"CNF_DATA_DIR={cnf}", f"SOL_DATA_DIR={sol}", f"SAVE_DIR={tmp / 'runs'}", "EPOCHS=2",
                                   "BATCH_SIZE=4", "network.H=64", "network.L=2", "LEARNING_RATE=0.001"]),
              log=lines.append)
    return res, cnf, sol, lines


def test_runner_logs_checkpoints_and_describes_its_model(trained):
    from marlsat.learners import params as Pm
    from marlsat.runners.bc_runner import load_predictor
    from marlsat.utils import checkpoints as ck

    res, cnf, sol, lines = trained
    with open(res["log_path"]) as f:
        logged = f.read().splitlines()
    assert len(logged) == 2
    for e, line in enumerate(logged, 1):
        m = LINE.fullmatch(line)
        assert m and int(m.group(1)) == e and line in lines
        tr, va = res["history"][e - 1]
        assert float(m.group(2)) == pytest.approx(tr["loss"], abs=5e-5)
        assert float(m.group(7)) == pytest.approx(va["sol_acc"], abs=5e-5)
        assert 0.0 < tr["loss"] < 2.0 and 0.0 <= tr["var_acc"] <= 1.0 and 0.0 <= va["sol_acc"] <= 1.0
    assert len(res["train_instances"]) == 8 and len(res["val_instances"]) == 2
    # epoch 1's Sol-Acc (>= 0) beats the initial -1: a best_<epoch> exists, exactly one
    best = os.listdir(res["ckpt_dir"])
    assert best == [f"best_{res['best_epoch']}"] and res["best_epoch"] >= 1
    with open(os.path.join(res["run_dir"], "assign_model.json")) as f:
        desc = json.load(f)
    assert (desc["H"], desc["L"], desc["INPUT"]) == (64, 2, "zeros")
    # the checkpoint is the parameter tree alone, and loads back bitwise
    tree = ck.restore_checkpoint(res["ckpt_dir"], "best_", None)
    assert set(tree) == {"encoder", "assign_dense_0", "assign_dense_1", "assign_output"}
    net, desc2 = load_predictor(res["run_dir"])
    assert desc2 == desc
    again = Pm.assign_to_flax(net.params.cpu().numpy(), 64, 2)
    flat = ck.flatten(tree)
    assert set(again) == set(flat) and all(np.array_equal(again[k].view(np.int32), flat[k].view(np.int32)) for k in flat)
    if res["best_epoch"] == 2:  # the final parameters are then the saved ones
        assert torch.equal(net.params.view(torch.int32), res["network"].params.view(torch.int32))


def _planted_pool(n, V=20, C=91, base=7700):
    from marlsat import SATEnv
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses, generate_sat_solution

    cl = np.stack([generate_sat_clauses(V, C, 3, base + i) for i in range(n)])
    sols = np.stack([generate_sat_solution(V, base + i) for i in range(n)]).astype(np.uint8)
    return SATEnv(V, C, max_steps=1, vars_per_agent=V).make_pool(cl), cl, sols


def test_solve_pool_from_planted_solutions_and_without_the_keyword():
    from marlsat.random import PRNGKey
    from marlsat.solvers.walksat import solve_pool

    pool, cl, sols = _planted_pool(6)
    kw = dict(tries=3, max_flips=2000, max_rounds=3, key=PRNGKey(9))
    warm = solve_pool(pool, init_assignments=sols, **kw)
    assert warm["solved"].all() and (warm["round"] == 0).all() and (warm["flips"] == 0).all()
    assert (warm["try"] == 0).all() and np.array_equal(warm["solution"], sols)
    warm_dev = solve_pool(pool, init_assignments=torch.from_numpy(sols).cuda(), **kw)
    plain, none = solve_pool(pool, **kw), solve_pool(pool, init_assignments=None, **kw)
    assert set(plain) == set(none) == set(warm) == {"solved", "solution", "flips", "round", "try"}
    for k in plain:
        assert np.array_equal(plain[k], none[k]) and plain[k].dtype == none[k].dtype, k
        assert np.array_equal(warm[k], warm_dev[k]), k
    assert plain["solved"].all() and (plain["flips"] > 0).any()  # a random start is not a solution
    # a start one flip away from the planted solution: round 0 still begins there (few flips), later rounds are random
    near = sols.copy()
    near[:, 3] ^= 1
    close = solve_pool(pool, init_assignments=near, **kw)
    assert close["solved"].all() and (close["round"] == 0).all() and close["flips"].mean() < plain["flips"].mean()
    with pytest.raises(ValueError, match="init_assignments"):
        solve_pool(pool, init_assignments=sols[:, :5], **kw)


def test_solve_directory_with_a_predictor_on_two_sizes(trained, tmp_path):
    from marlsat import SATEnv
    from marlsat.random import PRNGKey
    from marlsat.runners.bc_runner import load_predictor
    from marlsat.utils.data_parser import group_problems, load_cnf_problems
    from marlsat.utils.generate_cnf_dataset import generate_cnf_dataset_sat
    from marlsat.utils.sat_solver import predicted_starts, sol_path, solve_directory

    res = trained[0]
    mixed, out = str(tmp_path / "mixed"), str(tmp_path / "sols")
    generate_cnf_dataset_sat(4, 20, 91, mixed, seed=11)
    generate_cnf_dataset_sat(3, 13, 50, mixed, seed=12)
    logs = []
    got = solve_directory(mixed, out, init_model=res["run_dir"], tries=4, max_flips=5000, max_rounds=3,
                          key=PRNGKey(2), log=logs.append)
    assert len(got["solved"]) + len(got["unsolved"]) == 7 and len(got["solved"]) >= 1
    assert len(logs) == 2 and all("the prediction alone solved" in l and "round 0" in l for l in logs)
    groups = group_problems(load_cnf_problems(mixed))
    assert sorted(groups) == [(13, 50), (20, 91)]
    net, desc = load_predictor(res["run_dir"])  # one checkpoint, both sizes
    for (V, C), g in groups.items():
        env = SATEnv(V, C, max_steps=1, vars_per_agent=V)
        pred = predicted_starts(net, desc, env.make_pool(g["clauses"]), PRNGKey(2))[0].cpu().numpy()
        for name, row, cl in zip(g["names"], pred, g["clauses"]):
            assert np.array_equal(got["starts"][name], row), name  # round 0 started from predict's output
            path = sol_path(out, name)
            assert os.path.exists(path) == (name in got["solved"])
            if name in got["solved"]:
                with open(path) as f:
                    x = np.array([int(v) for v in f.readline().split()], np.uint8)
                _, nun = env._calculate_satisfaction_explicit(x[None], cl[None])
                assert x.shape == (V,) and int(nun) == 0, name
