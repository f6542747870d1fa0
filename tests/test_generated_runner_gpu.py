"""GPU: training on generated pools.  MAPPOLearner.set_pool swaps the pool under a learner (the policy's outputs are
then those of a fresh learner over the new pool, bitwise); the MAPPO runner with generation.ENABLED draws its
pools on the device, replaces the train pool every REFRESH_EVERY updates and writes the eval pool where
verify_solutions_file finds it; the device_generator tool writes .cnf / .sol pairs the directory-based tools read."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")
V, C = 12, 40


def _learner(pool, env, net, templates):
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner

    return MAPPOLearner(dict(NUM_ENVS=6, NUM_STEPS=2, MINIBATCH_SIZE=6), env, net, pool, templates=templates)


@pytest.mark.parametrize("templates", ["device", "host"])
def test_set_pool_equals_a_fresh_learner(templates):
    from marlsat import ProblemPool, SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.random import Key

    env = SATEnv(V, C, max_steps=8, vars_per_agent=4)
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, V, device="cuda", seed=3)
    pool1 = ProblemPool.generate((V, C, 2), 6, 1)
    pool2 = ProblemPool.generate((V, C, 2), 9, 2)
    assert not torch.equal(pool1.clauses, pool2.clauses[:6])
    swapped = _learner(pool1, env, net, templates)
    old_tpl = swapped.tpl
    swapped.set_pool(pool2)
    fresh = _learner(pool2, env, net, templates)
    assert swapped.pool is pool2 and swapped.tpl is not old_tpl and swapped.svf is pool2.static_var_features()
    assert (swapped.micro, swapped.chunk, swapped.actor_chunk) == (fresh.micro, fresh.chunk, fresh.actor_chunk)
    for f in ("vgid", "cgid", "slots", "ptr", "inc", "gv", "gc", "ge"):
        assert torch.equal(getattr(swapped.tpl, f), getattr(fresh.tpl, f)), f
    outs = []
    for lr in (swapped, fresh):
        rs = lr.init_runner_state(Key(5, 0))  # a state over the learner's current pool
        assert rs.env_state.pool is pool2
        for greedy in (False, True):
            outs.append(lr.policy(rs.env_state, Key(8, 1), greedy=greedy))
    for (a1, l1, v1), (a2, l2, v2) in zip(outs[:2], outs[2:]):
        assert torch.equal(a1, a2)
        assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
        assert torch.equal(v1.view(torch.int32), v2.view(torch.int32))
    with pytest.raises(ValueError, match="set_pool"):
        swapped.set_pool(ProblemPool.generate((V, C, 3), 4, 3))  # another clause width


def test_runner_trains_on_refreshed_generated_pools(tmp_path, monkeypatch):
    from marlsat import ProblemPool
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.runners.mappo_runner import load_config, run, verify_solutions_file
    from marlsat.utils.data_parser import parse_cnf
    from marlsat.utils.generation import eval_pool_key, train_pool_key

    ov = {"CNF_DATA_DIR": str(tmp_path / "no-such-dir"), "SAVE_DIR": str(tmp_path / "runs"), "SEED": 7,
          "environment.NUM_VARS": V, "environment.NUM_CLAUSES": C, "environment.VARS_PER_AGENT": 4,
          "environment.MAX_STEPS": 16, "network.GNN_HIDDEN_DIM": 64, "network.GNN_NUM_MESSAGE_PASSING_STEPS": 2,
          "training.NUM_ENVS": 4, "training.NUM_STEPS": 4, "training.NUM_UPDATES": 2, "training.UPDATE_EPOCHS": 1,
          "training.MINIBATCH_SIZE": 8, "evaluation.EVAL_INTERVAL": 1, "evaluation.EVAL_BATCH_SIZE": 2,
          "generation.ENABLED": "true", "generation.NUM_TRAIN": 16, "generation.NUM_EVAL": 4,
          "generation.REFRESH_EVERY": 1}
    seen = []
    real = MAPPOLearner.train_cycle

    def spy(self, rs, u, gen):
        assert rs.env_state.pool is self.pool and self.templates == "device"
        seen.append(self.pool.clauses.clone())
        return real(self, rs, u, gen)

    monkeypatch.setattr(MAPPOLearner, "train_cycle", spy)
    res = run(load_config(CFG, [f"{k}={v}" for k, v in ov.items()]), log=lambda *_: None)
    rd = res["run_dir"]
    lines = open(os.path.join(rd, "training_metrics.txt")).read().splitlines()
    assert len(lines) == 3 and all(np.isfinite([float(v) for v in l.split(",")]).all() for l in lines[1:])
    # a new train pool for the second update, each the pool of its key
    assert len(seen) == 2 and seen[0].shape == seen[1].shape == (16, C, 3) and not torch.equal(seen[0], seen[1])
    for e, cl in enumerate(seen):
        assert torch.equal(cl, ProblemPool.generate((V, C, 3), 16, train_pool_key(7, e)).clauses)
    assert res["train_pools"] == 2
    # the eval pool as files, read back to the pool
    gen_dir = os.path.join(rd, "generated_eval")
    assert res["generated_eval_dir"] == gen_dir
    names = sorted(os.listdir(gen_dir))
    assert names == [f"uf{V}-{i:03d}.cnf" for i in range(1, 5)]
    eval_cl = ProblemPool.generate((V, C, 3), 4, eval_pool_key(7)).clauses.cpu().numpy()
    for n, name in enumerate(names):
        v, c, cl = parse_cnf(os.path.join(gen_dir, name))
        assert (v, c) == (V, C)
        np.testing.assert_array_equal(np.asarray(cl, np.int32), eval_cl[n])
    sol = open(os.path.join(rd, "test_solutions.txt")).read().splitlines()
    assert len(sol) == 4 and all(l.startswith(f"Problem: uf{V}-") for l in sol)
    counts = verify_solutions_file(os.path.join(rd, "test_solutions.txt"), gen_dir)
    assert counts["failed"] == 0 and counts["verified"] + counts["skipped"] == 4


def test_device_generator_tool_writes_cnf_and_sol(tmp_path):
    from marlsat import SATEnv
    from marlsat.runners.behavioral_cloning import load_expert_data
    from marlsat.utils import device_generator
    from marlsat.utils.data_parser import load_cnf_problems

    cnf, sol = str(tmp_path / "cnf"), str(tmp_path / "sol")
    assert device_generator.main(["--num", "5", "--vars", "12", "--clauses", "40", "--seed", "9", "--cnf-dir", cnf,
                                  "--sol-dir", sol]) == 0
    assert sorted(os.listdir(cnf)) == [f"uf12-{i:03d}.cnf" for i in range(1, 6)]
    assert sorted(os.listdir(sol)) == [f"uf12-{i:03d}.sol" for i in range(1, 6)]
    probs = load_cnf_problems(cnf)
    assert all((p["num_vars"], p["num_clauses"]) == (12, 40) and len(p["clauses"][0]) == 3 for p in probs)
    experts = load_expert_data(cnf, sol)
    assert [e["name"] for e in experts] == [p["name"] for p in probs]
    env = SATEnv(12, 40, max_steps=1, vars_per_agent=4)
    for e in experts:
        assert e["expert_solution"].shape == (12,) and set(np.unique(e["expert_solution"])) <= {0, 1}
        _, nun = env._calculate_satisfaction_explicit(e["expert_solution"].astype(np.uint8), e["problem_clauses"])
        assert int(nun) == 0
    assert len({e["problem_clauses"].tobytes() for e in experts}) == 5
