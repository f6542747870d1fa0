"""GPU: the policy solver on actor-only graph batches (policy_search / solve_pool_with_policy(actor_only=True),
python -m marlsat.utils.policy_solver --actor-only) returns what the full-batch path returns, field for field:
uf20-91, six instances, H = 64, L = 2, at most 16 steps.  The learner's chunks are set small and unequal (4 full,
5 actor-only) so that the 12-row searches span several chunks: a sampled search without row_offset has the chunk
index in its Philox counter and must keep the full path's chunk; greedy and row_offset searches may use the other."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")
RECORD = ("prev_x", "best_x", "best_unsat", "best_step", "first_solve", "flips", "unsolved")


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
    assert lr.actor_chunk >= lr.chunk  # the same budget over fewer rows
    lr.chunk, lr.actor_chunk = 4, 5
    return clauses, env, pool, lr


def _spy_batches(lr, monkeypatch):
    """Record (g0, G, S) of every graph batch the learner assembles."""
    seen = []
    real = lr._batch

    def spy(*a, **kw):
        b = real(*a, **kw)
        seen.append((b.g0, b.G, b.S))
        return b

    monkeypatch.setattr(lr, "_batch", spy)
    return seen


@pytest.mark.parametrize("greedy,temperature,row_offset", [(True, 1.0, None), (False, 0.7, None), (False, 0.7, 24)],
                         ids=["greedy", "t0.7", "t0.7-row_offset"])
def test_policy_search_record_equals_full_batch(pool6, greedy, temperature, row_offset, monkeypatch):
    from marlsat.random import Key
    from marlsat.solvers.policy import policy_search

    clauses, env, pool, lr = pool6
    pidx = np.repeat(np.arange(6, dtype=np.int32), 2)
    kw = dict(greedy=greedy, temperature=temperature, early_exit=False, row_offset=row_offset)
    tr_full, tr_act = [], []
    full = policy_search(lr, pool, pidx, 12, Key(11, 3), trace=tr_full, **kw)
    seen = _spy_batches(lr, monkeypatch)
    act = policy_search(lr, pool, pidx, 12, Key(11, 3), trace=tr_act, actor_only=True, **kw)
    A = env.num_agents
    chunk = 5 if (greedy or row_offset is not None) else 4
    sizes = [min(chunk, 12 - b0) for b0 in range(0, 12, chunk)]
    assert seen == [(1, A, S) for S in sizes] * 12  # actor-only batches, the chunk the counter allows
    assert act.steps_run == full.steps_run == 12
    for f in RECORD:
        assert torch.equal(getattr(act, f), getattr(full, f)), f
    assert len(tr_act) == len(tr_full) == 13
    for t, (a, b) in enumerate(zip(tr_act, tr_full)):
        assert torch.equal(a, b), f"trace entry {t}"
    assert (full.flips > 0).any()  # the searches moved


def test_policy_requires_no_critic_for_actor_only(pool6):
    from marlsat.random import Key

    clauses, env, pool, lr = pool6
    _, st = env.reset_from_pool(pool, 6, Key(1, 0), with_obs=False)
    with pytest.raises(ValueError, match="critic=False"):
        lr.policy(st, Key(2, 0), actor_only=True)
    a0, l0, _ = lr.policy(st, Key(2, 0), critic=False)
    a1, l1, _ = lr.policy(st, Key(2, 0), critic=False, actor_only=True)
    assert torch.equal(a0, a1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))


@pytest.mark.parametrize("max_batch", [4096, 7], ids=["one-slab", "three-slabs"])
def test_pool_solve_equals_default(pool6, max_batch):
    """max_batch = 7 with tries = 3: the sampled round runs two instances per slab, three slabs when the greedy
    round solved none of the six."""
    from marlsat.random import Key
    from marlsat.solvers.policy import solve_pool_with_policy

    clauses, env, pool, lr = pool6
    kw = dict(tries=3, rounds=2, max_steps=16, temperature=0.7, finish_tries=8, finish_flips=20_000, noise=0.5,
              key=Key(5, 0))
    want = solve_pool_with_policy(lr, pool, **kw)
    got = solve_pool_with_policy(lr, pool, max_batch=max_batch, actor_only=True, **kw)
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert want["solved"].all() and (want["round"] >= 0).all()


def test_cli_actor_only_writes_the_same_files_and_report(tmp_path):
    from marlsat import SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.utils import checkpoints as ck
    from marlsat.utils.generate_cnf_dataset import generate_cnf_dataset_sat
    from marlsat.utils.policy_solver import SOLUTIONS_FILE, main

    data, run_dir = tmp_path / "data", tmp_path / "run"
    generate_cnf_dataset_sat(5, 20, 91, str(data), seed=5)
    env = SATEnv(20, 91, max_steps=16, vars_per_agent=10)
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, 20, device="cuda", seed=4)
    ck.save_checkpoint(str(run_dir / "checkpoints"), ck.train_state_dict(net), 0, "latest_model_")
    ov = ["environment.NUM_VARS=20", "environment.NUM_CLAUSES=91", "environment.VARS_PER_AGENT=10",
          "environment.MAX_STEPS=16", "network.GNN_HIDDEN_DIM=64", "network.GNN_NUM_MESSAGE_PASSING_STEPS=2"]
    reports, files = [], []
    for flag in ([], ["--actor-only"]):
        out, rep = tmp_path / f"out{len(flag)}", tmp_path / f"report{len(flag)}.json"
        rc = main(["--config", CFG, "--cnf-dir", str(data), "--sol-dir", str(out), "--checkpoint", str(run_dir),
                   "--tries", "3", "--rounds", "2", "--temperature", "0.7", "--finish-flips", "20000", "--max-batch",
                   "64", "--report", str(rep)] + flag + ov)
        assert rc == 0
        reports.append(json.loads(rep.read_text()))
        files.append({f: (out / f).read_bytes() for f in sorted(os.listdir(out))})
    assert sorted(files[0]) == sorted([f"uf20-{i:03d}.sol" for i in range(1, 6)] + [SOLUTIONS_FILE])
    assert files[1] == files[0]
    for k in ("checkpoint", "checkpoint_kind", "cnf_dir", "groups", "skipped", "unsolved"):
        assert reports[1][k] == reports[0][k], k
    assert set(reports[0]) == set(reports[1])
