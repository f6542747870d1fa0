"""GPU: BCLearner(actor_only=True) -- micro-batches of the agents' graphs alone, back-propagated with no value
gradient -- against the float64 oracle, at the bars of tests/test_bc_learner_gpu.py's
test_every_adam_step_matches_oracle (its helpers, imported): the loss 1e-5 relative, gradients 1e-4 normwise and
elementwise 1e-5 |ref| + GRAD_FACTOR x E32 + kink, every Adam step against optax's formula in float64.  One regular
shape (a padded agent slot) and the irregular 2-wide learner pool, each with one micro-batch per minibatch and
with several.  The critic head's parameters must not move by a bit."""
import numpy as np
import pytest
import torch

from test_bc_learner_gpu import _cfg, _check_trace, _dataset, precision_path  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

REGULAR = (23, 97, 10, 64, 2)  # agents of 8, 8 and 7 variables: a padded slot, a -inf logit
IRREGULAR = (12, 40, 4, 64, 2)  # tests/irregular_pools.learner_pool: literal 0, [v, v] and [v, -v] rows


def _learner(shape, MB, n, pool=None, micro_samples=None, actor_only=True):
    from marlsat import SATEnv
    from marlsat.learners.bc_learner import BCLearner
    from marlsat.learners.gnn import GNNActorCritic

    V, C, vpa, H, L = shape
    clauses, pidx, x, labels, ora = _dataset(V, C, vpa, pool=pool)
    env = SATEnv(V, C, max_steps=4, vars_per_agent=vpa)
    net = GNNActorCritic(H, L, env.num_agents, env.max_vars_per_agent, 0, V, device="cuda", seed=4)
    dpool = env.make_pool(clauses)
    budget = None
    if micro_samples is not None:  # an activation budget of micro_samples actor-only samples (activation_plan)
        from marlsat.learners.graphs import DeviceTemplates, build_templates

        rows = DeviceTemplates(build_templates(clauses, V, env.num_agents), env.num_agents, "cuda").mean_actor_rows
        budget = (micro_samples + 0.5) * (4.0 * L * rows * 12 * H + 4.0 * rows * 24 * H)
    learner = BCLearner(_cfg(H, L, MB), env, net, dpool, micro_bytes=budget, actor_only=actor_only)
    learner.set_data(pidx[:n], x[:n], labels[:n])
    return learner, net


def _run_and_check(shape, MB, sizes, micro, tag, pool=None, micro_samples=None):
    from marlsat.learners import graphs

    learner, net = _learner(shape, MB, 7, pool=pool, micro_samples=micro_samples)
    assert learner.actor_only and learner.micro == micro
    assert learner.tpl.mean_actor_rows < learner.tpl.mean_full_rows
    seen = []
    real = graphs.assemble

    def spy(*a, **kw):
        b = real(*a, **kw)
        seen.append((b.g0, b.G, b.S))
        return b

    import marlsat.learners.base as bcl  # the learners' one assemble call (Learner._batch)

    learner.trace = []
    p0 = net.to_flax()
    orig, bcl.assemble = bcl.assemble, spy
    try:
        out = learner.train_epoch(torch.Generator().manual_seed(7))
    finally:
        bcl.assemble = orig
    assert [len(r["idx"]) for r in learner.trace] == sizes
    # every micro-batch was an actor-only batch of at most `micro` samples
    assert seen and all(g0 == 1 and G == net.A and S <= micro for g0, G, S in seen)
    assert sum(S for _, _, S in seen) == 7 and len(seen) == sum(-(-s // micro) for s in sizes)
    assert np.isfinite(out["loss"]) and 0.0 <= out["accuracy"] <= 1.0
    _check_trace(learner, net, shape, tag, pool=pool)
    p1 = net.to_flax()
    critic = [k for k in p0 if k.startswith("critic")]
    assert critic and len(critic) < len(p0)
    bits = lambda a: np.asarray(a, np.float32).view(np.int32)
    for k in critic:
        assert np.array_equal(bits(p0[k]), bits(p1[k])), k
    for rec in learner.trace:  # and its gradient is exactly zero at every step
        g = {k: v for k, v in _unflat_grads(net, rec["grads"]).items() if k.startswith("critic")}
        assert g and not any(np.asarray(v).any() for v in g.values())
    moved = [k for k in p0 if not np.array_equal(bits(p0[k]), bits(p1[k]))]
    assert {k.split("/")[0].split("_")[0] for k in moved} >= {"encoder", "actor", "agent"}


def _unflat_grads(net, flat):
    from marlsat.learners import params as Pm

    return Pm.to_flax(flat.detach().cpu().numpy(), net.H, net.L, net.A, net.M, net.mode, net.E)


@pytest.mark.parametrize("precision_path", ["fp16x2", "bf16x3", "fp32"], indirect=True)
def test_actor_only_adam_steps_match_oracle(precision_path):
    """N = 7 in minibatches of 3, each one micro-batch: three Adam steps, the last on a single sample."""
    _run_and_check(REGULAR, 3, [3, 3, 1], 3, f"actor-only {precision_path} V23")


@pytest.mark.parametrize("precision_path", ["fp16x2", "bf16x3", "fp32"], indirect=True)
def test_actor_only_micro_batches_match_oracle(precision_path):
    """A budget of 2 actor-only samples: minibatches of 4 and 3 run as micro-batches of 2 + 2 and 2 + 1."""
    _run_and_check(REGULAR, 4, [4, 3], 2, f"actor-only micro {precision_path} V23", micro_samples=2)


def test_actor_only_adam_steps_match_oracle_on_an_irregular_pool():
    _run_and_check(IRREGULAR, 3, [3, 3, 1], 3, "actor-only irregular V12", pool="learner")


def test_actor_only_micro_batches_match_oracle_on_an_irregular_pool():
    _run_and_check(IRREGULAR, 4, [4, 3], 2, "actor-only micro irregular V12", pool="learner", micro_samples=2)


def test_runner_reads_the_actor_only_switch(tmp_path, monkeypatch):
    """bc_training.ACTOR_ONLY_GRAPHS reaches the learner the runner builds (default: the full batch)."""
    from marlsat.learners import bc_learner
    from marlsat.runners import behavioral_cloning as bcr
    from marlsat.utils.generate_cnf_dataset import generate_cnf_dataset_sat

    V, C = 20, 91
    cnf, sol = str(tmp_path / "cnf"), str(tmp_path / "sol")
    generate_cnf_dataset_sat(2, V, C, cnf, seed=1, sol_dir=sol)
    built = []
    init = bc_learner.BCLearner.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        built.append(self.actor_only)

    monkeypatch.setattr(bc_learner.BCLearner, "__init__", spy)
    for flag in (None, True):
        bc = {"NUM_SAMPLES_PER_EXPERT": 2, "SOL_DATA_DIR": sol, "SAVE_PATH": str(tmp_path / f"bc{flag}")}
        if flag is not None:
            bc["ACTOR_ONLY_GRAPHS"] = flag
        config = {"SEED": 3, "CNF_DATA_DIR": cnf,
                  "environment": {"NUM_VARS": V, "NUM_CLAUSES": C, "MAX_STEPS": 2, "VARS_PER_AGENT": 10,
                                  "action_mode": 0},
                  "network": {"GNN_HIDDEN_DIM": 64, "GNN_NUM_MESSAGE_PASSING_STEPS": 2},
                  "training": {"NUM_UPDATES": 1, "MINIBATCH_SIZE": 4, "LEARNING_RATE": 1e-3, "NUM_ENVS": 2,
                               "NUM_STEPS": 2},
                  "bc_training": bc}
        res = bcr.run(config, log=lambda *_: None)
        assert res["num_samples"] == 4 and np.isfinite(res["last_epoch"]["loss"])
    assert built == [False, True]
