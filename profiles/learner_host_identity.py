#!/usr/bin/env python3
"""Identity of the learners' host code (marlsat/learners/*_learner.py, base.py, params.py, utils/checkpoints.py)
across a refactor: the library calls the four learners issue, in order, and what they compute.  Run once per source
tree on the same built library, then compare (the method and the recorder of profiles/gnn_host_identity.py):

    MARLSAT_LIB=<libmarlsat.so> python profiles/learner_host_identity.py --tree <parent worktree> --out parent.json
    MARLSAT_LIB=<libmarlsat.so> python profiles/learner_host_identity.py --out tree.json
    python profiles/learner_host_identity.py --compare parent.json tree.json

`_lib.lib` is replaced by the recording proxy before any learner module binds it.  Per configuration the file keeps
the call trace (name, non-pointer arguments, pointer null-ness), sha256 of net.params, net.grads, adam_m and adam_v
(and of the tensors a configuration returns) after the run, and the returned metrics, floats by their repr.

Configurations, each the smallest at which a shared piece can go wrong (H 64, L 2):
  * MAPPO, action mode 0 (uf20-91, vars_per_agent 10) and mode 1 (V 16, C 60, vars_per_agent 4): NUM_ENVS 8,
    NUM_STEPS 4, MINIBATCH_SIZE 16, UPDATE_EPOCHS 2, a budget of 6 samples (micro-batches 6 + 6 + 4); one train_cycle,
    then with chunk = 3 (actor_chunk = 5) policy(greedy), policy(temperature 0.7, row_offset 5, actor-only, no critic)
    and critic_values on the 8 states the cycle ended in;
  * BC on the uf20-91 pool: 37 samples, MINIBATCH_SIZE 16 (a last minibatch of 5), a budget of 8 samples, one epoch
    on full batches and one on actor-only batches;
  * single-agent PPO: V 20, C 91, NUM_ENVS 4, NUM_STEPS 6, NUM_MINIBATCHES 3, UPDATE_EPOCHS 2, a budget of 4 samples;
    one train_cycle and one evaluate of 5 instances at max_steps 6;
  * assignment predictor: 37 samples, BATCH_SIZE 16, a budget of 8 samples; train_epoch on 25 of the rows, evaluate
    on the other 12, predict(slab = 5) on all;
  * checkpoints: sha256 of to_bytes(train_state_dict(net)) of the mode-0 MAPPO net and of the single-agent net after
    their runs (a tree that still has single_train_state_dict takes the single net's through it).

There is no --dry: the learners read device totals back, so a run without a GPU has nothing to plan from.
"""
import hashlib
import os
import sys

from gnn_host_identity import Recorder, compare, main, sha

H, L = 64, 2
NAME = "learner_host_identity"


def canon(v):
    """Metrics as JSON that compares exactly: floats by repr (NaN equals NaN), arrays as lists of them."""
    import numpy as np

    if isinstance(v, dict):
        return {k: canon(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return [canon(x) for x in v.ravel().tolist()]
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    return int(v) if isinstance(v, (bool, int, np.integer)) else v


def run(tree, dry):
    if dry:
        sys.exit(f"{NAME}: no --dry (see the module docstring)")
    sys.path[:0] = [tree, os.path.join(tree, "marl-sat_amd")]
    import numpy as np
    import torch

    from marlsat import _lib

    rec = _lib.lib = Recorder(_lib.lib, False)
    from marlsat import SATEnv
    from marlsat.learners import assign_learner, bc_learner, mappo_gnn_sat_learner, single_ppo_learner
    from marlsat.learners.assign_gnn import GNNAssignmentPredictor
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.graphs import DeviceTemplates, build_templates
    from marlsat.learners.single_gnn import GNNSingleActorCritic
    from marlsat.random import PRNGKey
    from marlsat.utils import checkpoints as ck
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    for m in (assign_learner, bc_learner, mappo_gnn_sat_learner, single_ppo_learner):
        assert m.L_ is rec, f"{m.__name__} was imported before the proxy was in place"

    def budget(samples, rows):
        """An activation budget of ``samples`` training samples of ``rows`` graph rows (activation_plan)."""
        return (samples + 0.5) * (4.0 * L * rows * 12 * H + 4.0 * rows * 24 * H)

    def rows_of(pool, V, A):
        t = DeviceTemplates(build_templates(pool, V, A), A, "cuda")
        return {"full": t.mean_full_rows, "actor": t.mean_actor_rows, "graph0": t.mean_full_rows - t.mean_actor_rows}

    configs = {}

    def config(name, net, f):
        """Run f() -> (tensors to hash, metrics) as configuration ``name``."""
        rec.cut()
        tensors, metrics = f()
        torch.cuda.synchronize()
        calls = rec.cut()
        tensors = dict(tensors, params=net.params, grads=net.grads, adam_m=net.adam_m, adam_v=net.adam_v)
        configs[name] = {"sha256": {k: sha(t) for k, t in tensors.items()}, "metrics": canon(metrics),
                         "calls": len(calls), "trace": [rec.index[c] for c in calls]}
        print(f"{name}: {len(calls)} calls", file=sys.stderr, flush=True)

    def state_sha(net, single=False):
        f = getattr(ck, "single_train_state_dict", ck.train_state_dict) if single else ck.train_state_dict
        return hashlib.sha256(ck.to_bytes(f(net))).hexdigest()

    pool20 = generate_problem_pool(20, 91, 6, size_id=11, skip_isolated=True)
    ckpt = {}

    # ---- MAPPO ----
    for mode, (V, C, vpa), pool in ((0, (20, 91, 10), pool20),
                                    (1, (16, 60, 4), generate_problem_pool(16, 60, 6, size_id=11, skip_isolated=True))):
        cfg = dict(NUM_ENVS=8, NUM_STEPS=4, NUM_UPDATES=10, UPDATE_EPOCHS=2, MINIBATCH_SIZE=16, LEARNING_RATE=3e-3,
                   GAMMA=0.995, GAE_LAMBDA=0.95, CLIP_EPS=0.12, ENT_COEF=0.005, VF_COEF=0.5, VF_CLIP=0.5,
                   ANNEAL_LR=True, LR_START_FACTOR=1.0, LR_END_FLOOR=2e-5, GNN_HIDDEN_DIM=H,
                   GNN_NUM_MESSAGE_PASSING_STEPS=L, action_mode=mode)
        env = SATEnv(V, C, max_steps=3, vars_per_agent=vpa, action_mode=mode)
        net = GNNActorCritic(H, L, env.num_agents, env.max_vars_per_agent, mode, V, device="cuda", seed=3)
        mb = budget(6, rows_of(pool, V, env.num_agents)["full"])
        box = {}

        def cycle():
            lr = box["lr"] = mappo_gnn_sat_learner.MAPPOLearner(cfg, env, net, env.make_pool(pool), micro_bytes=mb)
            assert lr.micro == 6, lr.micro  # 16 rows as 6 + 6 + 4
            rs = lr.init_runner_state(PRNGKey(0))
            box["rs"], metrics = lr.train_cycle(rs, 0, torch.Generator().manual_seed(123))
            return dict(lr.tr, adv=lr.adv, targets=lr.targets, last_val=lr.last_val), metrics

        def inference():
            lr, st = box["lr"], box["rs"].env_state
            lr.chunk, lr.actor_chunk = 3, 5
            a0, l0, v0 = lr.policy(st, PRNGKey(7), greedy=True)
            a1, l1, _ = lr.policy(st, PRNGKey(8), temperature=0.7, row_offset=5, actor_only=True, critic=False)
            cv = lr.critic_values(st.problem_idx, st.variable_assignments)
            return {"greedy_act": a0, "greedy_logp": l0, "greedy_val": v0, "temp_act": a1, "temp_logp": l1,
                    "critic_values": cv}, {}

        config(f"mappo mode {mode} train_cycle", net, cycle)
        config(f"mappo mode {mode} policy + critic_values", net, inference)
        if mode == 0:
            ckpt["mappo"] = state_sha(net)

    # ---- BC ----
    V, C, vpa, N = 20, 91, 10, 37
    rng = np.random.default_rng(5)
    pidx = rng.integers(0, len(pool20), N).astype(np.int32)
    x = rng.integers(0, 2, (N, V)).astype(np.uint8)
    env = SATEnv(V, C, max_steps=4, vars_per_agent=vpa)
    A, M = env.num_agents, env.max_vars_per_agent
    labels = np.where(rng.integers(0, 2, (N, A)) == 1, 0, M).astype(np.int32)  # the agent's first variable or the no-op
    rows = rows_of(pool20, V, A)
    for actor_only in (False, True):
        net = GNNActorCritic(H, L, A, M, 0, V, device="cuda", seed=4)

        def epoch():
            lr = bc_learner.BCLearner(dict(MINIBATCH_SIZE=16, LEARNING_RATE=3e-3), env, net, env.make_pool(pool20),
                                      micro_bytes=budget(8, rows["actor" if actor_only else "full"]),
                                      actor_only=actor_only)
            assert lr.micro == 8, lr.micro
            lr.set_data(pidx, x, labels)
            out = lr.train_epoch(torch.Generator().manual_seed(7))
            return {}, dict(out, minibatch_losses=lr.minibatch_losses)

        config(f"bc actor_only={int(actor_only)} train_epoch", net, epoch)

    # ---- single-agent PPO ----
    cfg = dict(NUM_ENVS=4, NUM_STEPS=6, NUM_MINIBATCHES=3, UPDATE_EPOCHS=2, NUM_CYCLES=1, LR=3e-3, ANNEAL_LR=True,
               GAMMA=0.99, GAE_LAMBDA=0.95, CLIP_EPS=0.2, VF_COEF=0.5, ENT_COEF=0.01)
    env = single_ppo_learner.make_single_env(V, C, 6, 2.5)
    net = GNNSingleActorCritic(H, L, V, device="cuda", seed=4)
    box = {}

    def cycle():
        lr = box["lr"] = single_ppo_learner.SinglePPOLearner(cfg, env, net, env.make_pool(pool20),
                                                             micro_bytes=budget(4, V + C))
        assert (lr.MB, lr.micro) == (8, 4), (lr.MB, lr.micro)
        _, stats = lr.train_cycle(lr.init_runner_state(PRNGKey(5)), torch.Generator().manual_seed(7))
        return dict(lr.tr, adv=lr.adv, targets=lr.targets, last_val=lr.last_val), dict(
            stats, minibatch_terms=lr.minibatch_terms, grad_norms=lr.grad_norms)

    def evaluate():
        lr = box["lr"]
        out = lr.evaluate([0, 1, 2, 3, 0], 6, key=PRNGKey(3))
        return {}, dict(out, **{f"episodes_{k}": np.asarray(v, np.float64) for k, v in lr.eval_episodes.items()})

    config("single train_cycle", net, cycle)
    config("single evaluate", net, evaluate)
    ckpt["single"] = state_sha(net, single=True)

    # ---- assignment predictor ----
    labels = rng.integers(0, 2, (N, V)).astype(np.uint8)
    order = rng.permutation(N).astype(np.int32)
    net = GNNAssignmentPredictor(H, L, device="cuda", seed=4)
    env = SATEnv(V, C, max_steps=4, vars_per_agent=V)
    box = {}

    def make():
        lr = box["lr"] = assign_learner.AssignLearner(dict(BATCH_SIZE=16, LEARNING_RATE=1e-3), net,
                                                      env.make_pool(pool20), micro_bytes=budget(8, V + C))
        assert lr.micro == 8, lr.micro
        lr.set_data(pidx, x, labels)
        out = lr.train_epoch(torch.Generator().manual_seed(7), rows=order[:25])
        return {}, dict(out, minibatch_losses=lr.minibatch_losses, minibatch_accs=lr.minibatch_accs)

    def evaluate():
        lr = box["lr"]
        out = lr.evaluate(order[25:])
        return {}, dict(out, minibatch_losses=lr.minibatch_losses, minibatch_accs=lr.minibatch_accs)

    def predict():
        pred, unsat, solved = box["lr"].predict(pidx, x, slab=5)
        return {"pred": pred, "unsat": unsat, "solved": solved}, {}

    config("assign train_epoch", net, make)
    config("assign evaluate", net, evaluate)
    config("assign predict", net, predict)

    configs["checkpoints"] = {"sha256": ckpt, "metrics": {}, "calls": 0, "trace": []}
    return {"dry": False, "call_table": rec.calls, "configs": configs}


def compare_learners(pa, pb):
    compare(pa, pb, keys=("sha256", "metrics", "calls"), tool=NAME,
            what="traces, parameter / gradient / Adam / output / checkpoint hashes and metrics")


if __name__ == "__main__":
    main(run, compare_learners, __doc__, NAME)
