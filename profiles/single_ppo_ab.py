"""One agent over all V variables, trained two ways (run on the GPU from the repo root):

    python profiles/single_ppo_ab.py [--envs 64] [--steps 8] [--pool 64] [--alternations 3] [--out FILE]

A ``SinglePPOLearner`` cycle (learners/single_ppo_learner.py: one shared encoder pass per sample, critic-only graph
batches) against a ``MAPPOLearner`` cycle at ``vars_per_agent = V`` -- the only way to train one agent without the
single-agent learner: that run encodes graph 0 for the critic and the single agent's graph (all variables again) for
the actor, carries a no-op slot, and evaluates the critic once more for its metrics.

Shapes uf50-218 and uf100-430, H = 128, L = 16, the same NUM_ENVS, NUM_STEPS, UPDATE_EPOCHS and minibatch count on
both sides, one device-generated pool per shape, randomly initialised networks (the time of a cycle does not depend
on the parameters).  After one untimed cycle of each the two are alternated --alternations times; a timing is wall
clock around ``train_cycle`` with a device synchronisation before and after; samples/s = NUM_ENVS * NUM_STEPS / it.

The shared encoder halves the graph rows per sample, so about half the time per sample is the expectation; it is
recorded beside the measurement (``predicted_ratio``) and is no pass bar.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-sat_amd")]

SHAPES = {"uf50-218": (50, 218), "uf100-430": (100, 430)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--minibatches", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from marlsat import ProblemPool, SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.learners.single_gnn import GNNSingleActorCritic
    from marlsat.learners.single_ppo_learner import SinglePPOLearner, make_single_env
    from marlsat.random import PRNGKey

    if not torch.cuda.is_available():
        raise SystemExit("single_ppo_ab: no GPU; nothing is measured on the CPU")
    B, T, E, K = args.envs, args.steps, args.epochs, args.minibatches
    N = B * T
    if N % K:
        raise SystemExit(f"--envs * --steps = {N} must be divisible by --minibatches = {K}")
    H, L = args.hidden, args.layers
    result = {"envs": B, "steps": T, "epochs": E, "minibatches": K, "pool": args.pool, "hidden": H, "layers": L,
              "alternations": args.alternations, "device": torch.cuda.get_device_name(0), "shapes": {}}
    common = dict(NUM_ENVS=B, NUM_STEPS=T, UPDATE_EPOCHS=E, GAMMA=0.99, GAE_LAMBDA=0.95, CLIP_EPS=0.2, ENT_COEF=0.01,
                  VF_COEF=0.5, ANNEAL_LR=False)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name, (V, C) in SHAPES.items():
        max_steps = 8 * T  # no time-out inside a cycle on either side
        senv = make_single_env(V, C, max_steps, 5.0)
        pool = ProblemPool.generate(senv, args.pool, PRNGKey(V))
        snet = GNNSingleActorCritic(H, L, V, device="cuda", seed=1)
        single = SinglePPOLearner(dict(common, NUM_MINIBATCHES=K, NUM_CYCLES=1000, LR=1e-4), senv, snet, pool)
        menv = SATEnv(V, C, max_steps, vars_per_agent=V)
        mnet = GNNActorCritic(H, L, menv.num_agents, menv.max_vars_per_agent, 0, V, device="cuda", seed=1)
        mappo = MAPPOLearner(dict(common, MINIBATCH_SIZE=N // K, NUM_UPDATES=1000, LEARNING_RATE=1e-4, VF_CLIP=0.2,
                                  GNN_HIDDEN_DIM=H, GNN_NUM_MESSAGE_PASSING_STEPS=L, action_mode=0), menv, mnet, pool)
        assert menv.num_agents == 1
        state = {"s": single.init_runner_state(PRNGKey(3)), "m": mappo.init_runner_state(PRNGKey(3)), "u": 0}
        gs, gm = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)

        def cycle_single():
            state["s"], _ = single.train_cycle(state["s"], gs)

        def cycle_mappo():
            state["m"], _ = mappo.train_cycle(state["m"], state["u"], gm)
            state["u"] += 1

        timed(cycle_single)  # untimed pass of each
        timed(cycle_mappo)
        rs, rm = [], []
        for _ in range(args.alternations):
            rs.append(N / timed(cycle_single))
            rm.append(N / timed(cycle_mappo))
            print(f"{name}: single {rs[-1]:.1f} samples/s, MAPPO at vars_per_agent = V {rm[-1]:.1f} samples/s",
                  file=sys.stderr, flush=True)
        rows_single = single.tpl.mean_full_rows - single.tpl.mean_actor_rows
        rows_mappo = mappo.tpl.mean_full_rows
        ms, mm = statistics.median(rs), statistics.median(rm)
        result["shapes"][name] = {
            "num_vars": V, "num_clauses": C, "samples_per_cycle": N, "single_samples_per_s": rs,
            "mappo_samples_per_s": rm, "single_median": ms, "mappo_median": mm,
            "single_spread": (max(rs) - min(rs)) / ms, "mappo_spread": (max(rm) - min(rm)) / mm,
            "time_per_sample_ratio": mm / ms, "graph_rows_single": rows_single, "graph_rows_mappo": rows_mappo,
            "predicted_ratio": rows_single / rows_mappo, "micro_single": single.micro, "micro_mappo": mappo.micro,
            "chunk_single": single.chunk, "chunk_mappo": mappo.chunk}
        del single, mappo, snet, mnet, pool
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
