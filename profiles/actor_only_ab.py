"""Actor-only graph batches against the full (critic + agents) batches, in the two paths that never read the value
(run on the GPU from the repo root):

    python profiles/actor_only_ab.py [--steps 32] [--rows 1024] [--pool 256] [--alternations 3] [--out FILE]

Solver leg.  Shapes uf50-218 and uf200-860 on the bench's pools (bench.WORKLOADS, seeds 1000 * size_id + i), row b
on instance b % pool, --rows rows, H = 128, L = 16, a randomly initialised network (the time of a step does not
depend on the parameters), greedy, --steps steps, early exit off.  policy_search(actor_only=False), the parent's
path untouched, and policy_search(actor_only=True) are alternated --alternations times after one untimed pass of
each; each timing is wall clock around the call with a device synchronisation before and after, reset and final
device -> host reads included, divided by the steps.  Both must return the same record.

BC leg.  BCLearner.train_epoch samples/s at uf50-218 with the committed config's network and training section
(configs/MAPPO_CONFIG.yaml: H, L, MINIBATCH_SIZE, LEARNING_RATE), 4 random assignments per pool instance with their
greedy labels, one learner per path on its own copy of the same network, alternated the same way (an epoch each);
the peak device memory of an epoch beside it.

The rule (set before measuring): at each shape the actor-only median must lie below the full path's fastest run
(for samples/s: above its best).  ``predicted_ratio`` is the row share left when graph 0 goes (1 - graph 0's share
of a sample's rows, from the templates); it is recorded beside the measured ratio of medians, and is no pass bar.
One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-sat_amd")]

SHAPES = ("uf50-218", "uf200-860")
BC_SHAPE = "uf50-218"
RECORD = ("prev_x", "best_x", "best_unsat", "best_step", "first_solve", "flips", "unsolved")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "MAPPO_CONFIG.yaml"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from marlsat import SATEnv
    from marlsat.learners.bc_learner import BCLearner
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.random import Key
    from marlsat.runners.behavioral_cloning import compute_joint_labels
    from marlsat.runners.mappo_runner import flat_config, load_config
    from marlsat.solvers.policy import policy_search
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    if not torch.cuda.is_available():
        raise SystemExit("actor_only_ab: no GPU; nothing is measured on the CPU")
    T, B = args.steps, args.rows
    result = {"steps": T, "rows": B, "pool": args.pool, "hidden": args.hidden, "layers": args.layers,
              "alternations": args.alternations, "device": torch.cuda.get_device_name(0), "shapes": {}}

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def shares(tpl):
        """graph 0's share of a sample's rows and incidences over the pool's instances."""
        rows_full = (tpl.full_v + tpl.full_c).double().sum().item()
        rows_crit = (tpl.crit_v + tpl.crit_c).double().sum().item()
        return rows_crit / rows_full, tpl.crit_e.double().sum().item() / tpl.full_e.double().sum().item()

    for name in SHAPES:
        V, C, vpa, _, size_id = bench.WORKLOADS[name]
        env = SATEnv(V, C, max_steps=T, vars_per_agent=vpa)
        pool = env.make_pool(generate_problem_pool(V, C, args.pool, size_id=size_id, skip_isolated=True))
        net = GNNActorCritic(args.hidden, args.layers, env.num_agents, env.max_vars_per_agent, 0, V, device="cuda",
                             seed=1)
        lr = MAPPOLearner(dict(NUM_ENVS=B, NUM_STEPS=1, MINIBATCH_SIZE=B), env, net, pool)
        pidx = np.arange(B) % args.pool
        key = Key(0x5EED, 7)
        run = lambda ao: policy_search(lr, pool, pidx, T, key, greedy=True, early_exit=False, actor_only=ao)
        _, want = timed(lambda: run(False))  # untimed pass of each
        _, got = timed(lambda: run(True))
        same = all(torch.equal(getattr(got, f), getattr(want, f)) for f in RECORD)
        full, act = [], []
        for _ in range(args.alternations):
            full.append(timed(lambda: run(False))[0] / T * 1e3)
            act.append(timed(lambda: run(True))[0] / T * 1e3)
            print(f"{name}: full {full[-1]:.3f} ms/step, actor-only {act[-1]:.3f} ms/step", file=sys.stderr, flush=True)
        row_share, inc_share = shares(lr.tpl)
        result["shapes"][name] = {
            "num_vars": V, "num_clauses": C, "agents": env.num_agents, "chunk": lr.chunk,
            "actor_chunk": lr.actor_chunk, "mean_full_rows": lr.tpl.mean_full_rows,
            "mean_actor_rows": lr.tpl.mean_actor_rows, "graph0_row_share": row_share,
            "graph0_incidence_share": inc_share, "full_ms_per_step": full, "actor_only_ms_per_step": act,
            "actor_only_median": statistics.median(act), "full_fastest": min(full),
            "meets_rule": statistics.median(act) < min(full),
            "measured_ratio": statistics.median(act) / statistics.median(full), "predicted_ratio": 1.0 - row_share,
            "records_equal": bool(same)}
        del lr, net, pool
        torch.cuda.empty_cache()

    # ---- behavioural cloning
    fc = flat_config(load_config(args.config, []))
    V, C, vpa, _, size_id = bench.WORKLOADS[BC_SHAPE]
    env = SATEnv(V, C, max_steps=4, vars_per_agent=vpa)
    clauses = generate_problem_pool(V, C, args.pool, size_id=size_id, skip_isolated=True)
    pool = env.make_pool(clauses)
    per = 4
    pidx = np.repeat(np.arange(args.pool, dtype=np.int32), per)
    x = np.random.default_rng(0).integers(0, 2, (pidx.size, V)).astype(np.uint8)
    labels = compute_joint_labels(env, pool, pidx, x, 0.0)
    H, L = int(fc["GNN_HIDDEN_DIM"]), int(fc["GNN_NUM_MESSAGE_PASSING_STEPS"])
    learners = {}
    for ao in (False, True):
        net = GNNActorCritic(H, L, env.num_agents, env.max_vars_per_agent, 0, V, device="cuda", seed=1)
        learners[ao] = BCLearner(fc, env, net, pool, actor_only=ao)
        learners[ao].set_data(pidx, x, labels)
    gens = {ao: torch.Generator().manual_seed(3) for ao in learners}

    def epoch(ao):
        torch.cuda.reset_peak_memory_stats()
        dt, out = timed(lambda: learners[ao].train_epoch(gens[ao]))
        return pidx.size / dt, out["loss"], torch.cuda.max_memory_allocated()

    first = {ao: epoch(ao) for ao in (False, True)}  # untimed pass of each
    rate = {False: [], True: []}
    peak, loss = {}, {False: [first[False][1]], True: [first[True][1]]}
    for _ in range(args.alternations):
        for ao in (False, True):
            r, l, m = epoch(ao)
            rate[ao].append(r)
            loss[ao].append(l)
            peak[ao] = m
        print(f"BC {BC_SHAPE}: full {rate[False][-1]:.1f} samples/s, actor-only {rate[True][-1]:.1f} samples/s",
              file=sys.stderr, flush=True)
    row_share, inc_share = shares(learners[True].tpl)
    result["bc"] = {
        "shape": BC_SHAPE, "hidden": H, "layers": L, "samples": int(pidx.size), "minibatch": learners[True].MB,
        "micro_full": learners[False].micro, "micro_actor_only": learners[True].micro,
        "graph0_row_share": row_share, "graph0_incidence_share": inc_share,
        "full_samples_per_s": rate[False], "actor_only_samples_per_s": rate[True],
        "actor_only_median": statistics.median(rate[True]), "full_fastest": max(rate[False]),
        "meets_rule": statistics.median(rate[True]) > max(rate[False]),
        "measured_ratio": statistics.median(rate[False]) / statistics.median(rate[True]),  # time per sample, as above
        "predicted_ratio": 1.0 - row_share,
        "peak_bytes_full": int(peak[False]), "peak_bytes_actor_only": int(peak[True]),
        "epoch_losses_full": loss[False], "epoch_losses_actor_only": loss[True]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
