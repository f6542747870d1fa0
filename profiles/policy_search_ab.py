"""policy_search against evaluate_policy, per step, and the policy solver's throughput (run on the GPU from the repo
root):

    python profiles/policy_search_ab.py [--steps 32] [--rows 1024] [--pool 256] [--alternations 3] [--out FILE]

Shapes: uf50-218 x 1024 rows and uf200-860 x 1024 rows on the bench's pools (bench.WORKLOADS, seeds
1000 * size_id + i), row b on instance b % pool, H = 128, L = 16, a randomly initialised network (the time of a step
does not depend on the parameters), greedy, 32 steps, early exit off.  evaluate_policy (runners/mappo_runner.py,
unchanged by the policy solver: the runner's loop, which writes the observation block every step and tracks the
first solve with four torch ops) and policy_search (solvers/policy.py: no observation, the record kept by
msat_solve_track) are alternated --alternations times after one untimed pass of each; each timing is wall clock
around the call with a device synchronisation before and after, reset and final device -> host reads included, divided
by the steps.  Both must report the same (solved, steps, solution).

Then solve_pool_with_policy's throughput at tries = 8: --rows / 8 instances x 8 sampled tries = --rows rows in
one slab, one round, no greedy round, no finish, --steps steps: instance-tries x steps per second, three timed
calls after a warm-up; then the same at twice the rows (--pool caps the instances), whose rate against the first
says whether the smaller batch already fills the device.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from marlsat import SATEnv
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
    from marlsat.random import Key, split
    from marlsat.runners.mappo_runner import evaluate_policy
    from marlsat.solvers.policy import policy_search, solve_pool_with_policy
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    if not torch.cuda.is_available():
        raise SystemExit("policy_search_ab: no GPU; nothing is measured on the CPU")
    T, B = args.steps, args.rows
    result = {"steps": T, "rows": B, "pool": args.pool, "hidden": args.hidden, "layers": args.layers,
              "alternations": args.alternations, "device": torch.cuda.get_device_name(0), "shapes": {}}

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    for name in SHAPES:
        V, C, vpa, _, size_id = bench.WORKLOADS[name]
        env = SATEnv(V, C, max_steps=T, vars_per_agent=vpa)
        pool = env.make_pool(generate_problem_pool(V, C, args.pool, size_id=size_id, skip_isolated=True))
        net = GNNActorCritic(args.hidden, args.layers, env.num_agents, env.max_vars_per_agent, 0, V, device="cuda",
                             seed=1)
        lr = MAPPOLearner(dict(NUM_ENVS=B, NUM_STEPS=1, MINIBATCH_SIZE=B), env, net, pool)
        pidx = np.arange(B) % args.pool
        key = Key(0x5EED, 7)
        run_eval = lambda: evaluate_policy(key, lr, pool, pidx, T, early_exit=False)
        run_search = lambda: policy_search(lr, pool, pidx, T, key, greedy=True, early_exit=False).as_evaluation(T)
        _, want = timed(run_eval)  # untimed pass of each
        _, got = timed(run_search)
        _, nun0 = env._calculate_satisfaction_explicit(
            env.reset_from_pool(pool, B, split(key, 2)[0], problem_idx=pidx,
                                with_obs=False)[1].variable_assignments.cpu().numpy(),
            pool.clauses.cpu().numpy()[pidx])
        start_sat = (nun0.cpu().numpy() == 0)
        same = all(np.array_equal(g[~start_sat], w[~start_sat]) for g, w in zip(got, want))
        ev, ps = [], []
        for _ in range(args.alternations):
            ev.append(timed(run_eval)[0] / T * 1e3)
            ps.append(timed(run_search)[0] / T * 1e3)
            print(f"{name}: evaluate_policy {ev[-1]:.3f} ms/step, policy_search {ps[-1]:.3f} ms/step", file=sys.stderr,
                  flush=True)
        shape = {"num_vars": V, "num_clauses": C, "agents": env.num_agents, "chunk": lr.chunk,
                 "evaluate_policy_ms_per_step": ev, "policy_search_ms_per_step": ps,
                 "policy_search_median": statistics.median(ps), "evaluate_policy_slowest": max(ev),
                 "not_slower": statistics.median(ps) <= max(ev), "outputs_equal": bool(same),
                 "rows_satisfied_at_reset": int(start_sat.sum()), "solved_rows": int(want[0].sum())}
        # solver throughput at tries = 8: one slab of B rows, then of 2 B rows (does the rate still grow?)
        shape["solver"] = []
        for rows in (B, 2 * B):
            n_inst = min(rows // 8, args.pool)
            sub = env.make_pool(pool.clauses.cpu().numpy()[:n_inst])
            lr8 = MAPPOLearner(dict(NUM_ENVS=rows, NUM_STEPS=1, MINIBATCH_SIZE=rows), env, net, sub)
            solve = lambda c: solve_pool_with_policy(lr8, sub, tries=8, rounds=1, max_steps=T, greedy_round=False,
                                                     finish="none", max_batch=rows, key=Key(0x5EED, c))
            timed(lambda: solve(0))
            rates, solved = [], []
            for c in range(1, 4):
                dt, res = timed(lambda: solve(c))
                rates.append(n_inst * 8 * T / dt)
                solved.append(int(res["solved"].sum()))
            shape["solver"].append({"instances": n_inst, "tries": 8, "rows": n_inst * 8, "steps": T,
                                    "instance_tries_x_steps_per_s": rates, "solved_of_instances": solved})
            print(f"{name}: solver {n_inst * 8} rows {statistics.median(rates):.0f} instance-tries x steps/s",
                  file=sys.stderr, flush=True)
        r1, r2 = (statistics.median(x["instance_tries_x_steps_per_s"]) for x in shape["solver"])
        shape["rate_gain_at_twice_the_rows"] = r2 / r1  # ~1: the smaller batch already fills the device
        result["shapes"][name] = shape
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
