"""Delta observation write vs the full write, alternated in one process (run on the GPU from the repo root):

    python profiles/obs_delta_sweep.py [--workload uf200-860] [--envs 4096] [--rounds 5] [--steps 200] [--out FILE]

For every round, in turn: the full write (obs_delta=False) and the delta write at G = 16, 64, 128 aligned bytes per
stored group (MARLSAT_OBS_DELTA_GROUP is read once at import, so the steppers are built with the module value
patched).  Every leg steps its own state + obs (same seeds, same actions), so all legs compute the same rollout; the
mean launch time of K back-to-back launches is taken with device events, as bench.py does.  One JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-sat_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uf200-860")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--preroll-s", type=float, default=3.0)
    ap.add_argument("--obs-dtype", default="int32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import time

    import torch

    import bench
    from marlsat import SATEnv
    from marlsat.envs import multi_agent_sat_env as mod
    from marlsat.random import Key
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    V, C, vpa, _, size_id = bench.WORKLOADS[args.workload]
    B = args.envs
    dt = torch.int32 if args.obs_dtype == "int32" else torch.int8
    env = SATEnv(V, C, max_steps=512, vars_per_agent=vpa, obs_dtype=dt)
    pool = env.make_pool(generate_problem_pool(V, C, 1024, size_id=size_id))
    gen = torch.Generator(device="cuda").manual_seed(1234)
    ring = 64
    acts = torch.randint(0, env.max_vars_per_agent + 1, (ring, B, env.num_agents), generator=gen, device="cuda",
                         dtype=torch.int32)
    stagger = torch.randint(0, 512, (B,), generator=gen, device="cuda", dtype=torch.int32)
    legs = {}
    for name, g in (("full", 0), ("g16", 16), ("g64", 64), ("g128", 128)):
        o, st = env.reset_from_pool(pool, B, Key(0x5EED0000, 0))
        st.step.copy_(stagger)
        st.invalidate_reset_queue()
        mod.OBS_DELTA_GROUP = g or 16
        legs[name] = {"step": env.stepper(st, o, env._step_out(B), autoreset=True, seed=0x5EED0000, obs_delta=g != 0),
                      "obs": o, "st": st, "ms": [], "counter": 1}

    def run(leg, n):
        for i in range(n):
            leg["step"](acts[leg["counter"] % ring], leg["counter"])
            leg["counter"] += 1

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.preroll_s:  # clocks settle under load (bench.py's pre-roll)
        for leg in legs.values():
            run(leg, 32)
        torch.cuda.synchronize()
    for r in range(args.rounds):
        for leg in legs.values():
            run(leg, 20)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            run(leg, args.steps)
            b.record()
            torch.cuda.synchronize()
            leg["ms"].append(a.elapsed_time(b) / args.steps)
    ref = legs["full"]
    same = {n: bool(torch.equal(l["obs"], ref["obs"]) and torch.equal(l["st"].variable_assignments,
                                                                      ref["st"].variable_assignments))
            for n, l in legs.items()}
    rec = {"workload": f"{args.workload}/B{B}/{args.obs_dtype}", "steps": args.steps,
           "launch_us": {n: [round(1e3 * v, 3) for v in l["ms"]] for n, l in legs.items()},
           "min_us": {n: round(1e3 * min(l["ms"]), 3) for n, l in legs.items()},
           "obs_and_state_equal_to_full": same}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    assert all(same.values()), same


if __name__ == "__main__":
    main()
