"""WalkSAT on the device: flips/s and instances solved/s per kernel form (run on the GPU from the repo root):

    python profiles/walksat_throughput.py [--max-flips 20000] [--reps 5] [--pool 256] [--out FILE]

Shapes: uf50-218 x 1024 samples and uf200-860 x 4096 samples on the bench's pools (bench.WORKLOADS, seeds
1000 * size_id + i), noise 0.5, RNG starts, sample s on instance s % pool; uf100-430 x 4096 (between the two, for
the choice of form 0); and the two at 32768 samples, where every
CU holds as many waves as it can (the two smaller launches last about as long as their one longest run).  Every form that accepts the shape
(0 = the automatic choice) is timed with device events over --reps launches with different counters after one
warm-up launch; the forms are alternated inside each repetition.  flips/s = flips actually made (sum of the
flips output) / time; solved/s = samples solved / time.  All forms must agree bitwise on every output.  Beside it,
the NumPy replay of tests/walksat_replay.py on a few of the same samples, timed on the host: a restatement for
checking, "replay, not a solver".  One JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-sat_amd"), os.path.join(ROOT, "tests")]

SHAPES = (("uf50-218", 1024), ("uf200-860", 4096), ("uf100-430", 4096), ("uf50-218", 32768), ("uf200-860", 32768))
REG_CAPS = (128, 256, 512, 1023)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-flips", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--replay-samples", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from marlsat import SATEnv
    from marlsat.random import Key
    from marlsat.solvers.walksat import noise_p32, walksat, walksat_forms
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool
    from walksat_replay import replay

    if not torch.cuda.is_available():
        raise SystemExit("walksat_throughput: no GPU; nothing is measured on the CPU")
    seed = 0x5EED0000
    result = {"max_flips": args.max_flips, "noise": args.noise, "reps": args.reps, "pool": args.pool,
              "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, S in SHAPES:
        V, C, vpa, _, size_id = bench.WORKLOADS[name]
        pool_np = generate_problem_pool(V, C, args.pool, size_id=size_id)
        env = SATEnv(V, C, max_steps=1, vars_per_agent=vpa)
        pool = env.make_pool(pool_np)
        pidx_np = np.arange(S) % args.pool
        pidx = torch.from_numpy(pidx_np.astype(np.int32)).cuda()
        forms = [0] + [f for f in range(1, walksat_forms() + 1) if f > len(REG_CAPS) or C <= REG_CAPS[f - 1]]
        ms = {f: [] for f in forms}
        flips = {f: 0 for f in forms}
        solved = {f: 0 for f in forms}
        longest = []  # the longest run of each timed launch: the launch lasts as long as its slowest sample
        for rep in range(-1, args.reps):  # rep -1: warm-up, not timed
            key = Key(seed, 100 + rep)
            outs = {}
            for f in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[f] = walksat(pool, pidx, key=key, max_flips=args.max_flips, noise=args.noise, form=f)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 0:
                    ms[f].append(e0.elapsed_time(e1))
                    flips[f] += int(outs[f][2].sum().item())
                    solved[f] += int(outs[f][1].sum().item())
            if rep >= 0:
                longest.append(int(outs[0][2].max().item()))
            for f in forms[1:]:
                assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[f])), (name, f, "forms disagree")
            if rep == -1:
                _, nun = env._calculate_satisfaction_explicit(outs[0][0][:256], pool_np[pidx_np[:256]])
                assert torch.equal(nun == 0, outs[0][1][:256] != 0), "a solved flag the env does not confirm"
        shape = {"V": V, "C": C, "samples": S, "longest_run_flips": longest, "forms": {}}
        for f in forms:
            t = sum(ms[f]) / 1e3
            shape["forms"][str(f)] = {"ms_per_launch": [round(m, 3) for m in ms[f]],
                                      "flips_per_s": flips[f] / t, "solved_per_s": solved[f] / t,
                                      "us_per_flip_of_longest_run": 1e3 * sum(ms[f]) / max(sum(longest), 1),
                                      "mean_flips": flips[f] / (S * args.reps),
                                      "solved_fraction": solved[f] / (S * args.reps)}
        n = args.replay_samples
        t0 = time.perf_counter()
        r = replay(pool_np, V, pidx_np[:n], min(args.max_flips, 2000), noise_p32(args.noise), seed, 100)
        dt = time.perf_counter() - t0
        shape["replay, not a solver"] = {"samples": n, "flips_per_s": float(r[2].sum()) / dt,
                                         "solved_per_s": float(r[1].sum()) / dt, "host": "NumPy, one process"}
        result["shapes"][f"{name} x {S}"] = shape
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
