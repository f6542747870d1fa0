"""DPLL on the device: verdicts, launch time and nodes/s on unplanted random 3-SAT at the threshold (run on the GPU
from the repo root):

    python profiles/dpll_throughput.py [--reps 3] [--pools uf50-218,uf100-430] [--out FILE]

It writes profiles/dpll_throughput.json (--out: elsewhere).

Pools: uf50-218 x 256, uf100-430 x 256 and uf200-860 x 32 instances, drawn by the seeded host generator below (three
distinct variables per clause, random signs, nothing planted: about half of each pool is unsatisfiable).  Per pool:
  - one launch, one sample per instance, under the pool's node budget (POOLS): the SAT / UNSAT / UNKNOWN counts, the launch
    time (device events over --reps launches after one warm-up launch; one timed launch where the warm-up took more
    than 10 s) and nodes/s = nodes made / time;
  - on the UNSAT subset: the launch time with cube_bits 0 against cube_bits 4 (16 cubes per instance), alternated
    inside each repetition, and the nodes each makes;
  - on the same subset: the wall time of WalkSAT's default budget (solve_pool: 8 tries x 100000 flips x 4 rounds,
    which solves none of them) beside the wall time of the decide_pool call that decides it;
  - decide_pool with its defaults on the whole pool: verdict counts and wall time.
Every SAT model is checked with the env's clause check.  No number here has a threshold.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-sat_amd")]

POOLS = (("uf50-218", 50, 218, 256, 4096), ("uf100-430", 100, 430, 256, 65536), ("uf200-860", 200, 860, 32, 1 << 20))


def random_pool(np, V, C, N, seed):
    """(N, C, 3) int32: unplanted random 3-SAT, three distinct variables per clause, random signs."""
    rng = np.random.default_rng(seed)
    vs = np.argsort(rng.random((N, C, V)), axis=2)[:, :, :3] + 1
    return (vs * rng.choice([-1, 1], size=vs.shape)).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20240)
    ap.add_argument("--pools", default=",".join(p[0] for p in POOLS), help="comma-separated subset of the pools")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpll_throughput.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from marlsat import SATEnv
    from marlsat.random import PRNGKey
    from marlsat.solvers.dpll import SAT, UNKNOWN, UNSAT, decide_pool, dpll
    from marlsat.solvers.walksat import solve_pool

    if not torch.cuda.is_available():
        raise SystemExit("dpll_throughput: no GPU; nothing is measured on the CPU")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def counts(st):
        st = np.asarray(st)
        return {"SAT": int((st == SAT).sum()), "UNSAT": int((st == UNSAT).sum()), "UNKNOWN": int((st == UNKNOWN).sum())}

    result = {"reps": args.reps, "seed": args.seed, "device": torch.cuda.get_device_name(0), "pools": {}}
    for i, (name, V, C, N, budget) in enumerate(POOLS):
        if name not in args.pools.split(","):
            continue
        pool_np = random_pool(np, V, C, N, args.seed + i)
        env = SATEnv(V, C, max_steps=1, vars_per_agent=V)
        pool = env.make_pool(pool_np)
        idx = torch.arange(N, dtype=torch.int32, device="cuda")
        entry = {"V": V, "C": C, "instances": N, "max_nodes": budget}

        # ---- one launch, one sample per instance
        (out, warm_ms) = timed(lambda: dpll(pool, idx, max_nodes=budget))
        reps = args.reps if warm_ms < 10e3 else 1
        print(f"{name}: warm-up launch {warm_ms:.1f} ms, {reps} timed launches", file=sys.stderr, flush=True)
        ms = [timed(lambda: dpll(pool, idx, max_nodes=budget))[1] for _ in range(reps)]
        st, x, nd = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.int64)
        _, nun = env._calculate_satisfaction_explicit(x, pool_np)
        assert (nun.cpu().numpy()[st == SAT] == 0).all(), "a model the env does not confirm"
        entry["single"] = {"status": counts(st), "ms_per_launch": [round(m, 3) for m in ms],
                           "warmup_ms": round(warm_ms, 3), "nodes": int(nd.sum()), "max_nodes_of_a_sample": int(nd.max()),
                           "nodes_per_s": float(nd.sum()) / (min(ms) / 1e3),
                           "us_per_node_of_longest_sample": 1e3 * min(ms) / max(int(nd.max()), 1),
                           "mean_nodes": {"SAT": float(nd[st == SAT].mean()) if (st == SAT).any() else None,
                                          "UNSAT": float(nd[st == UNSAT].mean()) if (st == UNSAT).any() else None}}

        # ---- the UNSAT subset: cube_bits 0 against 4, alternated
        un = np.flatnonzero(st == UNSAT)
        if un.size:
            sub = env.make_pool(pool_np[un])
            forms = {}
            for bits in (0, 4):
                K = 1 << bits
                forms[bits] = (torch.arange(un.size, dtype=torch.int32, device="cuda").repeat_interleave(K),
                               torch.arange(K, dtype=torch.int32, device="cuda").repeat(un.size))
            ab = {bits: [] for bits in forms}
            nodes_ab = {}
            for rep in range(-1, reps):  # rep -1: warm-up, not timed
                for bits, (pi, cu) in forms.items():
                    o, m = timed(lambda: dpll(sub, pi, cubes=cu, cube_bits=bits, max_nodes=budget))
                    if rep >= 0:
                        ab[bits].append(m)
                    s2 = o[0].reshape(un.size, -1)
                    assert bool((s2 == UNSAT).all()), "a cube of an UNSAT instance that is not UNSAT"
                    nodes_ab[bits] = (int(o[2].sum().item()), int(o[2].max().item()))
            entry["unsat_subset"] = {"instances": int(un.size), "cube_bits": {
                str(b): {"samples": int(un.size) << b, "ms_per_launch": [round(m, 3) for m in ab[b]],
                         "nodes": nodes_ab[b][0], "max_nodes_of_a_sample": nodes_ab[b][1]} for b in ab}}
            # ---- WalkSAT's default budget on it, beside the decide_pool call that decides it
            decide_pool(sub, max_nodes=1, max_rounds=2)  # warm-up of both calls' host paths, not timed
            solve_pool(sub, key=PRNGKey(1), max_flips=1, max_rounds=1)
            ws, ws_ms = wall(lambda: solve_pool(sub, key=PRNGKey(1)))
            dec, dec_ms = wall(lambda: decide_pool(sub))
            entry["unsat_subset"]["walksat_default_budget"] = {"wall_ms": round(ws_ms, 1), "solved": int(ws["solved"].sum())}
            entry["unsat_subset"]["decide_pool_defaults"] = {"wall_ms": round(dec_ms, 1), "status": counts(dec["status"])}
            print(f"{name}: UNSAT subset {un.size}: walksat {ws_ms:.0f} ms, decide_pool {dec_ms:.0f} ms", file=sys.stderr,
                  flush=True)

        # ---- decide_pool with its defaults on the whole pool
        dec, dec_ms = wall(lambda: decide_pool(pool))
        _, nun = env._calculate_satisfaction_explicit(dec["solution"], pool_np)
        assert (nun.cpu().numpy()[dec["status"] == SAT] == 0).all(), "a model the env does not confirm"
        entry["decide_pool_defaults"] = {"wall_ms": round(dec_ms, 1), "status": counts(dec["status"]),
                                         "nodes": int(dec["nodes"].sum())}
        result["pools"][name] = entry
        print(f"{name}: {json.dumps(entry)}", file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
