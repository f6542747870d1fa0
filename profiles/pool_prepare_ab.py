"""Preparing a problem pool: the host path against the device path, at the same commit on the same machine (run on
the GPU from the repo root):

    python profiles/pool_prepare_ab.py [--instances 1024] [--alternations 3] [--device-reps 50]
                                       [--out profiles/pool_prepare_ab.json]

Shapes uf50-218 at A = 10 and uf200-860 at A = 25, --instances instances each.  Two legs per shape:

  templates   host: build_templates(pool.clauses.cpu().numpy(), V, A) + DeviceTemplates(...) (the upload), what the
              learners' constructors run;  device: build_templates_device(pool, V, A) (count kernel, scan, one read
              of the totals, fill kernel).  Both over the same generated pool; the twelve arrays must be equal.
  generation  host: generate_problem_pool(V, C, N, skip_isolated=True) + ProblemPool(...) (Mersenne-Twister loop,
              upload, pack);  device: ProblemPool.generate((V, C, 3), N, key) (Philox kernel with the retry rule,
              pack, the read of `attempts`).  The two make different instances of the same family.

Each timing is wall clock around the work with a device synchronisation before and after.  A device call is about a
millisecond, too short a window on its own, so a device timing is --device-reps calls back to back (each with its
own read of the totals or of `attempts`, as a user's call has) divided by their number; a host timing is one call.
One untimed pass of each path first (code objects load, allocator warms), then the two paths alternated
--alternations times; the record keeps every run, the median and the min-max spread, and ratio = host median /
device median.  Nothing is gated.
One JSON line, also written to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-sat_amd")]

SHAPES = (("uf50-218", 50, 218, 10), ("uf200-860", 200, 860, 25))  # name, V, C, A
ARRAYS = ("vgid", "cgid", "slots", "ptr", "inc", "voff", "coff", "eoff", "poff", "gv", "gc", "ge")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--device-reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_prepare_ab.json"))
    args = ap.parse_args()

    import torch

    from marlsat import ProblemPool
    from marlsat.learners.graphs import DeviceTemplates, build_templates, build_templates_device
    from marlsat.random import Key
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    if not torch.cuda.is_available():
        raise SystemExit("pool_prepare_ab: no GPU; nothing is measured on the CPU")
    N = args.instances

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def ab(host, device):
        """One untimed pass of each, then alternated; (summary dict, last host output, last device output)."""
        host(), device()
        runs = {"host": [], "device": []}
        last = {}
        for _ in range(args.alternations):
            t, last["host"] = timed(host)
            runs["host"].append(t)
            t, last["device"] = timed(lambda: [device() for _ in range(args.device_reps)][-1])
            runs["device"].append(t / args.device_reps)
        summ = {k: {"seconds": [round(t, 6) for t in v], "median": round(statistics.median(v), 6),
                    "min": round(min(v), 6), "max": round(max(v), 6)} for k, v in runs.items()}
        summ["ratio_host_over_device"] = round(summ["host"]["median"] / summ["device"]["median"], 2)
        # the device path is faster only if its slowest run beats the host path's fastest
        summ["device_faster_beyond_spread"] = summ["device"]["max"] < summ["host"]["min"]
        return summ, last["host"], last["device"]

    result = {"instances": N, "alternations": args.alternations, "device_reps": args.device_reps,
              "device": torch.cuda.get_device_name(0), "cpus": len(os.sched_getaffinity(0)), "shapes": {}}
    for name, V, C, A in SHAPES:
        pool = ProblemPool.generate((V, C, 3), N, Key(1234, 0))
        tpl, h, d = ab(lambda: DeviceTemplates(build_templates(pool.clauses.cpu().numpy(), V, A), A, pool.device),
                       lambda: build_templates_device(pool, V, A))
        tpl["equal"] = all(torch.equal(getattr(h, f), getattr(d, f)) for f in ARRAYS)
        tpl["var_rows"], tpl["clause_rows"], tpl["incidences"] = (int(h.vgid.numel()), int(h.cgid.numel()),
                                                                  int(h.inc.numel()))
        size_id = {50: 1, 200: 3}[V]
        gen, hp, dp = ab(lambda: ProblemPool(generate_problem_pool(V, C, N, size_id=size_id, skip_isolated=True), V,
                                             pool.device),
                         lambda: ProblemPool.generate((V, C, 3), N, Key(99, 7)))
        gen["device_instances_redrawn"] = int((dp.attempts > 0).sum().item())
        gen["shapes_equal"] = tuple(hp.clauses.shape) == tuple(dp.clauses.shape)
        result["shapes"][name] = {"V": V, "C": C, "A": A, "templates": tpl, "generation": gen}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(s["templates"]["equal"] for s in result["shapes"].values()):
        raise SystemExit("pool_prepare_ab: the device templates differ from the host builder's")


if __name__ == "__main__":
    main()
