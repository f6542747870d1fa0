"""A trained policy applied to a directory of CNF files -- the policy's side of ``utils.sat_solver``.

    python -m marlsat.utils.policy_solver --config configs/MAPPO_CONFIG.yaml [section.KEY=VALUE ...] \\
        --checkpoint experiments/mappo_runs/<run> --cnf-dir data/uf50-218 --sol-dir out/uf50-218 \\
        [--tries 8 --rounds 2 --max-steps 512 --temperature 1.0 --no-greedy-round --finish walksat|none
         --finish-tries 8 --finish-flips 100000 --noise 0.5 --seed 0 --report report.json --baseline-walksat
         --actor-only]

The network is the config's (``environment`` / ``network`` sections) with the parameters of ``--checkpoint``: a
run directory (``<dir>/checkpoints/latest_model_0``, ``load_train_state``) or a behavioural-cloning directory
(``<dir>/bc_model_<N>``, ``inject_bc``).  The files are grouped by (num_vars, num_clauses); the parameter layout
depends on the agent partition and the heads on how num_vars splits, so a group is solved when its num_vars is
the config's NUM_VARS (any num_clauses) and listed as skipped otherwise.  Each solved group is one device
problem pool searched by ``solvers.policy.solve_pool_with_policy``: an optional greedy round, rounds of sampled
tries, and WalkSAT from the best assignment the policy reached for what is left.

Every reported solution, the policy's or WalkSAT's, is verified with ``SATEnv._calculate_satisfaction_explicit``
before anything is written: ``<stem>.sol`` in the reference's format (``sat_solver.write_sol``, read by
``runners.behavioral_cloning.load_expert_data``) and ``policy_solutions.txt`` in the runner's
``test_solutions.txt`` format (``verify_solutions_file`` reads it).  ``--report`` writes the JSON report: per
instance who solved it, in which round and try, with how many policy steps and flips and how many WalkSAT flips;
per group the solve rates of the policy alone and with the finish and the medians of the policy solves; with
``--baseline-walksat`` the solve rate and median flips of ``solve_pool`` on the same instances beside them.
The exit status is 1 if a non-skipped instance stayed unsolved, like ``sat_solver``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, List, Optional

import numpy as np

from .data_parser import group_problems, load_cnf_problems
from .sat_solver import sol_path, write_sol

SOLUTIONS_FILE = "policy_solutions.txt"
BY_NAMES = ("none", "policy", "walksat")
INSTANCE_FIELDS = ("name", "solved", "by", "round", "try", "steps", "flips", "finish_flips", "best_unsat")


def _median(values) -> Optional[float]:
    v = np.asarray(values)
    return float(np.median(v)) if v.size else None


def instance_report(name: str, res: Dict[str, np.ndarray], i: int) -> Dict:
    """One instance's report entry (``INSTANCE_FIELDS``) from ``solve_pool_with_policy``'s arrays."""
    return {"name": name, "solved": bool(res["solved"][i]), "by": BY_NAMES[int(res["by"][i])],
            "round": int(res["round"][i]), "try": int(res["try"][i]), "steps": int(res["steps"][i]),
            "flips": int(res["flips"][i]), "finish_flips": int(res["finish_flips"][i]),
            "best_unsat": int(res["best_unsat"][i])}


def group_report(V: int, C: int, names: List[str], res: Dict[str, np.ndarray], baseline=None) -> Dict:
    """A group's report: counts, the solve rate of the policy alone and with the finish, the median steps and
    flips of the policy's solves (None when it solved nothing), and the WalkSAT baseline when one was run."""
    n = len(names)
    by = np.asarray(res["by"])
    pol = by == 1
    g = {"num_vars": int(V), "num_clauses": int(C), "instances": n,
         "solved_by_policy": int(pol.sum()), "solved_by_walksat": int((by == 2).sum()),
         "unsolved": int((~np.asarray(res["solved"])).sum()),
         "solve_rate_policy": float(pol.sum()) / n if n else 0.0,
         "solve_rate_with_finish": float(np.asarray(res["solved"]).sum()) / n if n else 0.0,
         "median_policy_steps": _median(res["steps"][pol]), "median_policy_flips": _median(res["flips"][pol]),
         "median_finish_flips": _median(res["finish_flips"][by == 2]),
         "results": [instance_report(nm, res, i) for i, nm in enumerate(names)]}
    if baseline is not None:
        ok = np.asarray(baseline["solved"])
        g["baseline_walksat"] = {"solve_rate": float(ok.sum()) / n if n else 0.0,
                                 "median_flips": _median(np.asarray(baseline["flips"])[ok])}
    return g


def find_checkpoint(path: str):
    """``("rl", state)`` for a run directory, ``("bc", state)`` for a BC directory; an error when neither holds
    a checkpoint (never a silently random network)."""
    from . import checkpoints as ck

    st = ck.restore_checkpoint(os.path.join(path, "checkpoints"), "latest_model_", 0)
    if st is not None:
        return "rl", st
    st = ck.restore_checkpoint(path, "latest_model_", 0)
    if st is not None:
        return "rl", st
    st = ck.restore_checkpoint(path, "bc_model_", None)
    if st is not None:
        return "bc", st
    raise FileNotFoundError(f"no checkpoint in {path!r}: expected <dir>/checkpoints/latest_model_0 (a run directory) "
                            f"or <dir>/bc_model_<N> (behavioural cloning)")


def solve_directory_with_policy(config: Dict, checkpoint: str, cnf_dir: str, sol_dir: str, *, baseline: bool = False,
                                log=None, key=None, **solve_kwargs) -> Dict:
    """The CLI's work; returns the report (``groups``, ``skipped``, ``unsolved`` names)."""
    from ..envs.multi_agent_sat_env import SATEnv
    from ..learners.gnn import GNNActorCritic
    from ..learners.mappo_gnn_sat_learner import MAPPOLearner
    from ..runners.mappo_runner import flat_config, solution_line
    from ..solvers.policy import solve_pool_with_policy
    from ..solvers.walksat import solve_pool
    from . import checkpoints as ck

    kind, state = find_checkpoint(checkpoint)
    fc = flat_config(config)
    V0 = int(fc["NUM_VARS"])
    max_steps = int(solve_kwargs.pop("max_steps", None) or fc["MAX_STEPS"])
    max_batch = int(solve_kwargs.get("max_batch", 4096))
    problems = load_cnf_problems(cnf_dir)
    os.makedirs(sol_dir, exist_ok=True)
    report = {"checkpoint": os.path.abspath(checkpoint), "checkpoint_kind": kind, "cnf_dir": os.path.abspath(cnf_dir),
              "groups": [], "skipped": [], "unsolved": []}
    lines = {}
    net = None
    for (V, C), g in group_problems(problems).items():
        if V != V0:
            report["skipped"].append({"num_vars": V, "num_clauses": C, "names": list(g["names"]),
                                      "reason": f"num_vars {V} is not the config's NUM_VARS {V0}: the network's "
                                                f"parameter layout and heads are built for that partition"})
            continue
        env = SATEnv(V, C, max(max_steps, int(fc["MAX_STEPS"])), vars_per_agent=fc.get("VARS_PER_AGENT"),
                     action_mode=fc.get("action_mode", 0))
        if net is None:  # one network for every group: its layout depends on (A, M, V), not on C
            net = GNNActorCritic(fc["GNN_HIDDEN_DIM"], fc["GNN_NUM_MESSAGE_PASSING_STEPS"], env.num_agents,
                                 env.max_vars_per_agent, env.action_mode, env.num_vars,
                                 seed=int(config.get("SEED", 42)))
            if kind == "rl":
                ck.load_train_state(net, state, reset_optimizer=True)
            else:
                ck.inject_bc(net, state)
        pool = env.make_pool(g["clauses"])
        learner = MAPPOLearner(dict(fc, NUM_ENVS=max_batch, NUM_STEPS=1, MINIBATCH_SIZE=max_batch), env, net, pool)
        res = solve_pool_with_policy(learner, pool, max_steps=max_steps, key=key, **solve_kwargs)
        _, nun = env._calculate_satisfaction_explicit(res["solution"], g["clauses"])
        valid = res["solved"] & (nun.cpu().numpy() == 0)
        if (res["solved"] & ~valid).any():
            bad = [n for n, s, v in zip(g["names"], res["solved"], valid) if s and not v]
            raise RuntimeError(f"the solver reported solutions that do not satisfy their formulas: {bad}")
        base = solve_pool(pool, key=key) if baseline else None
        for i, name in enumerate(g["names"]):
            if valid[i]:
                write_sol(sol_path(sol_dir, name), res["solution"][i])
            else:
                report["unsolved"].append(name)
            steps = res["steps"][i] if res["by"][i] == 1 else max_steps  # the runner's Steps: policy steps taken
            lines[name] = solution_line(name, bool(valid[i]), int(steps), res["solution"][i])
        gr = group_report(V, C, list(g["names"]), res, base)
        report["groups"].append(gr)
        if log is not None:
            log(f"V={V} C={C}: policy {gr['solved_by_policy']}, walksat finish {gr['solved_by_walksat']}, unsolved "
                f"{gr['unsolved']} of {gr['instances']}")
    with open(os.path.join(sol_dir, SOLUTIONS_FILE), "w", encoding="utf-8") as f:
        for p in problems:
            if p["name"] in lines:
                f.write(lines[p["name"]])
    return report


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="A trained policy with sampled restarts and a WalkSAT finish: one .sol "
                                             "per .cnf of a directory")
    ap.add_argument("--config", default="configs/MAPPO_CONFIG.yaml")
    ap.add_argument("overrides", nargs="*", help="section.KEY=VALUE (hydra-style)")
    ap.add_argument("--checkpoint", required=True, help="run directory or behavioural-cloning directory")
    ap.add_argument("--cnf-dir", required=True)
    ap.add_argument("--sol-dir", required=True)
    ap.add_argument("--tries", type=int, default=8, help="sampled tries per unsolved instance and round")
    ap.add_argument("--rounds", type=int, default=2, help="rounds, the greedy one included")
    ap.add_argument("--max-steps", type=int, default=None, help="env steps per try (default: the config's MAX_STEPS)")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--no-greedy-round", action="store_true", help="round 0 samples too")
    ap.add_argument("--finish", choices=("walksat", "none"), default="walksat")
    ap.add_argument("--finish-tries", type=int, default=8)
    ap.add_argument("--finish-flips", type=int, default=100_000)
    ap.add_argument("--noise", type=float, default=0.5, help="WalkSAT's random-walk probability")
    ap.add_argument("--max-batch", type=int, default=4096, help="env rows per device batch")
    ap.add_argument("--actor-only", action="store_true",
                    help="encode the agents' graphs alone in every search step (no critic graph; same results)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--report", default=None, help="write the JSON report here")
    ap.add_argument("--baseline-walksat", action="store_true", help="also run solve_pool on the same instances")
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    from ..random import PRNGKey
    from ..runners.mappo_runner import load_config

    a = build_parser().parse_args(argv)
    try:
        report = solve_directory_with_policy(
            load_config(a.config, a.overrides), a.checkpoint, a.cnf_dir, a.sol_dir, baseline=a.baseline_walksat,
            log=print, key=PRNGKey(a.seed), tries=a.tries, rounds=a.rounds, max_steps=a.max_steps,
            temperature=a.temperature, greedy_round=not a.no_greedy_round, finish=a.finish,
            finish_tries=a.finish_tries, finish_flips=a.finish_flips, noise=a.noise, max_batch=a.max_batch,
            actor_only=a.actor_only)
    except FileNotFoundError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    if a.report:
        with open(a.report, "w", encoding="utf-8") as f:
            json.dump(report, f, indent=1)
    n = sum(g["instances"] for g in report["groups"])
    print(f"solved {n - len(report['unsolved'])}, unsolved {len(report['unsolved'])} of {n} files in {a.cnf_dir}; "
          f"{sum(len(s['names']) for s in report['skipped'])} skipped; solutions in {a.sol_dir}")
    for s in report["skipped"]:
        print(f"skipped V={s['num_vars']} C={s['num_clauses']} ({len(s['names'])} files): {s['reason']}")
    for nm in report["unsolved"]:
        print(f"unsolved: {nm}")
    return 1 if report["unsolved"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
