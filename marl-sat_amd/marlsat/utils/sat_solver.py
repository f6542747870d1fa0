"""Expert solutions for a directory of CNF files -- stands in for src/utils/sat_solver.py.

    python -m marlsat.utils.sat_solver --cnf-dir data/uf50-218 --sol-dir data/uf50-218-answer

The reference runs pysat's Glucose3 over every ``.cnf`` and writes ``<stem>.sol`` as ``' '.join(map(str, assign))``
(one line of 0/1 values, ``sat_solver.py:5-29``).  Here the files are grouped by (num_vars, num_clauses), each
group becomes one device problem pool, and ``solvers.walksat.solve_pool`` (batched WalkSAT/SKC with random
restarts, ``msat_walksat``) searches all of its instances at once.  Every solution is verified with
``SATEnv._calculate_satisfaction_explicit`` before its file is written, in the reference's format, which
``runners.behavioral_cloning.load_expert_data`` reads as is.  Local search is incomplete: an instance it does not
solve (an unsatisfiable one never is) gets no file and is reported as unsolved.

``--complete`` (``solve_directory(complete=True)``) closes that gap: the instances WalkSAT leaves unsolved go to
``solvers.dpll.decide_pool`` (batched DPLL, ``msat_dpll``), which returns a model or the verdict
that none exists.  Its models are verified and written like WalkSAT's; the proven-unsatisfiable names are listed
in ``<sol_dir>/unsat.txt``; only what the node budgets (``--max-nodes``, ``--cube-bits``) leave undecided is still
reported as unsolved, and only that makes the exit status 1.

``--init-model <run_dir>`` (``solve_directory(init_model=...)``) starts round 0 from an assignment predictor's output
(runners/bc_runner.py) instead of random draws: one checkpoint serves every size of the directory,
because no parameter of that network depends on V or C.  An instance the prediction already satisfies is solved with
0 flips; verification, the file format and the exit status are the same.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

from .data_parser import group_problems, load_cnf_problems


def sol_path(sol_dir: str, cnf_name: str) -> str:
    stem = cnf_name[: -len(".cnf")] if cnf_name.endswith(".cnf") else cnf_name
    return os.path.join(sol_dir, stem + ".sol")


def write_sol(path: str, assignment) -> None:
    """One line of space-separated 0/1 values (the reference's ``' '.join(map(str, assign))``)."""
    with open(path, "w") as f:
        f.write(" ".join(str(int(v)) for v in np.asarray(assignment).reshape(-1)) + "\n")


def predicted_starts(net, desc: Dict, pool, key=None):
    """The predictor's assignment for every instance of ``pool``: (pred (N, V) u8, num_unsat (N,), solved (N,)) on
    the device.  Its input is x = 0, or, for a model trained with INPUT: corrupted, the assignment ``env.reset``
    draws for env n under ``key`` (what msat_walksat starts from without an initial assignment)."""
    import torch

    from ..learners.assign_learner import AssignLearner
    from ..solvers.walksat import walksat

    N, V = int(pool.num_problems), int(pool.num_vars)
    idx = torch.arange(N, dtype=torch.int32, device=pool.device)
    if desc.get("INPUT", "zeros") == "zeros":
        x = torch.zeros((N, V), dtype=torch.uint8, device=pool.device)
    else:
        x = walksat(pool, idx, key=key, max_flips=0)[0]
    return AssignLearner({}, net, pool).predict(idx, x)


def solve_directory(cnf_dir: str, sol_dir: str, *, names: Optional[Sequence[str]] = None, log=None,
                    init_model: Optional[str] = None, complete: bool = False, dpll_kwargs: Optional[Dict] = None,
                    **solve_kwargs) -> Dict[str, List[str]]:
    """Solve the ``.cnf`` files of ``cnf_dir`` (all of them, or only ``names``) and write ``<stem>.sol`` into
    ``sol_dir`` for each one solved.  ``solve_kwargs`` go to ``solve_pool`` (tries, max_flips, max_rounds, noise,
    key).  ``init_model``: a bc_runner run directory; its predictor, loaded once, gives round 0's starts for every
    (V, C) group.  Returns ``{"solved": [names], "unsolved": [names]}`` in directory order (with ``init_model`` also
    ``"starts": {name: (V,) uint8}``, the predicted assignments).

    ``complete``: ``solvers.dpll.decide_pool(**dpll_kwargs)`` (max_nodes, cube_bits, max_rounds) then searches the
    instances WalkSAT left unsolved.  Its models are verified and written like WalkSAT's (their names are among
    ``"solved"``), the proven-unsatisfiable names are returned under the new key ``"unsat"`` and written to
    ``<sol_dir>/unsat.txt``, one per line in directory order, and ``"unsolved"`` holds only the undecided ones."""
    from ..envs.multi_agent_sat_env import SATEnv
    from ..solvers.walksat import solve_pool

    model = None
    if init_model is not None:
        from ..runners.bc_runner import load_predictor

        model = load_predictor(init_model)
    starts = {}
    unsat = set()

    problems = load_cnf_problems(cnf_dir)
    if names is not None:
        keep = set(names)
        problems = [p for p in problems if p["name"] in keep]
    os.makedirs(sol_dir, exist_ok=True)
    done = {}
    for (V, C), g in group_problems(problems).items():
        env = SATEnv(V, C, max_steps=1, vars_per_agent=V)  # one agent: only the clause check is used
        pool = env.make_pool(g["clauses"])
        note = ""
        if model is not None:
            pred, _, pre = predicted_starts(model[0], model[1], pool, solve_kwargs.get("key"))
            res = solve_pool(pool, init_assignments=pred, **solve_kwargs)
            starts.update(zip(g["names"], pred.cpu().numpy()))
            note = (f"; the prediction alone solved {int((pre != 0).sum())}, round 0 "
                    f"{int((res['round'] == 0).sum())}")
        else:
            res = solve_pool(pool, **solve_kwargs)
        _, nun = env._calculate_satisfaction_explicit(res["solution"], g["clauses"])
        valid = res["solved"] & (nun.cpu().numpy() == 0)
        if (res["solved"] & ~valid).any():
            bad = [n for n, s, v in zip(g["names"], res["solved"], valid) if s and not v]
            raise RuntimeError(f"walksat reported solutions that do not satisfy their formulas: {bad}")
        for name, ok, x in zip(g["names"], valid, res["solution"]):
            done[name] = bool(ok)
            if ok:
                write_sol(sol_path(sol_dir, name), x)
        left = np.flatnonzero(~valid)
        if complete and left.size:
            from ..solvers.dpll import SAT, UNSAT, decide_pool

            sub = g["clauses"][left]
            dec = decide_pool(env.make_pool(sub), **(dpll_kwargs or {}))
            _, dnun = env._calculate_satisfaction_explicit(dec["solution"], sub)
            dnun = dnun.cpu().numpy()
            bad = [g["names"][i] for k, i in enumerate(left) if dec["status"][k] == SAT and dnun[k] != 0]
            if bad:
                raise RuntimeError(f"dpll reported models that do not satisfy their formulas: {bad}")
            for k, i in enumerate(left):
                name = g["names"][i]
                if dec["status"][k] == SAT:
                    done[name] = True
                    write_sol(sol_path(sol_dir, name), dec["solution"][k])
                elif dec["status"][k] == UNSAT:
                    unsat.add(name)
            note += (f"; dpll on {left.size}: {int((dec['status'] == SAT).sum())} SAT, "
                     f"{int((dec['status'] == UNSAT).sum())} UNSAT, {int((dec['status'] == 0).sum())} undecided")
        elif complete:
            note += "; dpll on 0: 0 SAT, 0 UNSAT, 0 undecided"
        if log is not None:
            log(f"V={V} C={C}: {int(valid.sum())} / {len(valid)} solved{note}")
    order = [p["name"] for p in problems]
    out = {"solved": [n for n in order if done[n]],
           "unsolved": [n for n in order if not done[n] and n not in unsat]}
    if complete:
        out["unsat"] = [n for n in order if n in unsat]
        with open(os.path.join(sol_dir, "unsat.txt"), "w") as f:
            f.write("".join(n + "\n" for n in out["unsat"]))
    if model is not None:
        out["starts"] = starts
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="WalkSAT on the device: one .sol per .cnf of a directory")
    ap.add_argument("--cnf-dir", required=True)
    ap.add_argument("--sol-dir", required=True)
    ap.add_argument("--tries", type=int, default=8, help="samples per unsolved instance and round")
    ap.add_argument("--max-flips", type=int, default=100_000, help="flips per sample and launch")
    ap.add_argument("--max-rounds", type=int, default=4, help="restart rounds")
    ap.add_argument("--noise", type=float, default=0.5, help="random-walk probability")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--init-model", default=None, help="a bc_runner run directory: its assignment predictor gives "
                                                       "round 0's starting assignments")
    ap.add_argument("--complete", action="store_true", help="DPLL on what WalkSAT leaves unsolved: a model or the "
                                                            "verdict UNSAT (listed in <sol-dir>/unsat.txt)")
    ap.add_argument("--max-nodes", type=int, default=None, help="--complete: branch nodes of the first DPLL round")
    ap.add_argument("--cube-bits", type=int, default=None, help="--complete: later rounds run 2^bits cubes per "
                                                                "instance")
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    from ..random import PRNGKey

    a = build_parser().parse_args(argv)
    if not a.complete:
        res = solve_directory(a.cnf_dir, a.sol_dir, tries=a.tries, max_flips=a.max_flips, max_rounds=a.max_rounds,
                              noise=a.noise, key=PRNGKey(a.seed), log=print, init_model=a.init_model)
        print(f"solved {len(res['solved'])}, unsolved {len(res['unsolved'])} of "
              f"{len(res['solved']) + len(res['unsolved'])} files in {a.cnf_dir}; solutions in {a.sol_dir}")
    else:
        dk = {k: v for k, v in (("max_nodes", a.max_nodes), ("cube_bits", a.cube_bits)) if v is not None}
        res = solve_directory(a.cnf_dir, a.sol_dir, tries=a.tries, max_flips=a.max_flips, max_rounds=a.max_rounds,
                              noise=a.noise, key=PRNGKey(a.seed), log=print, init_model=a.init_model, complete=True,
                              dpll_kwargs=dk)
        total = len(res["solved"]) + len(res["unsat"]) + len(res["unsolved"])
        print(f"solved {len(res['solved'])}, unsatisfiable {len(res['unsat'])}, undecided {len(res['unsolved'])} of "
              f"{total} files in {a.cnf_dir}; solutions and unsat.txt in {a.sol_dir}")
        for n in res["unsat"]:
            print(f"unsat: {n}")
    for n in res["unsolved"]:
        print(f"unsolved: {n}")
    return 1 if res["unsolved"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
