"""Planted random k-SAT files from the device generator.

    python -m marlsat.utils.device_generator --num N --vars V --clauses C [--k 3 --seed S] --cnf-dir D --sol-dir S

Writes ``uf{V}-{i:03d}.cnf`` (i = 1..N, DIMACS, what utils/data_parser.parse_cnf reads) and the planted assignment of
each as ``uf{V}-{i:03d}.sol`` (one line, a signed DIMACS model, what runners/behavioral_cloning.load_expert_data
reads), so behavioural cloning and every other directory-based tool run on device-generated data unchanged.  The
instances are ``ProblemPool.generate``'s (msat_pool_generate): the family of utils/generate_cnf_dataset.py, drawn
from Philox words on the device, not the same bytes.  Instances that leave a variable in no clause are redrawn
(``--allow-isolated`` keeps them).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

from ..envs.multi_agent_sat_env import ProblemPool
from .data_parser import write_cnf
from .generation import instance_name


def write_pool(pool: ProblemPool, cnf_dir: str, sol_dir: Optional[str] = None) -> List[str]:
    """The pool's instances as uf{V}-{i:03d}.cnf under cnf_dir and, with sol_dir and a planted pool, their planted
    assignments as uf{V}-{i:03d}.sol; returns the .cnf names."""
    os.makedirs(cnf_dir, exist_ok=True)
    clauses = pool.clauses.cpu().numpy()
    planted = None
    if sol_dir is not None:
        if pool.planted is None:
            raise ValueError("write_pool: sol_dir given, but the pool carries no planted assignments")
        os.makedirs(sol_dir, exist_ok=True)
        planted = pool.planted.cpu().numpy()
    names = []
    for i, cl in enumerate(clauses):
        name = instance_name(pool.num_vars, i)
        write_cnf(os.path.join(cnf_dir, name), pool.num_vars, cl)
        if planted is not None:
            with open(os.path.join(sol_dir, name[: -len(".cnf")] + ".sol"), "w") as f:
                f.write(" ".join(str(v + 1 if b else -(v + 1)) for v, b in enumerate(planted[i])) + "\n")
        names.append(name)
    return names


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num", type=int, required=True, help="number of instances")
    ap.add_argument("--vars", type=int, required=True, help="variables per instance")
    ap.add_argument("--clauses", type=int, required=True, help="clauses per instance")
    ap.add_argument("--k", type=int, default=3, help="literals per clause (1..3)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cnf-dir", required=True)
    ap.add_argument("--sol-dir", default=None, help="also write the planted assignments there")
    ap.add_argument("--max-attempts", type=int, default=64)
    ap.add_argument("--allow-isolated", action="store_true", help="keep instances with a variable in no clause")
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    a = parser().parse_args(argv)
    if a.num < 1 or a.num > 999:
        raise SystemExit(f"--num {a.num} must be in [1, 999] (three-digit file names)")
    pool = ProblemPool.generate((a.vars, a.clauses, a.k), a.num, a.seed, reject_isolated=not a.allow_isolated,
                                max_attempts=a.max_attempts)
    names = write_pool(pool, a.cnf_dir, a.sol_dir)
    redrawn = int((pool.attempts > 0).sum().item())
    print(f"wrote {len(names)} instances (V={a.vars}, C={a.clauses}, K={a.k}; {redrawn} redrawn) to {a.cnf_dir}"
          f"{f' and their planted assignments to {a.sol_dir}' if a.sol_dir else ''}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
