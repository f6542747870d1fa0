"""Behavioural-cloning pre-training -- drop-in for src/runners/behavioral_cloning.py.

    python -m marlsat.runners.behavioral_cloning --config configs/MAPPO_CONFIG.yaml [section.KEY=VALUE ...]

Data side:
* ``load_expert_data(cnf_dir, sol_dir)`` (behavioral_cloning.py:29-50): ``<name>.sol`` files
  (first line: signed DIMACS model or 0/1 values; a positive entry is 1, anything else 0) paired with
  ``<name>.cnf`` (``utils.generate_cnf_dataset.generate_cnf_dataset_sat(sol_dir=...)`` writes the planted
  solutions in that format);
* ``compute_joint_labels_parallel_greedy(env, clauses, assignments, tau)`` (:54-100): the
  reference signature for one env, and ``compute_joint_labels`` for a whole batch -- both run
  ``msat_bc_greedy_labels`` (one workgroup per env evaluates every single-variable flip in one
  clause pass; the reference re-evaluates the formula once per candidate flip);
* ``preprocess(...)`` (:103-151): NUM_SAMPLES_PER_EXPERT corrupted copies of every expert
  solution (CORRUPTION_LEVEL distinct variables flipped; ``corrupt`` with numpy's generator on the host, or
  ``corrupt_device`` = ``msat_bc_corrupt`` with ``device_corrupt=True``), labelled with TAU_IMPROVE; the
  result is saved as ``.npz`` (instance ids, assignments, labels) -- the global GNN input is
  re-derived on the device from (instance, assignment), as in the MAPPO learner.
Training side, ``run(config)`` (:194-349): NUM_UPDATES epochs of joint cross-entropy on the actor
(learners/bc_learner.BCLearner), ``bc_training_log.txt``, the ``bc_model_<NUM_UPDATES>`` checkpoint that
``mappo_runner``'s ``loading.inject_bc_model_path`` consumes, then the greedy evaluation of the trained actor
as a solver on every loaded problem -> ``solver_solutions_log.txt``.  Single process.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import SATEnv, _lib
from ..envs.multi_agent_sat_env import ProblemPool
from ..random import PRNGKey, as_key, split
from ..utils.data_parser import clauses_array, load_cnf_problems

SOLVER_LOG_HEADER = "# Format: CNF_File, Solved_Status, Steps_To_Solve, Is_Solution_Valid, Predicted_Solution\n"


def load_expert_data(cnf_dir: str, sol_dir: str) -> List[Dict[str, np.ndarray]]:
    problems = {p["name"]: p for p in load_cnf_problems(cnf_dir)}
    out = []
    for sol in sorted(f for f in os.listdir(sol_dir) if f.endswith(".sol")):
        name = sol[: -len(".sol")] + ".cnf"
        if name not in problems:
            continue
        with open(os.path.join(sol_dir, sol)) as f:
            vals = [int(v) for v in f.readline().split()]
        out.append({"name": name, "problem_clauses": clauses_array(problems[name]),
                    "expert_solution": np.array([int(v > 0) for v in vals], dtype=np.int32)})
    return out


def compute_joint_labels(env: SATEnv, pool: ProblemPool, problem_idx, assignments, tau: float = 0.0,
                         return_deltas: bool = False):
    """Batched labels (B, A) int32 (device): per agent the best single flip among its variables
    (local index) if it lowers the unsatisfied count by more than -tau, else the no-op index M."""
    dev = env.device
    pidx = torch.as_tensor(problem_idx, device=dev).to(torch.int32).contiguous()
    x = torch.as_tensor(assignments, device=dev).to(torch.uint8).contiguous()
    B = pidx.numel()
    if x.shape != (B, env.num_vars):
        raise ValueError(f"assignments must be (B, V) = ({B}, {env.num_vars})")
    labels = torch.empty((B, env.num_agents), dtype=torch.int32, device=dev)
    deltas = torch.empty((B, env.num_vars), dtype=torch.int32, device=dev) if return_deltas else None
    _lib.check(_lib.lib.msat_bc_greedy_labels(env._desc(B, pool), pool.packed.data_ptr(), pidx.data_ptr(),
                                              x.data_ptr(), float(tau), labels.data_ptr(), _lib.ptr(deltas),
                                              _lib.stream_ptr(dev)), "msat_bc_greedy_labels")
    return (labels, deltas) if return_deltas else labels


def compute_joint_labels_parallel_greedy(env: SATEnv, clauses: np.ndarray, assignments: np.ndarray,
                                         tau: float) -> np.ndarray:
    """behavioral_cloning.py:54-100 signature: one env's (C, K) clauses and (V,) assignment -> (A,) labels."""
    pool = env.make_pool(np.asarray(clauses, dtype=np.int32)[None])
    lab = compute_joint_labels(env, pool, [0], np.asarray(assignments)[None], tau)
    return lab[0].cpu().numpy()


def corrupt(solutions: np.ndarray, num_samples: int, level: int, seed: int = 0) -> np.ndarray:
    """(N, V) expert solutions -> (N * num_samples, V): `level` distinct variables flipped per copy
    (behavioral_cloning.py:121-124; numpy RNG instead of jax.random.choice)."""
    rng = np.random.default_rng(seed)
    N, V = solutions.shape
    out = np.repeat(solutions.astype(np.uint8), num_samples, axis=0)
    for r in range(out.shape[0]):
        out[r, rng.choice(V, size=min(level, V), replace=False)] ^= 1
    return out


def corrupt_device(solutions, num_samples: int, level: int, key=None, device=None) -> torch.Tensor:
    """``corrupt`` on the device (msat_bc_corrupt): (N, V) -> (N * num_samples, V) uint8 device tensor, row
    e * num_samples + k a copy of expert e with min(level, V) distinct variables flipped.  The variables are
    Floyd's sample drawn from the Philox stream of ``key`` (include/marlsat.h), so a host can replay them; the
    stream differs from ``corrupt``'s numpy generator."""
    k = as_key(key)
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    src = torch.as_tensor(np.asarray(solutions) if not torch.is_tensor(solutions) else solutions,
                          device=dev).to(torch.uint8).contiguous()
    if src.dim() != 2:
        raise ValueError(f"solutions must be (N, V), got {tuple(src.shape)}")
    N, V = src.shape
    if N < 1 or num_samples < 0:
        raise ValueError(f"corrupt_device: N={N} experts, num_samples={num_samples}")
    rows = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(int(num_samples)).contiguous()
    out = torch.empty((rows.numel(), V), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.msat_bc_corrupt(src.data_ptr(), N, rows.data_ptr(), rows.numel(), V, int(level), k.seed,
                                        k.counter, out.data_ptr(), _lib.stream_ptr(dev)), "msat_bc_corrupt")
    return out


def bc_settings(config: Optional[dict]) -> Dict:
    """The ``bc_training`` section with the reference's defaults (behavioral_cloning.py:107-110, :202, :229).
    The reference's train_step has one mode and reads neither coefficient; a request for anything else is
    refused instead of being silently ignored."""
    bc = dict((config or {}).get("bc_training") or {})
    mode = bc.get("MODE", "parallel_joint")
    if mode != "parallel_joint":
        raise ValueError(f"bc_training.MODE={mode!r}: only 'parallel_joint' (joint cross-entropy over every agent's "
                         f"greedy label) exists, in the reference's train_step as here")
    for coef in ("CONSISTENCY_COEF", "NOOP_SUPERVISION_COEF"):
        if float(bc.get(coef, 0.0) or 0.0) != 0.0:
            raise ValueError(f"bc_training.{coef}={bc[coef]}: the reference's train_step has no such term (its loss is "
                             f"the joint cross-entropy alone); set it to 0.0")
    return {"NUM_SAMPLES_PER_EXPERT": int(bc.get("NUM_SAMPLES_PER_EXPERT", 5)),
            "CORRUPTION_LEVEL": int(bc.get("CORRUPTION_LEVEL", 3)),
            "TAU_IMPROVE": float(bc.get("TAU_IMPROVE", 0.0)),
            "SOL_DATA_DIR": bc.get("SOL_DATA_DIR", "data/uf20-91-answer"),
            "SOLVE_MISSING_EXPERTS": bool(bc.get("SOLVE_MISSING_EXPERTS", False)),
            # ours: with SOLVE_MISSING_EXPERTS, DPLL decides what WalkSAT leaves unsolved (solve_directory(complete=True))
            "SOLVE_MISSING_COMPLETE": bool(bc.get("SOLVE_MISSING_COMPLETE", False)),
            # ours (no reference key): micro-batches without the critic's graph (BCLearner(actor_only=True))
            "ACTOR_ONLY_GRAPHS": bool(bc.get("ACTOR_ONLY_GRAPHS", False)),
            "SAVE_PATH": bc.get("SAVE_PATH", "models/bc_pretrained")}


def solve_missing_experts(cnf_dir: str, sol_dir: str, seed: int = 0, log=print,
                          complete: bool = False) -> Dict[str, List[str]]:
    """bc_training.SOLVE_MISSING_EXPERTS: WalkSAT on the device (utils.sat_solver.solve_directory) for the
    ``.cnf`` files of cnf_dir that have no ``.sol`` in sol_dir; the files that have one are left alone.
    ``complete`` (bc_training.SOLVE_MISSING_COMPLETE): DPLL then decides what WalkSAT left unsolved, and the files
    it proves unsatisfiable are logged as dropped from the BC set (no policy can ever finish them)."""
    from ..utils.sat_solver import sol_path, solve_directory

    names = sorted(f for f in os.listdir(cnf_dir) if f.endswith(".cnf"))
    missing = [n for n in names if not os.path.exists(sol_path(sol_dir, n))]
    if not complete:
        res = {"solved": [], "unsolved": []}
        if missing:
            res = solve_directory(cnf_dir, sol_dir, names=missing, key=PRNGKey(seed))
        log(f"[*] experts: {len(names) - len(missing)} .sol files found, {len(res['solved'])} solved by WalkSAT, "
            f"{len(res['unsolved'])} skipped (unsolved)")
        return res
    res = {"solved": [], "unsolved": [], "unsat": []}
    if missing:
        res = solve_directory(cnf_dir, sol_dir, names=missing, key=PRNGKey(seed), complete=True)
    log(f"[*] experts: {len(names) - len(missing)} .sol files found, {len(res['solved'])} solved by WalkSAT or DPLL, "
        f"{len(res['unsat'])} proven unsatisfiable, {len(res['unsolved'])} skipped (undecided)")
    for n in res["unsat"]:
        log(f"[*] experts: {n} is unsatisfiable: dropped from the BC set")
    return res


def preprocess(expert_data: List[Dict[str, np.ndarray]], env: SATEnv, config: Optional[dict] = None,
               save_path: Optional[str] = None, seed: int = 0, device_corrupt: bool = False) -> Dict[str, np.ndarray]:
    bc = (config or {}).get("bc_training", {}) or {}
    S = int(bc.get("NUM_SAMPLES_PER_EXPERT", 5))
    level = int(bc.get("CORRUPTION_LEVEL", 3))
    tau = float(bc.get("TAU_IMPROVE", 0.0))
    clauses = np.stack([e["problem_clauses"] for e in expert_data])
    sols = np.stack([e["expert_solution"][: env.num_vars] for e in expert_data])
    pool = env.make_pool(clauses)
    pidx = np.repeat(np.arange(len(expert_data), dtype=np.int32), S)
    if device_corrupt:
        xd = corrupt_device(sols, S, level, PRNGKey(seed), env.device)
        labels = compute_joint_labels(env, pool, pidx, xd, tau).cpu().numpy()
        x = xd.cpu().numpy()
    else:
        x = corrupt(sols, S, level, seed)
        labels = compute_joint_labels(env, pool, pidx, x, tau).cpu().numpy()
    data = {"problem_idx": pidx, "assignments": x, "labels": labels, "clauses": clauses}
    if save_path:
        np.savez_compressed(save_path, **data)
    return data


def solver_log_line(name: str, solved: bool, steps: int, valid: bool, solution: np.ndarray) -> str:
    """behavioral_cloning.py:336-337."""
    s = "".join(str(int(v)) for v in solution) if solved else "N/A"
    return f"{name}, {bool(solved)}, {int(steps)}, {bool(valid)}, {s}\n"


# ------------------------------------------------------------------ main ----
def run(config: Dict, log=print) -> Dict:
    from ..learners.bc_learner import BCLearner
    from ..learners.gnn import GNNActorCritic
    from ..learners.mappo_gnn_sat_learner import MAPPOLearner
    from ..utils import checkpoints as ck
    from .mappo_runner import evaluate_policy, flat_config

    bc = bc_settings(config)
    fc = flat_config(config)
    seed = int(config.get("SEED", 42))
    np.random.seed(seed)
    key = PRNGKey(seed)
    save_path = os.path.abspath(bc["SAVE_PATH"])
    os.makedirs(save_path, exist_ok=True)
    rewards = fc.get("rewards") or {}
    env = SATEnv(fc["NUM_VARS"], fc["NUM_CLAUSES"], fc["MAX_STEPS"], vars_per_agent=fc.get("VARS_PER_AGENT"),
                 action_mode=fc.get("action_mode", 0), r_clause=rewards.get("R_CLAUSE", 0.02),
                 r_sat=rewards.get("R_SAT", 1.0), gamma=fc.get("GAMMA", 0.99))
    cnf_dir = config.get("CNF_DATA_DIR", "data")
    if bc["SOLVE_MISSING_EXPERTS"]:
        if bc["SOLVE_MISSING_COMPLETE"]:
            solve_missing_experts(cnf_dir, bc["SOL_DATA_DIR"], seed, log, complete=True)
        else:
            solve_missing_experts(cnf_dir, bc["SOL_DATA_DIR"], seed, log)
    experts = load_expert_data(cnf_dir, bc["SOL_DATA_DIR"])
    if not experts:
        log(f"no expert (.cnf, .sol) pairs found in {cnf_dir} / {bc['SOL_DATA_DIR']}")
        return {}
    for e in experts:
        if e["problem_clauses"].shape[0] != env.num_clauses or e["expert_solution"].shape[0] < env.num_vars:
            raise ValueError(f"{e['name']}: {e['problem_clauses'].shape[0]} clauses, a model of "
                             f"{e['expert_solution'].shape[0]} values; the config is V={env.num_vars}, "
                             f"C={env.num_clauses} (one size per run, as the reference)")
    log(f"[*] {len(experts)} expert problem-solution pairs")
    net = GNNActorCritic(fc["GNN_HIDDEN_DIM"], fc["GNN_NUM_MESSAGE_PASSING_STEPS"], env.num_agents,
                         env.max_vars_per_agent, env.action_mode, env.num_vars, seed=seed)
    key, k_data = split(key, 2)
    data = preprocess(experts, env, config, seed=k_data.seed, device_corrupt=True)
    train_pool = env.make_pool(data["clauses"])
    learner = BCLearner(fc, env, net, train_pool, actor_only=bc["ACTOR_ONLY_GRAPHS"])
    learner.set_data(data["problem_idx"], data["assignments"], data["labels"])
    n_upd = int(fc["NUM_UPDATES"])
    gen = torch.Generator().manual_seed(seed)
    log(f"[*] BC pre-training (parallel_joint): {learner.N} samples, {n_upd} epochs of "
        f"{-(-learner.N // learner.MB)} minibatches")
    last = {}
    t0 = time.time()
    with open(os.path.join(save_path, "bc_training_log.txt"), "w", encoding="utf-8") as logf:
        logf.write("epoch,loss\n")
        for epoch in range(n_upd):
            last = learner.train_epoch(gen)
            logf.write(f"{epoch + 1},{last['loss']:.6f}\n")
            logf.flush()
    torch.cuda.synchronize()
    train_seconds = time.time() - t0
    rate = learner.N * n_upd / max(train_seconds, 1e-9)
    if last:
        log(f"epoch {n_upd}: loss {last['loss']:.6f}, label accuracy {last['accuracy']:.2%}; "
            f"{rate:.1f} training samples/s")
    ck.save_checkpoint(save_path, {"params": ck.train_state_dict(net)["params"]}, step=n_upd, prefix="bc_model_",
                       overwrite=True)
    log(f"[+] model saved to {save_path} (bc_model_{n_upd})")
    # the trained actor as a solver (:297-349): greedy joint actions on every problem of CNF_DATA_DIR
    problems = load_cnf_problems(cnf_dir)
    for p in problems:
        if (p["num_vars"], p["num_clauses"]) != (env.num_vars, env.num_clauses):
            raise ValueError(f"{p['name']} is V={p['num_vars']}, C={p['num_clauses']}; the config is "
                             f"V={env.num_vars}, C={env.num_clauses}")
    all_clauses = np.stack([clauses_array(p) for p in problems])
    eval_pool = env.make_pool(all_clauses)
    n = len(problems)
    eval_learner = MAPPOLearner(dict(fc, NUM_ENVS=n, NUM_STEPS=1, MINIBATCH_SIZE=n), env, net, eval_pool)
    key, k_ev = split(key, 2)
    solved, steps, sols = evaluate_policy(k_ev, eval_learner, eval_pool, range(n), int(fc["MAX_STEPS"]))
    _, nun = env._calculate_satisfaction_explicit(sols, all_clauses)
    valid = solved & (nun.cpu().numpy() == 0)
    with open(os.path.join(save_path, "solver_solutions_log.txt"), "w", encoding="utf-8") as f:
        f.write(SOLVER_LOG_HEADER)
        for p, s, k, v, x in zip(problems, solved, steps, valid, sols):
            f.write(solver_log_line(p["name"], bool(s), int(k), bool(v), x))
    solve_rate = float(solved.mean()) if n else 0.0
    avg_steps = float(steps[solved].mean()) if solved.any() else 0.0
    log(f"BC model as a solver: {int(solved.sum())} / {n} problems solved ({solve_rate:.2%}); average steps to "
        f"solve {avg_steps:.2f} (solved problems)")
    return {"save_path": save_path, "train_seconds": train_seconds, "samples_per_second": rate, "last_epoch": last,
            "solve_rate": solve_rate, "avg_steps": avg_steps, "num_samples": learner.N, "network": net}


def main(argv: Optional[List[str]] = None):
    from .mappo_runner import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="configs/MAPPO_CONFIG.yaml")
    ap.add_argument("overrides", nargs="*", help="section.KEY=VALUE (hydra-style)")
    a = ap.parse_args(argv)
    run(load_config(a.config, a.overrides))


if __name__ == "__main__":
    main(sys.argv[1:])
