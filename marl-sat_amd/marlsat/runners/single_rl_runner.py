"""Single-agent PPO baseline: training / evaluation driver -- drop-in for src/runners/single_rl_runner.py.

    python -m marlsat.runners.single_rl_runner --config configs/SINGLE_RL_PPO_CONFIG.yaml [section.KEY=VALUE ...]

One agent flips one of all V variables per step; the question it answers is whether MAPPO's decomposition over a
variable partition buys anything.  The cycle loop is the reference's (runner:372-516):
  1. rollout (every env onto a freshly drawn instance, NUM_STEPS steps with auto-reset) -> PPO update -> train
     statistics (learners/single_ppo_learner.py);
  2. greedy evaluation on EVAL_EPISODES instances drawn from the pool, only when the cycle's train solve rate reaches
     EVAL_MIN_TRAIN_SOLVE_RATE; a better (solve rate, then shorter length) result is saved as ``best_eval_<cycle>``;
  3. ``cycle_<n>`` checkpoints, the last 3 kept; ``final_model_<NUM_CYCLES>`` at the end;
  4. ``train_eval_log.txt``: the reference's header and one line per cycle in its field order (train_avg_len and
     train_avg_return are written as 0, as the reference writes them; a skipped evaluation as 0 inf 0 0).
Instances come from ENV_PARAMS.CNF_DATA_DIR (every .cnf file of one size; no train / eval split, as the reference)
or, with ``generation.ENABLED``, from a pool of NUM_TRAIN planted instances drawn on the device
(ENV_PARAMS.NUM_VARS / NUM_CLAUSES give the size; CNF_DATA_DIR is not read).
Resume (TRAIN_PARAMS.RESUME_CKPT_PATH, runner:315-346): the parameters of the directory's latest ``cycle_``
checkpoint, both heads re-initialised from SEED, fresh optimiser state and step.  A path without a checkpoint is
an error.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time
from datetime import datetime
from typing import Dict, List, Optional

import numpy as np

from ..utils.generation import parse_generation, train_pool_key
from .mappo_runner import load_config  # the YAML file with hydra-style section.KEY=VALUE overrides

LOG_FILE = "train_eval_log.txt"
LOG_FIELDS = ("# Fields: cycle | "
              "train_loss_total train_loss_value train_loss_policy train_entropy | "
              "train_value_mean train_value_std train_reward_mean train_reward_std | "
              "train_ep_num train_solve_rate train_avg_len train_avg_return | "
              "eval_solve_rate eval_avg_len eval_avg_return eval_episodes\n")

# section -> {key: default}: the keys a section may hold (anything else is refused)
SECTIONS = {
    "ENV_PARAMS": {"CNF_DATA_DIR": "data", "NUM_VARS": 0, "NUM_CLAUSES": 0, "WRAPPER_PARAMS": {}},
    "WRAPPER_PARAMS": {"max_clause_len": 3, "c_bonus": 5.0, "alpha": 1.0, "max_steps": 750},
    "MODEL_PARAMS": {"HIDDEN_DIM": 128, "NUM_MESSAGE_PASSING_STEP": 8},
    "TRAIN_PARAMS": {"RESUME_CKPT_PATH": None, "LR": 1e-4, "ANNEAL_LR": True, "NUM_CYCLES": 5000, "NUM_ENVS": 4,
                     "NUM_STEPS": 750, "EVAL_EPISODES": 50, "EVAL_MIN_TRAIN_SOLVE_RATE": 0.70,
                     "MICROBATCH_BYTES": None},
    "PPO_PARAMS": {"GAMMA": 0.99, "GAE_LAMBDA": 0.95, "CLIP_EPS": 0.2, "VF_COEF": 0.5, "ENT_COEF": 0.01,
                   "UPDATE_EPOCHS": 2, "NUM_MINIBATCHES": 4, "MAX_GRAD_NORM": None},
}
TOP_LEVEL = {"SEED", "SAVE_DIR", "ENV_PARAMS", "MODEL_PARAMS", "TRAIN_PARAMS", "PPO_PARAMS", "generation"}


def _section(config: Dict, name: str, where: str) -> Dict:
    sec = config.get(name)
    sec = {} if sec is None else sec
    if not isinstance(sec, dict):
        raise ValueError(f"{where}{name} must be a mapping, got {sec!r}")
    unknown = sorted(set(sec) - set(SECTIONS[name]))
    if unknown:
        raise ValueError(f"{where}{name}: unknown key(s) {unknown}; known: {sorted(SECTIONS[name])}")
    return {**SECTIONS[name], **sec}


def single_settings(config: Dict) -> Dict:
    """The validated settings of a loaded config as one flat dict (the learner's keys + the runner's).  Unknown
    keys and inconsistent values are refused with a message that names them."""
    unknown = sorted(set(config) - TOP_LEVEL)
    if unknown:
        raise ValueError(f"unknown top-level key(s) {unknown}; known: {sorted(TOP_LEVEL)}")
    env = _section(config, "ENV_PARAMS", "")
    wrap = _section(env, "WRAPPER_PARAMS", "ENV_PARAMS.")
    model = _section(config, "MODEL_PARAMS", "")
    train = _section(config, "TRAIN_PARAMS", "")
    ppo = _section(config, "PPO_PARAMS", "")
    gen = parse_generation(config)
    s = {"SEED": int(config.get("SEED", 0)), "SAVE_DIR": str(config.get("SAVE_DIR", "experiments/single_rl")),
         "CNF_DATA_DIR": env["CNF_DATA_DIR"], "NUM_VARS": int(env["NUM_VARS"]), "NUM_CLAUSES": int(env["NUM_CLAUSES"]),
         "c_bonus": float(wrap["c_bonus"]), "max_steps": int(wrap["max_steps"]),
         "HIDDEN_DIM": int(model["HIDDEN_DIM"]), "NUM_MESSAGE_PASSING_STEP": int(model["NUM_MESSAGE_PASSING_STEP"]),
         **{k: train[k] for k in SECTIONS["TRAIN_PARAMS"]}, **{k: ppo[k] for k in SECTIONS["PPO_PARAMS"]},
         "generation": gen}
    for k in ("NUM_CYCLES", "NUM_ENVS", "NUM_STEPS", "UPDATE_EPOCHS", "NUM_MINIBATCHES", "max_steps", "HIDDEN_DIM",
              "NUM_MESSAGE_PASSING_STEP"):
        if isinstance(s[k], bool) or not isinstance(s[k], int) or s[k] < 1:
            raise ValueError(f"{k} must be an integer >= 1, got {s[k]!r}")
    if isinstance(s["EVAL_EPISODES"], bool) or not isinstance(s["EVAL_EPISODES"], int) or s["EVAL_EPISODES"] < 0:
        raise ValueError(f"TRAIN_PARAMS.EVAL_EPISODES must be an integer >= 0, got {s['EVAL_EPISODES']!r}")
    if not isinstance(s["ANNEAL_LR"], bool):
        raise ValueError(f"TRAIN_PARAMS.ANNEAL_LR must be true or false, got {s['ANNEAL_LR']!r}")
    if (s["NUM_ENVS"] * s["NUM_STEPS"]) % s["NUM_MINIBATCHES"]:
        raise ValueError(f"NUM_ENVS * NUM_STEPS = {s['NUM_ENVS'] * s['NUM_STEPS']} must be divisible by "
                         f"PPO_PARAMS.NUM_MINIBATCHES = {s['NUM_MINIBATCHES']}")
    if not 0.0 <= float(s["EVAL_MIN_TRAIN_SOLVE_RATE"]) <= 1.0:
        raise ValueError(f"TRAIN_PARAMS.EVAL_MIN_TRAIN_SOLVE_RATE must be in [0, 1], got "
                         f"{s['EVAL_MIN_TRAIN_SOLVE_RATE']!r}")
    if not float(s["LR"]) > 0.0 or not float(s["CLIP_EPS"]) > 0.0:
        raise ValueError(f"TRAIN_PARAMS.LR and PPO_PARAMS.CLIP_EPS must be > 0, got {s['LR']!r}, {s['CLIP_EPS']!r}")
    if s["MAX_GRAD_NORM"] is not None and not 0.0 < float(s["MAX_GRAD_NORM"]) < float("inf"):
        raise ValueError(f"PPO_PARAMS.MAX_GRAD_NORM must be positive and finite, got {s['MAX_GRAD_NORM']!r}")
    if gen.enabled:
        if s["NUM_VARS"] < 1 or s["NUM_CLAUSES"] < 1:
            raise ValueError("generation.ENABLED needs ENV_PARAMS.NUM_VARS and ENV_PARAMS.NUM_CLAUSES (the size of "
                             "the generated instances)")
        if gen.refresh_every:
            raise ValueError("generation.REFRESH_EVERY must be 0 here: the single-agent runner trains on one pool")
    if s["MICROBATCH_BYTES"] is None:
        del s["MICROBATCH_BYTES"]  # activation_plan's default
    return s


def log_line(cycle: int, tr: Dict, ev: Dict) -> str:
    """One line of train_eval_log.txt in the reference's field order (runner:501-509)."""
    return (f"{cycle} | "
            f"{tr['loss_total']:.6f} {tr['loss_value']:.6f} {tr['loss_policy']:.6f} {tr['entropy']:.6f} | "
            f"{tr['value_mean']:.6f} {tr['value_std']:.6f} {tr['reward_mean']:.6f} {tr['reward_std']:.6f} | "
            f"{tr['train_ep_num']} {tr['train_solve_rate']:.6f} {0.0:.6f} {0.0:.6f} | "
            f"{ev['eval_solve_rate']:.6f} {ev['eval_avg_len']:.6f} {ev['eval_avg_return']:.6f} "
            f"{ev['eval_episodes']}\n")


def better_eval(ev: Dict, best_solve: float, best_len: float) -> bool:
    """runner:482-483: a higher solve rate, or the same one in fewer steps."""
    return ev["eval_solve_rate"] > best_solve or (abs(ev["eval_solve_rate"] - best_solve) < 1e-9
                                                  and ev["eval_avg_len"] < best_len)


def resume(net, path: str, seed: int, log=print) -> None:
    """runner:315-346: parameters only, heads back to the seed's initial draw, optimiser state and step cleared."""
    from ..utils import checkpoints as ck

    st = ck.restore_checkpoint(path, "cycle_", None)
    if st is None:
        raise FileNotFoundError(f"TRAIN_PARAMS.RESUME_CKPT_PATH={path!r} holds no cycle_<n> checkpoint")
    ck.load_train_state(net, st, reset_optimizer=True)
    net.reset_heads(seed)
    log(f"resumed the GNN body from {path}; actor / critic heads and optimiser state re-initialised")


def run(config: Dict, log=print) -> Dict:
    import torch

    from ..envs.multi_agent_sat_env import ProblemPool
    from ..learners.single_gnn import GNNSingleActorCritic
    from ..learners.single_ppo_learner import SinglePPOLearner, make_single_env
    from ..random import PRNGKey, split
    from ..utils import checkpoints as ck
    from ..utils.data_parser import clauses_array, load_cnf_problems
    from ..utils.generate_cnf_dataset import has_isolated_variable

    s = single_settings(config)
    seed, gen = s["SEED"], s["generation"]
    random.seed(seed)
    np.random.seed(seed)
    key = PRNGKey(seed)
    if gen.enabled:
        V, C = s["NUM_VARS"], s["NUM_CLAUSES"]
        env = make_single_env(V, C, s["max_steps"], s["c_bonus"])
        pool = ProblemPool.generate(env, gen.num_train, train_pool_key(seed, 0), reject_isolated=True,
                                    max_attempts=gen.max_attempts)
        log(f"[*] generated pool: {gen.num_train} planted instances of uf{V}-{C}")
    else:
        raw = load_cnf_problems(s["CNF_DATA_DIR"])
        if not raw:
            raise FileNotFoundError(f"no .cnf problems found in ENV_PARAMS.CNF_DATA_DIR={s['CNF_DATA_DIR']!r}")
        V, C = raw[0]["num_vars"], raw[0]["num_clauses"]
        for p in raw:
            if (p["num_vars"], p["num_clauses"]) != (V, C):
                raise ValueError(f"{p['name']} is V={p['num_vars']}, C={p['num_clauses']}; the first problem is "
                                 f"V={V}, C={C} (one size per run, as the reference)")
        iso = [p["name"] for p in raw if has_isolated_variable(clauses_array(p), V)]
        if iso:
            log(f"warning: {len(iso)} problem(s) leave a variable in no clause ({', '.join(iso[:5])}): the learner "
                f"stops with FloatingPointError if an update turns non-finite (tests/test_isolated_variable.py)")
        env = make_single_env(V, C, s["max_steps"], s["c_bonus"])
        pool = env.make_pool(np.stack([clauses_array(p) for p in raw]))
        log(f"[*] {len(raw)} problems of uf{V}-{C}")
    net = GNNSingleActorCritic(s["HIDDEN_DIM"], s["NUM_MESSAGE_PASSING_STEP"], V, seed=seed)
    if s["RESUME_CKPT_PATH"]:
        resume(net, str(s["RESUME_CKPT_PATH"]), seed, log)
    learner = SinglePPOLearner(s, env, net, pool, templates="device" if gen.enabled else "host")
    time_str = datetime.now().strftime("%Y-%m-%d_%H-%M-%S")
    run_dir = os.path.abspath(os.path.join(s["SAVE_DIR"], time_str))
    ckpt_dir = os.path.join(run_dir, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    log_path = os.path.join(run_dir, LOG_FILE)
    key, k_rs = split(key, 2)
    rs = learner.init_runner_state(k_rs)
    g = torch.Generator().manual_seed(seed)
    best_solve, best_len = -1.0, float("inf")
    n_cycles, anneal = s["NUM_CYCLES"], s["ANNEAL_LR"]
    state_dict = lambda: ck.train_state_dict(net, anneal)
    t0 = time.time()
    last_tr, last_ev = {}, {}
    with open(log_path, "w", encoding="utf-8") as f:
        f.write(f"# Train/Eval Log | start_time={time_str} | seed={seed}\n")
        f.write(LOG_FIELDS)
        for cycle in range(1, n_cycles + 1):
            rs, tr = learner.train_cycle(rs, g)
            log(f"cycle {cycle}: loss {tr['loss_total']:.3f} V {tr['loss_value']:.3f} pi {tr['loss_policy']:.3f} "
                f"H {tr['entropy']:.3f} | value {tr['value_mean']:.3f}+-{tr['value_std']:.3f} reward "
                f"{tr['reward_mean']:.3f}+-{tr['reward_std']:.3f} | episodes {tr['train_ep_num']} solved "
                f"{tr['train_solve_rate']:.1%} | grad norm {tr['grad_norm']:.3g}")
            ev = {"eval_solve_rate": 0.0, "eval_avg_len": float("inf"), "eval_avg_return": 0.0, "eval_episodes": 0}
            if s["EVAL_EPISODES"] > 0 and tr["train_solve_rate"] >= float(s["EVAL_MIN_TRAIN_SOLVE_RATE"]):
                pick = torch.randint(0, pool.num_problems, (s["EVAL_EPISODES"],), generator=g)
                key, k_ev = split(key, 2)
                ev = learner.evaluate(pick, s["max_steps"], key=k_ev)
                log(f"  eval: solved {ev['eval_solve_rate']:.1%}, length {ev['eval_avg_len']:.2f}, return "
                    f"{ev['eval_avg_return']:+.4f}, {ev['eval_episodes']} episodes")
                if better_eval(ev, best_solve, best_len):
                    best_solve, best_len = ev["eval_solve_rate"], ev["eval_avg_len"]
                    ck.prune_checkpoints(ckpt_dir, "best_eval_", 0)  # overwrite=True: one best checkpoint
                    ck.save_checkpoint(ckpt_dir, state_dict(), cycle, "best_eval_", overwrite=True)
            ck.save_checkpoint(ckpt_dir, state_dict(), cycle, "cycle_", overwrite=True)
            ck.prune_checkpoints(ckpt_dir, "cycle_", 3)
            f.write(log_line(cycle, tr, ev))
            f.flush()
            last_tr, last_ev = tr, ev
    ck.save_checkpoint(ckpt_dir, state_dict(), n_cycles, "final_model_", overwrite=True)
    log(f"final model and {LOG_FILE} in {run_dir}")
    return {"run_dir": run_dir, "ckpt_dir": ckpt_dir, "log_path": log_path, "train_seconds": time.time() - t0,
            "last_train": last_tr, "last_eval": last_ev, "best_eval_solve_rate": best_solve}


def main(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="configs/SINGLE_RL_PPO_CONFIG.yaml")
    ap.add_argument("overrides", nargs="*", help="section.KEY=VALUE (hydra-style)")
    a = ap.parse_args(argv)
    run(load_config(a.config, a.overrides))


if __name__ == "__main__":
    main(sys.argv[1:])
