"""Assignment predictor: supervised training driver -- drop-in for src/runners/bc_runner.py.

    python -m marlsat.runners.bc_runner --config configs/ASSIGN_BC_CONFIG.yaml [KEY=VALUE ...]

A GNN reads a formula and predicts, for every variable, its value in an expert solution (learners/assign_gnn.py,
learners/assign_learner.py).  The flow is the reference's ``main()`` with its constants as config keys:
  1. (.cnf, .sol) pairs of CNF_DATA_DIR / SOL_DATA_DIR (all of one size: they form one device pool), or, with
     ``generation.ENABLED``, NUM_TRAIN planted instances drawn on the device whose planted solutions are the experts;
  2. a seeded shuffle, then the first TRAIN_RATIO of the instances train and the rest validate (bc_runner.py:82-85);
  3. per epoch one pass over each split and one log line with the reference's fields, order and formats
     (bc_runner.py:144-147), printed and appended to ``<run_dir>/bc_log.txt``;
  4. ``checkpoints/best_<epoch>`` (the parameter tree alone, one kept) whenever the validation Sol-Acc is strictly
     greater than the best so far (bc_runner.py:150-159);
  5. ``<run_dir>/assign_model.json``: H, L and the input mode, so ``load_predictor(run_dir)`` needs no config.
The network's input assignment is INPUT: ``zeros`` (the formula alone) or ``corrupted`` (NUM_SAMPLES_PER_EXPERT
copies of the expert with CORRUPTION_LEVEL variables flipped, msat_bc_corrupt; the labels stay the expert).  The
reference writes the label itself into a variable feature (graph_constructor.py:64); that leak is not reproduced
(DESIGN.md §17).  Single process.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time
from datetime import datetime
from typing import Dict, List, Optional

import numpy as np

from ..utils.generation import instance_name, parse_generation, train_pool_key
from .mappo_runner import load_config  # the YAML file with hydra-style KEY=VALUE overrides

LOG_FILE = "bc_log.txt"
MODEL_FILE = "assign_model.json"
BEST_PREFIX = "best_"
INPUT_MODES = ("zeros", "corrupted")

DEFAULTS = {"SEED": 0, "LEARNING_RATE": 1e-4, "EPOCHS": 100, "BATCH_SIZE": 32, "TRAIN_RATIO": 0.8,
            "CNF_DATA_DIR": "data/uf20-91", "SOL_DATA_DIR": "data/uf20-91-answer", "SAVE_DIR": "experiments/bc",
            "network": {}, "MICROBATCH_BYTES": None, "SOLVE_MISSING_EXPERTS": False, "INPUT": "zeros",
            "NUM_SAMPLES_PER_EXPERT": 5, "CORRUPTION_LEVEL": 3, "NUM_VARS": 0, "NUM_CLAUSES": 0, "generation": {}}
NETWORK_DEFAULTS = {"H": 128, "L": 8}


def _pos_int(s: Dict, k: str, lo: int = 1) -> None:
    if isinstance(s[k], bool) or not isinstance(s[k], int) or s[k] < lo:
        raise ValueError(f"{k} must be an integer >= {lo}, got {s[k]!r}")


def assign_settings(config: Dict) -> Dict:
    """The validated settings of a loaded config as one flat dict.  Unknown keys and inconsistent values are refused
    with a message that names them."""
    unknown = sorted(set(config) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"unknown key(s) {unknown}; known: {sorted(DEFAULTS)}")
    net = config.get("network")
    net = {} if net is None else net
    if not isinstance(net, dict):
        raise ValueError(f"network must be a mapping, got {net!r}")
    unknown = sorted(set(net) - set(NETWORK_DEFAULTS))
    if unknown:
        raise ValueError(f"network: unknown key(s) {unknown}; known: {sorted(NETWORK_DEFAULTS)}")
    s = {**DEFAULTS, **{k: v for k, v in config.items() if k not in ("network", "generation")},
         **{**NETWORK_DEFAULTS, **net}}
    del s["network"]
    s["generation"] = gen = parse_generation(config)
    for k in ("EPOCHS", "BATCH_SIZE", "H", "L", "NUM_SAMPLES_PER_EXPERT"):
        _pos_int(s, k)
    for k in ("SEED", "CORRUPTION_LEVEL", "NUM_VARS", "NUM_CLAUSES"):
        _pos_int(s, k, 0)
    if not float(s["LEARNING_RATE"]) > 0.0:
        raise ValueError(f"LEARNING_RATE must be > 0, got {s['LEARNING_RATE']!r}")
    if isinstance(s["TRAIN_RATIO"], bool) or not 0.0 < float(s["TRAIN_RATIO"]) < 1.0:
        raise ValueError(f"TRAIN_RATIO must be in (0, 1), got {s['TRAIN_RATIO']!r}")
    if s["INPUT"] not in INPUT_MODES:
        raise ValueError(f"INPUT must be one of {list(INPUT_MODES)}, got {s['INPUT']!r}")
    if not isinstance(s["SOLVE_MISSING_EXPERTS"], bool):
        raise ValueError(f"SOLVE_MISSING_EXPERTS must be true or false, got {s['SOLVE_MISSING_EXPERTS']!r}")
    if gen.enabled:
        if s["NUM_VARS"] < 1 or s["NUM_CLAUSES"] < 1:
            raise ValueError("generation.ENABLED needs NUM_VARS and NUM_CLAUSES (the size of the generated instances)")
        if gen.refresh_every:
            raise ValueError("generation.REFRESH_EVERY must be 0 here: the predictor trains on one pool")
    if s["MICROBATCH_BYTES"] is None:
        del s["MICROBATCH_BYTES"]  # activation_plan's default
    return s


def log_line(epoch: int, tr: Dict, va: Dict) -> str:
    """bc_runner.py:144-147: the reference's fields, order and formats."""
    return (f"Epoch {epoch:03d} | Train Loss: {tr['loss']:.4f}, Train Var-Acc: {tr['var_acc']:.4f}, "
            f"Train Sol-Acc: {tr['sol_acc']:.4f} | "
            f"Val Loss: {va['loss']:.4f}, Val Var-Acc: {va['var_acc']:.4f}, Val Sol-Acc: {va['sol_acc']:.4f}")


def split_instances(n: int, ratio: float, seed: int):
    """bc_runner.py:82-85 with a seeded shuffle: (train instance ids, validation instance ids)."""
    order = list(range(n))
    random.Random(seed).shuffle(order)
    cut = int(n * ratio)
    if cut < 1 or cut >= n:
        raise ValueError(f"{n} instance(s) at TRAIN_RATIO={ratio}: {cut} train, {n - cut} validation; both splits "
                         f"need at least one")
    return np.array(order[:cut], np.int64), np.array(order[cut:], np.int64)


def save_best(ckpt_dir: str, net, epoch: int) -> str:
    """The parameter tree alone as ``best_<epoch>``, the earlier best removed (flax's overwrite=True keeps one)."""
    from ..utils import checkpoints as ck

    ck.prune_checkpoints(ckpt_dir, BEST_PREFIX, 0)
    return ck.save_checkpoint(ckpt_dir, ck.nest({k: v.astype(np.float32) for k, v in net.to_flax().items()}), epoch,
                              BEST_PREFIX, overwrite=True)


def load_predictor(run_dir: str, device=None):
    """(network, model description) of a run directory: assign_model.json's H and L, the parameters of its
    ``checkpoints/best_<epoch>``.  The description holds H, L, INPUT and CORRUPTION_LEVEL."""
    from ..learners.assign_gnn import GNNAssignmentPredictor
    from ..utils import checkpoints as ck

    with open(os.path.join(run_dir, MODEL_FILE)) as f:
        desc = json.load(f)
    tree = ck.restore_checkpoint(os.path.join(run_dir, "checkpoints"), BEST_PREFIX, None)
    if tree is None:
        raise FileNotFoundError(f"{run_dir!r} holds no checkpoints/{BEST_PREFIX}<epoch>")
    net = GNNAssignmentPredictor(int(desc["H"]), int(desc["L"]), device=device)
    net.load_flax(ck.flatten(tree))
    return net, desc


def run(config: Dict, log=print) -> Dict:
    import torch

    from ..envs.multi_agent_sat_env import ProblemPool
    from ..learners.assign_gnn import GNNAssignmentPredictor
    from ..learners.assign_learner import AssignLearner
    from ..random import PRNGKey, split
    from ..utils.generate_cnf_dataset import has_isolated_variable
    from .behavioral_cloning import corrupt_device, load_expert_data, solve_missing_experts

    s = assign_settings(config)
    seed, gen = s["SEED"], s["generation"]
    random.seed(seed)
    np.random.seed(seed)
    key = PRNGKey(seed)
    if gen.enabled:
        V, C = s["NUM_VARS"], s["NUM_CLAUSES"]
        pool = ProblemPool.generate((V, C), gen.num_train, train_pool_key(seed, 0), reject_isolated=True,
                                    max_attempts=gen.max_attempts)
        sols = pool.planted.cpu().numpy()
        names = [instance_name(V, i) for i in range(gen.num_train)]
        log(f"[*] generated pool: {gen.num_train} planted instances of uf{V}-{C}")
    else:
        if s["SOLVE_MISSING_EXPERTS"]:
            solve_missing_experts(s["CNF_DATA_DIR"], s["SOL_DATA_DIR"], seed, log)
        experts = load_expert_data(s["CNF_DATA_DIR"], s["SOL_DATA_DIR"])
        if not experts:
            raise FileNotFoundError(f"no (.cnf, .sol) pairs found in {s['CNF_DATA_DIR']!r} / {s['SOL_DATA_DIR']!r}")
        C, V = experts[0]["problem_clauses"].shape[0], experts[0]["expert_solution"].shape[0]
        for e in experts:
            if e["problem_clauses"].shape[0] != C or e["expert_solution"].shape[0] != V:
                raise ValueError(f"{e['name']}: {e['problem_clauses'].shape[0]} clauses, a model of "
                                 f"{e['expert_solution'].shape[0]} values; the first pair is V={V}, C={C} (the files of "
                                 f"a run form one pool: one size per run)")
        iso = [e["name"] for e in experts if has_isolated_variable(e["problem_clauses"], V)]
        if iso:
            log(f"warning: {len(iso)} problem(s) leave a variable in no clause ({', '.join(iso[:5])}): the learner "
                f"stops with FloatingPointError if an update turns non-finite (tests/test_isolated_variable.py)")
        pool = ProblemPool(np.stack([e["problem_clauses"] for e in experts]), V)
        sols = np.stack([e["expert_solution"] for e in experts]).astype(np.uint8)
        names = [e["name"] for e in experts]
        log(f"[*] {len(experts)} expert problem-solution pairs of uf{V}-{C}")
    n = len(names)
    train_inst, val_inst = split_instances(n, float(s["TRAIN_RATIO"]), seed)
    log(f"Training on {len(train_inst)} samples, validating on {len(val_inst)} samples.")
    # dataset rows: one per instance (zeros) or NUM_SAMPLES_PER_EXPERT per instance (corrupted), instance-major
    if s["INPUT"] == "zeros":
        per = 1
        x = torch.zeros((n, V), dtype=torch.uint8, device=pool.device)
    else:
        per = s["NUM_SAMPLES_PER_EXPERT"]
        key, k_data = split(key, 2)
        x = corrupt_device(sols, per, s["CORRUPTION_LEVEL"], k_data, pool.device)
    pidx = np.repeat(np.arange(n, dtype=np.int32), per)
    rows_of = lambda inst: (inst[:, None] * per + np.arange(per)[None, :]).reshape(-1).astype(np.int32)
    train_rows, val_rows = rows_of(train_inst), rows_of(val_inst)
    net = GNNAssignmentPredictor(s["H"], s["L"], seed=seed)
    learner = AssignLearner(s, net, pool, templates="device" if gen.enabled else "host")
    learner.set_data(pidx, x, np.repeat(sols, per, axis=0))
    time_str = datetime.now().strftime("%m-%d_%H-%M-%S")
    run_dir = os.path.abspath(os.path.join(s["SAVE_DIR"], time_str))
    ckpt_dir = os.path.join(run_dir, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    with open(os.path.join(run_dir, MODEL_FILE), "w") as f:
        json.dump({"H": s["H"], "L": s["L"], "INPUT": s["INPUT"], "CORRUPTION_LEVEL": s["CORRUPTION_LEVEL"],
                   "NUM_VARS": V, "NUM_CLAUSES": C, "SEED": seed}, f, indent=1)
        f.write("\n")
    g = torch.Generator().manual_seed(seed)
    best, best_epoch = -1.0, 0
    history = []
    t0 = time.time()
    with open(os.path.join(run_dir, LOG_FILE), "a", encoding="utf-8") as logf:
        for epoch in range(1, s["EPOCHS"] + 1):
            tr = learner.train_epoch(g, rows=train_rows)
            va = learner.evaluate(val_rows)
            line = log_line(epoch, tr, va)
            log(line)
            logf.write(line + "\n")
            logf.flush()
            history.append((tr, va))
            if va["sol_acc"] > best:
                best, best_epoch = va["sol_acc"], epoch
                save_best(ckpt_dir, net, epoch)
                log(f"New best model saved at epoch {epoch} with Val Sol-Acc={best:.4f}")
    torch.cuda.synchronize()
    log("Training finished!")
    return {"run_dir": run_dir, "ckpt_dir": ckpt_dir, "log_path": os.path.join(run_dir, LOG_FILE),
            "train_seconds": time.time() - t0, "history": history, "best_val_sol_acc": best, "best_epoch": best_epoch,
            "train_instances": [names[i] for i in train_inst], "val_instances": [names[i] for i in val_inst],
            "network": net, "learner": learner, "val_rows": val_rows, "train_rows": train_rows}


def main(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="configs/ASSIGN_BC_CONFIG.yaml")
    ap.add_argument("overrides", nargs="*", help="KEY=VALUE or section.KEY=VALUE (hydra-style)")
    a = ap.parse_args(argv)
    run(load_config(a.config, a.overrides))


if __name__ == "__main__":
    main(sys.argv[1:])
