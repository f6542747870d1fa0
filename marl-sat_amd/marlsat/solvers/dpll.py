"""Batched DPLL on the device (``msat_dpll``; the algorithm is fixed in include/marlsat.h): the complete search
beside WalkSAT's local search.  A sample returns a model, the verdict that none exists, or, when its node budget
runs out, neither.

``dpll`` is one launch: S independent samples, each the search of one instance of a ``ProblemPool`` under one cube
(the phases of its first ``cube_bits`` decisions).  ``decide_pool`` wraps it in rounds of growing budget until every
instance is decided or the rounds run out: what ``utils.sat_solver --complete`` runs on the instances WalkSAT
leaves unsolved.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .. import _lib

UNKNOWN, SAT, UNSAT = 0, 1, 2  # MSAT_DPLL_UNKNOWN / _SAT / _UNSAT
BUDGET_FACTOR = 8              # decide_pool: a round's node budget is this many times the round's before


def dpll(pool, problem_idx, *, cubes=None, cube_bits: int = 0, max_nodes: int):
    """Sample s searches instance ``problem_idx[s]`` of ``pool`` under cube ``cubes[s]`` (None: cube 0), at most
    ``max_nodes`` branch nodes.  Returns the device tensors ``status (S,) uint8`` (0 unknown, 1 SAT, 2 UNSAT),
    ``assignments (S, V) uint8`` (a model where SAT, zeros otherwise), ``nodes``, ``conflicts``, ``propagations``
    ``(S,) int32``."""
    dev = pool.device
    if torch.is_tensor(problem_idx):
        pidx = problem_idx.to(device=dev, dtype=torch.int32).contiguous()
    else:
        host_idx = np.asarray(problem_idx, dtype=np.int64).reshape(-1)
        if host_idx.size and (host_idx.min() < 0 or host_idx.max() >= pool.num_problems):
            raise ValueError(f"problem_idx out of [0, {pool.num_problems})")
        pidx = torch.from_numpy(host_idx.astype(np.int32)).to(dev)
    if pidx.dim() != 1:
        raise ValueError(f"problem_idx must be (S,), got {tuple(pidx.shape)}")
    S, V = int(pidx.numel()), int(pool.num_vars)
    if not 0 <= int(cube_bits) <= 30:
        raise ValueError(f"cube_bits must be in [0, 30], got {cube_bits}")
    if int(max_nodes) < 0:
        raise ValueError(f"max_nodes must be >= 0, got {max_nodes}")
    cube = None
    if cubes is not None:
        if torch.is_tensor(cubes):
            cube = cubes.to(device=dev, dtype=torch.int32).contiguous()
        else:
            host_cube = np.asarray(cubes, dtype=np.int64).reshape(-1)
            if host_cube.size and (host_cube.min() < 0 or host_cube.max() >= 1 << int(cube_bits)):
                raise ValueError(f"cubes out of [0, 2^cube_bits = {1 << int(cube_bits)})")
            cube = torch.from_numpy(host_cube.astype(np.int32)).to(dev)
        if tuple(cube.shape) != (S,):
            raise ValueError(f"cubes must be (S,) = ({S},), got {tuple(cube.shape)}")
    status = torch.empty((S,), dtype=torch.uint8, device=dev)
    x = torch.empty((S, V), dtype=torch.uint8, device=dev)
    nodes = torch.empty((S,), dtype=torch.int32, device=dev)
    conflicts = torch.empty((S,), dtype=torch.int32, device=dev)
    props = torch.empty((S,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib.msat_dpll(pool.packed.data_ptr(), pool.num_problems, V, pool.num_clauses, pidx.data_ptr(),
                                  _lib.ptr(cube), S, int(cube_bits), int(max_nodes), status.data_ptr(), x.data_ptr(),
                                  nodes.data_ptr(), conflicts.data_ptr(), props.data_ptr(), _lib.stream_ptr(dev)),
               "msat_dpll")
    return status, x, nodes, conflicts, props


def decide_pool(pool, *, max_nodes: int = 4096, cube_bits: int = 4, max_rounds: int = 4) -> Dict[str, np.ndarray]:
    """Every instance of ``pool`` decided, where the budgets reach.  Round 0 searches every instance as one sample
    of at most ``max_nodes`` nodes.  Round r >= 1 takes the instances still undecided, runs each as its
    2^cube_bits cubes (samples i * 2^cube_bits + cube for the i-th of them, in instance order) and gives every
    sample ``max_nodes * BUDGET_FACTOR ** r`` nodes.  An instance is SAT when some cube is (the model of the lowest
    such cube is kept), UNSAT when every cube is, undecided otherwise.  One device -> host read per round.

    The defaults, from profiles/dpll_throughput.json: round 0's 4096 nodes decide every
    unplanted uf50-218 and uf100-430 instance of the measured pools in one launch (largest search 1,044 nodes) and
    cost at most 0.17 s at uf200-860 (41 us per node); what is left are long searches, and 16 cubes per instance cut
    the uf200 launch 4.7x for 0.1 % more nodes, under 32,768, 262,144 and 2,097,152 nodes per cube.

    Returns host arrays over the N instances: ``status`` uint8 (0 undecided, 1 SAT, 2 UNSAT), ``solution`` (N, V)
    uint8 (zeros unless SAT) and ``nodes`` int64, the sum over the instance's samples of every round."""
    if max_rounds < 0 or max_nodes < 0 or not 0 <= cube_bits <= 30:
        raise ValueError(f"decide_pool: max_nodes={max_nodes}, cube_bits={cube_bits}, max_rounds={max_rounds}")
    N, V = int(pool.num_problems), int(pool.num_vars)
    out = {"status": np.zeros(N, dtype=np.uint8), "solution": np.zeros((N, V), dtype=np.uint8),
           "nodes": np.zeros(N, dtype=np.int64)}
    dev = pool.device
    for r in range(int(max_rounds)):
        todo = np.flatnonzero(out["status"] == UNKNOWN)
        if todo.size == 0:
            break
        bits = 0 if r == 0 else int(cube_bits)
        K = 1 << bits
        budget = min(int(max_nodes) * BUDGET_FACTOR ** r, 2 ** 31 - 1)
        pidx = torch.from_numpy(np.repeat(todo, K).astype(np.int32)).to(dev)
        cubes = torch.arange(K, dtype=torch.int32, device=dev).repeat(todo.size)
        st, x, nd, _, _ = dpll(pool, pidx, cubes=cubes, cube_bits=bits, max_nodes=budget)
        stm = st.reshape(todo.size, K)
        sat = stm == SAT
        any_sat = sat.any(dim=1)
        all_unsat = (stm == UNSAT).all(dim=1)
        # lowest SAT cube of each instance (a unique maximum: argmax leaves ties open)
        first = torch.argmax(sat.to(torch.int32) * torch.arange(K, 0, -1, dtype=torch.int32, device=dev), dim=1)
        rows = torch.arange(todo.size, device=dev) * K + first
        verdict = torch.where(any_sat, SAT, torch.where(all_unsat, UNSAT, UNKNOWN)).to(torch.int64)
        model = x[rows].to(torch.int64) * any_sat[:, None].to(torch.int64)
        packed = torch.cat([model, verdict[:, None], nd.reshape(todo.size, K).to(torch.int64).sum(dim=1)[:, None]],
                           dim=1).cpu().numpy()  # the round's one read
        out["status"][todo] = packed[:, V].astype(np.uint8)
        out["solution"][todo] = packed[:, :V].astype(np.uint8)
        out["nodes"][todo] += packed[:, V + 1]
    return out
