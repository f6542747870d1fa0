"""Batched WalkSAT/SKC on the device (``msat_walksat``; the algorithm is fixed in include/marlsat.h).

``walksat`` is one launch: S independent samples, each a run of at most ``max_flips`` flips on one instance of
a ``ProblemPool``.  ``solve_pool`` wraps it in random restarts until every instance has a solution or the
rounds run out: the expert solutions that behavioural cloning needs for CNF files nobody planted
(``utils.sat_solver``), and the classical local-search baseline beside ``evaluate_policy``.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from ..random import Key, as_key


def walksat_forms() -> int:
    """Number of kernel forms; ``form=0`` picks one, ``1..n`` force one."""
    return int(_lib.lib.msat_walksat_forms())


def noise_p32(noise: float) -> int:
    """The noise probability as the kernel compares it: a random walk step is taken when a uniform uint32 draw
    is below this value (and no candidate has break count 0)."""
    if not 0.0 <= float(noise) <= 1.0:
        raise ValueError(f"noise must be in [0, 1], got {noise}")
    return min(int(float(noise) * 2 ** 32), 2 ** 32 - 1)


def walksat(pool, problem_idx, *, key=None, max_flips: int, noise: float = 0.5, assignments=None, form: int = 0):
    """Sample s runs instance ``problem_idx[s]`` of ``pool`` from ``assignments[s]`` ((S, V) 0/1), or, when
    ``assignments`` is None, from the assignment ``env.reset`` would draw for env s under ``key``.  Returns the
    device tensors ``assignments (S, V) uint8, solved (S,) uint8, flips (S,) int32, num_unsat (S,) int32``."""
    k = as_key(key)
    dev = pool.device
    if torch.is_tensor(problem_idx):
        host_idx = None
        pidx = problem_idx.to(device=dev, dtype=torch.int32).contiguous()
    else:
        host_idx = np.asarray(problem_idx, dtype=np.int64).reshape(-1)
        if host_idx.size and (host_idx.min() < 0 or host_idx.max() >= pool.num_problems):
            raise ValueError(f"problem_idx out of [0, {pool.num_problems})")
        pidx = torch.from_numpy(host_idx.astype(np.int32)).to(dev)
    if pidx.dim() != 1:
        raise ValueError(f"problem_idx must be (S,), got {tuple(pidx.shape)}")
    S, V = int(pidx.numel()), int(pool.num_vars)
    init = None
    if assignments is not None:
        init = torch.as_tensor(np.asarray(assignments) if not torch.is_tensor(assignments) else assignments)
        init = init.to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(init.shape) != (S, V):
            raise ValueError(f"assignments must be (S, V) = ({S}, {V}), got {tuple(init.shape)}")
    x = torch.empty((S, V), dtype=torch.uint8, device=dev)
    solved = torch.empty((S,), dtype=torch.uint8, device=dev)
    flips = torch.empty((S,), dtype=torch.int32, device=dev)
    nun = torch.empty((S,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib.msat_walksat(pool.packed.data_ptr(), pool.num_problems, V, pool.num_clauses, pidx.data_ptr(),
                                     S, _lib.ptr(init), int(max_flips), noise_p32(noise), k.seed, k.counter,
                                     int(form), x.data_ptr(), solved.data_ptr(), flips.data_ptr(), nun.data_ptr(),
                                     _lib.stream_ptr(dev)), "msat_walksat")
    return x, solved, flips, nun


def solve_pool(pool, *, tries: int = 8, max_flips: int = 100_000, max_rounds: int = 4, noise: float = 0.5,
               key=None, init_assignments=None) -> Dict[str, np.ndarray]:
    """One solution per instance of ``pool`` by random restarts.  Round r launches ``tries`` samples for every
    instance still unsolved (samples i * tries .. i * tries + tries - 1 for the i-th of them, in instance order)
    with ``counter = key.counter + r``, so every restart is a fresh draw.  The winner of an instance is the
    lowest sample index that solved it, in its earliest solving round.  One device -> host read per round.

    ``init_assignments`` ((N, V) 0/1, host or device; e.g. an assignment predictor's output): round 0 starts every
    one of an instance's ``tries`` samples from its row instead of a random draw; the samples still differ by their
    Philox row streams, and an instance its row already satisfies is solved with 0 flips.  Later rounds are the
    random restarts they are without it, at the same counters.  None: every output is what it is without the
    keyword, bit for bit.

    Returns host arrays over the N instances: ``solved`` bool, ``solution`` (N, V) uint8 (zeros where unsolved),
    ``flips`` int32, ``round`` int32 and ``try`` int32 (-1 where unsolved)."""
    if tries < 1 or max_rounds < 0:
        raise ValueError(f"solve_pool: tries={tries}, max_rounds={max_rounds}")
    k = as_key(key)
    N, V = int(pool.num_problems), int(pool.num_vars)
    out = {"solved": np.zeros(N, dtype=bool), "solution": np.zeros((N, V), dtype=np.uint8),
           "flips": np.full(N, -1, dtype=np.int32), "round": np.full(N, -1, dtype=np.int32),
           "try": np.full(N, -1, dtype=np.int32)}
    init = None
    if init_assignments is not None:
        init = torch.as_tensor(np.asarray(init_assignments) if not torch.is_tensor(init_assignments)
                               else init_assignments).to(device=pool.device, dtype=torch.uint8)
        if tuple(init.shape) != (N, V):
            raise ValueError(f"init_assignments must be (N, V) = ({N}, {V}), got {tuple(init.shape)}")
    for r in range(int(max_rounds)):
        todo = np.flatnonzero(~out["solved"])
        if todo.size == 0:
            break
        pidx = np.repeat(todo, tries)
        start = init.repeat_interleave(tries, dim=0) if init is not None and r == 0 else None  # round 0: every instance
        x, ok, fl, _ = walksat(pool, pidx, key=Key(k.seed, (k.counter + r) & ((1 << 64) - 1)), max_flips=max_flips,
                               noise=noise, assignments=start)
        okm = ok.reshape(todo.size, tries) != 0
        any_ok = okm.any(dim=1)
        # lowest solving try of each instance (a unique maximum: argmax leaves ties open)
        first = torch.argmax(okm.to(torch.int32) * torch.arange(tries, 0, -1, dtype=torch.int32, device=x.device),
                             dim=1)
        rows = torch.arange(todo.size, device=x.device) * tries + first
        packed = torch.cat([x[rows].to(torch.int32), fl[rows, None], first[:, None].to(torch.int32),
                            any_ok[:, None].to(torch.int32)], dim=1).cpu().numpy()  # the round's one read
        won = packed[:, V + 2] != 0
        idx = todo[won]
        out["solved"][idx] = True
        out["solution"][idx] = packed[won, :V].astype(np.uint8)
        out["flips"][idx] = packed[won, V]
        out["try"][idx] = packed[won, V + 1]
        out["round"][idx] = r
    return out
