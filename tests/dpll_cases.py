"""Instances and ground truth shared by tests/test_dpll_cpu.py and tests/test_dpll_gpu.py: seeded pools, the
hand-made edge cases, brute-force satisfiability and a clause check that share nothing with tests/dpll_replay.py.
Replays are computed once per session and shared (never modified)."""
import itertools

import numpy as np

from dpll_replay import replay


def random_pool(V, C, N, seed):
    """N unplanted random 3-SAT instances (N, C, 3) int32: three distinct variables per clause, random signs."""
    rng = np.random.default_rng(seed)
    out = np.zeros((N, C, 3), dtype=np.int32)
    for n in range(N):
        for c in range(C):
            vs = rng.choice(V, size=min(3, V), replace=False) + 1
            out[n, c, :len(vs)] = vs * rng.choice([-1, 1], size=len(vs))
    return out


def pigeonhole(pigeons=4, holes=3):
    """PHP(pigeons, holes) as (1, C, 3) int32, the binary clauses padded with literal 0.  Unsatisfiable."""
    var = lambda i, j: i * holes + j + 1
    cls = [[var(i, j) for j in range(holes)] for i in range(pigeons)]
    for j in range(holes):
        for a, b in itertools.combinations(range(pigeons), 2):
            cls.append([-var(a, j), -var(b, j), 0])
    return np.asarray([cls], dtype=np.int32), pigeons * holes


def satisfied(x, clauses):
    """(C,) bool: the clauses (C, K) int32 under the 0/1 assignment x (..., V); literal 0 is false."""
    x = np.asarray(x)
    var = np.maximum(np.abs(clauses) - 1, 0)
    val = x[..., var]
    return (((clauses > 0) & (val == 1)) | ((clauses < 0) & (val == 0))).any(axis=-1)


def brute_force_sat(clauses, V):
    """True iff some of the 2^V assignments satisfies every clause of (C, K) int32.  V <= 14."""
    assert V <= 14
    allx = ((np.arange(1 << V)[:, None] >> np.arange(V)[None, :]) & 1).astype(np.uint8)
    return bool(satisfied(allx, np.asarray(clauses)).all(axis=-1).any())


# name: (clauses (1, C, K), V, status (1 SAT / 2 UNSAT), nodes or None)
HAND_MADE = {
    "x": ([[[1]]], 1, 1, 0),
    "not x": ([[[-1]]], 1, 1, 0),
    "x and not x": ([[[1], [-1]]], 1, 2, 0),
    "all-NULL clause": ([[[1, 2, 0], [0, 0, 0], [-1, 3, 2], [2, -3, 0]]], 3, 2, 0),
    "duplicates": ([[[1, 1, 2], [-1, -1, 0], [-2, -2, -2], [3, 3, 0]]], 3, 2, 0),
    "duplicate unit": ([[[1, 1, 0], [-1, 2, 2], [3, -2, 3]]], 3, 1, 0),
    "tautology": ([[[1, -1, 2], [-2, 0, 0], [1, 3, 0], [-1, -3, 0]]], 3, 1, None),
    "tautology alone": ([[[1, -1, 2]]], 2, 1, 1),
    "contradicting units of one pass": ([[[1, 2, 0], [-1, 0, 0], [2, 3, 0], [-2, 3, 0], [-3, 0, 0]]], 3, 2, 0),
    "contradicting units under a decision": ([[[1, 2, 3], [-1, 2, 0], [-1, -2, 0], [1, -3, 2], [1, -3, -2]]], 3, 1,
                                             None),
}


def hand_made(name):
    cl, V, status, nodes = HAND_MADE[name]
    return np.asarray(cl, dtype=np.int32), V, status, nodes


_REFS = {}


def shared_replay(key, clauses, V, pidx, cubes=None, cube_bits=0, max_nodes=0):
    """replay(...) once per session under `key`."""
    if key not in _REFS:
        _REFS[key] = replay(clauses, V, pidx, cubes, cube_bits, max_nodes)
    return _REFS[key]
