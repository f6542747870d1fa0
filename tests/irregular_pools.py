"""Irregular CNF pools for the learning-path tests: the inputs `generate_problem_pool` never makes.

Builders only (host NumPy; nothing here touches the device).  Each builder starts from
``generate_sat_clauses`` with fixed seeds, edits some instances, and returns an ``IrregularPool``:
the (N, C, K) int32 literal array, a short name per instance, and S samples (``inst`` (S,) int32,
``x`` (S, V) uint8).  Every instance is sampled at least once and one instance twice; an instance with
isolated variables (in no clause) is sampled twice, the isolated variables all 0 in the first sample
and all 1 in the second.

What the pools hold that the generator's do not: literal 0 slots, a variable twice in a clause with the
same sign (the adjacency counts 2) and with both signs, an all-zero clause, clauses 2 and 1 wide,
variables in no clause, and an agent with no related clause and no neighbour (a graph of var rows only,
between two ordinary graphs of the batch).  The wide pools (wide257, wide300, wide513k2, wide600) hold the same
quirks on variables and clause rows past index 255, a variable in more than 64 clauses, and more variables than
the 256 lanes of the cold kernels' one workgroup per instance.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

# literal 0 = the reference's null literal (network: no edge; env: always false)
QUIRK_ROWS_3 = [[1, 1, -2], [3, -3, 4], [0, 5, -6], [0, 0, 7], [0, 0, 0], [9, 9, 9], [-9, 0, -9]]
QUIRK_ROWS_2 = [[2, 2], [5, -5], [0, 7], [-3, 0]]


@dataclass
class IrregularPool:
    name: str
    V: int
    C: int
    K: int
    vpa: int  # vars_per_agent
    pool: np.ndarray  # (N, C, K) int32
    names: List[str]  # one per instance
    inst: np.ndarray  # (S,) int32
    x: np.ndarray  # (S, V) uint8


def isolated_vars(clauses: np.ndarray, V: int) -> np.ndarray:
    """0-based variables in no clause of the (C, K) literal array (literal 0 names no variable)."""
    lits = np.abs(np.asarray(clauses)).ravel()
    return np.nonzero(np.bincount(lits[lits > 0] - 1, minlength=V) == 0)[0]


def _clauses(V, C, K, seed):
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses

    return generate_sat_clauses(V, C, K, seed=seed)


def _samples(pool: np.ndarray, V: int, seed: int):
    """inst, x as the module docstring says: each instance once, then again every instance with isolated
    variables (or instance N - 1 if there is none, so that one instance is always repeated)."""
    N = pool.shape[0]
    iso = [isolated_vars(pool[n], V) for n in range(N)]
    again = [n for n in range(N) if len(iso[n])] or [N - 1]
    inst = np.array(list(range(N)) + again, np.int32)
    assert len(inst) <= 6
    x = np.random.default_rng(seed).integers(0, 2, (len(inst), V)).astype(np.uint8)
    for s, n in enumerate(inst):
        x[s, iso[n]] = 0 if s < N else 1
    return inst, x


def quirks23() -> IrregularPool:
    """V = 23, C = 40, K = 3, vars_per_agent = 10: agents of 8, 8 and 7 variables (a padded slot)."""
    V, C = 23, 40
    pool = np.stack([_clauses(V, C, 3, 2300 + n) for n in range(4)])
    pool[1, :len(QUIRK_ROWS_3)] = QUIRK_ROWS_3
    # variable 23 (the last agent's last own variable) -> 22 everywhere, sign kept: 23 is in no clause
    p2 = pool[2]
    pool[2] = np.where(np.abs(p2) == 23, np.sign(p2) * 22, p2)
    # every literal on agent 1's variables 9..16 moved onto a variable of agent 0 (1..8) or 2 (17..23), sign kept
    p3 = pool[3]
    rows = np.arange(C)[:, None]
    moved = np.where(rows % 2 == 0, np.abs(p3) - 8, np.minimum(np.abs(p3) + 8, 23))
    pool[3] = np.where((np.abs(p3) >= 9) & (np.abs(p3) <= 16), np.sign(p3) * moved, p3)
    assert not len(isolated_vars(pool[0], V)) and not len(isolated_vars(pool[1], V))
    assert isolated_vars(pool[2], V).tolist() == [22]
    assert isolated_vars(pool[3], V).tolist() == list(range(8, 16))
    inst, x = _samples(pool, V, 23)
    return IrregularPool("quirks23", V, C, 3, 10, pool.astype(np.int32),
                         ["plain", "quirk-rows", "isolated-own-var", "empty-agent"], inst, x)


def k2(C: int = 20, N: int = 2, seed: int = 1200, allow_isolated: bool = True) -> IrregularPool:
    """V = 12, K = 2, vars_per_agent = 4: a 2-wide pool; the odd instances get [v, v], [v, -v] and literal 0
    rows.  allow_isolated=False passes over the seeds that leave a variable in no clause.  Pools of more than three
    instances carry no samples (the learners draw their own)."""
    V = 12
    out, names = [], []
    while len(out) < N:
        cl = _clauses(V, C, 2, seed)
        seed += 1
        if len(out) % 2:
            cl[:len(QUIRK_ROWS_2)] = QUIRK_ROWS_2
        if not allow_isolated and len(isolated_vars(cl, V)):
            continue
        names.append("quirk-rows" if len(out) % 2 else "plain")
        out.append(cl)
    pool = np.stack(out).astype(np.int32)
    inst, x = _samples(pool, V, 12) if N <= 3 else (np.zeros(0, np.int32), np.zeros((0, V), np.uint8))
    return IrregularPool(f"k2-C{C}", V, C, 2, 4, pool, names, inst, x)


def k1() -> IrregularPool:
    """V = 6, C = 6, K = 1, vars_per_agent = 3: unit clauses only, so no agent has a neighbour."""
    V, C = 6, 6
    pool = _clauses(V, C, 1, 600)[None].astype(np.int32)
    inst, x = _samples(pool, V, 6)
    return IrregularPool("k1", V, C, 1, 3, pool, ["unit-clauses"], inst, x)


def solo() -> IrregularPool:
    """V = 10, C = 24, K = 3, vars_per_agent = 10: one agent, so its graph never has neighbour rows."""
    V, C = 10, 24
    pool = np.stack([_clauses(V, C, 3, 1000 + n) for n in range(2)])
    pool[1, :len(QUIRK_ROWS_3)] = QUIRK_ROWS_3
    inst, x = _samples(pool, V, 10)
    return IrregularPool("solo", V, C, 3, 10, pool.astype(np.int32), ["plain", "quirk-rows"], inst, x)


def learner_pool() -> IrregularPool:
    """The learners' pool: k2 widened to C = 40, six instances, every variable in some clause.  The learners start
    from the flax zero biases, where a variable in no clause is a constant row through every LayerNorm
    (the reference's own gradient blows up there), so isolated variables stay out of it."""
    p = k2(C=40, N=6, seed=1240, allow_isolated=False)
    assert all(not len(isolated_vars(cl, p.V)) for cl in p.pool)
    return p


# ---- wide pools: more variables than one 256-thread workgroup has lanes, quirks planted past index 255
WIDE_HOT = 70  # clauses that hold the hot variable: more than 64, one wave's worth of occurrences
WIDE_ROW0 = 256  # first clause row of the quirk rows


def wide_quirk_rows(V: int, K: int) -> List[List[int]]:
    """The quirk rows of a wide pool on its top variables (1-based V, V - 1, V - 2; 0-based V - 1 >= 256): a
    literal 0 among real literals, an all-zero clause, a variable twice with both signs, twice with one sign."""
    T, T2, T3 = V, V - 1, V - 2
    if K == 3:
        return [[T, 0, -3], [0, 0, 0], [T, -T, T2], [0, 0, -T], [T2, T2, -T3]]
    assert K == 2
    return [[0, T], [0, 0], [T, -T], [-T2, 0], [T2, T2]]


def _wide(name: str, V: int, C: int, K: int, vpa: int, seed: int) -> IrregularPool:
    """Two instances.  "quirk-rows": wide_quirk_rows at clause rows 256.., variable V in the first slot of the
    first WIDE_HOT clauses (signs alternating), and, where V >= 300, 0-based variable V - 6 moved onto V - 7 so
    that it is in no clause.  "low-vars": literals on the variables below the last agent's first only, so the last
    agent has no related clause and every variable from there on (all those past 455 or 559 in the two largest
    pools, 0-based 256 in the others) is in no clause."""
    A = -(-V // vpa)
    base, rem = divmod(V, A)
    last_lo = (A - 1) * base + min(A - 1, rem)  # 0-based first own variable of the last agent
    assert C >= WIDE_ROW0 + 5 and V > 256
    q = _clauses(V, C, K, seed)
    q[np.arange(WIDE_HOT), 0] = np.where(np.arange(WIDE_HOT) % 2 == 0, V, -V)
    if V >= 300:
        iso = V - 5  # 1-based; 0-based V - 6 >= 256
        q = np.where(np.abs(q) == iso, np.sign(q) * (iso - 1), q)
    rows = wide_quirk_rows(V, K)
    q[WIDE_ROW0:WIDE_ROW0 + len(rows)] = rows
    low = _clauses(last_lo, C, K, seed + 1)
    pool = np.stack([q, low]).astype(np.int32)
    if V >= 300:
        assert V - 6 in isolated_vars(pool[0], V).tolist()
    assert isolated_vars(pool[1], V).tolist()[-(V - last_lo):] == list(range(last_lo, V))
    assert (np.abs(pool[0]) == V).any(1).sum() > 64
    inst, x = _samples(pool, V, V)
    return IrregularPool(name, V, C, K, vpa, pool, ["quirk-rows", "low-vars"], inst, x)


def wide257() -> IrregularPool:
    """V = 257, C = 300, K = 3, vars_per_agent = 8: 33 agents (26 of 8 variables, 7 of 7); one variable past the
    workgroup, C no multiple of 32.  The last agent owns 250..256, so no agent lies wholly past 255."""
    return _wide("wide257", 257, 300, 3, 8, 25700)


def wide300() -> IrregularPool:
    """V = 300, C = 400, K = 3, vars_per_agent = 60: 5 agents; 4096 < A * D = 5000 < 16384 (the env steps it with
    256 lanes, fewer than V).  The last agent owns 240..299."""
    return _wide("wide300", 300, 400, 3, 60, 30000)


def wide513k2() -> IrregularPool:
    """V = 513, C = 704, K = 2, vars_per_agent = 64: 9 agents of 57, 2-wide clauses, C a multiple of 64, three
    trips of a 256-lane loop over V.  The last agent owns 456..512, all past 255."""
    return _wide("wide513k2", 513, 704, 2, 64, 51300)


def wide600() -> IrregularPool:
    """V = 600, C = 1800, K = 3, vars_per_agent = 40: 15 agents; A * D = 45000 >= 16384 (the env steps it with 512
    lanes, fewer than V).  The last agent owns 560..599, all past 255."""
    return _wide("wide600", 600, 1800, 3, 40, 60000)


WIDE = ["wide257", "wide300", "wide513k2", "wide600"]
BUILDERS = {"quirks23": quirks23, "k2": k2, "k1": k1, "solo": solo, "wide257": wide257, "wide300": wide300,
            "wide513k2": wide513k2, "wide600": wide600}
_CACHE = {}


def get(name: str) -> IrregularPool:
    """The named pool, built once per process (callers must not write into it)."""
    if name not in _CACHE:
        _CACHE[name] = learner_pool() if name == "learner" else BUILDERS[name]()
    return _CACHE[name]
