"""Instances and ground truth shared by the tests/test_dpll_*.py modules: seeded pools, the hand-made edge cases,
brute-force satisfiability and a clause check that share nothing with tests/dpll_replay.py, the pools whose verdicts
are held against tests/dpll_independent.py with their meaning-preserving rewrites, and the hand-derived chain
instances that search past level 255.  Replays and independent verdicts are computed once per session and shared
(never modified)."""
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


# ------------------------------------------------------------------ verdict soundness ----
# The pools whose verdicts are held against tests/dpll_independent.py (random_pool arguments).  The independent
# solver found 8 SAT / 8 UNSAT, 17 / 15 and 4 / 2.
SOUND = {"uf20": (20, 91, 16, 31), "uf50": (50, 218, 32, 11), "uf100": (100, 430, 6, 12)}


def sound_pool(name):
    """(pool (N, C, 3), V, N), built once per session."""
    V, C, N, seed = SOUND[name]
    if ("pool", name) not in _REFS:
        _REFS["pool", name] = random_pool(V, C, N, seed)
    return _REFS["pool", name], V, N


def shared_verdicts(name, rule="short"):
    """The independent solver's verdicts (N,) uint8 on a SOUND pool under one branching rule, once per session."""
    from dpll_independent import verdicts

    if ("verdict", name, rule) not in _REFS:
        pool, V, _ = sound_pool(name)
        _REFS["verdict", name, rule] = verdicts(pool, V, rule)
    return _REFS["verdict", name, rule]


def sound_verdicts(name):
    """The ground truth of a SOUND pool, from the independent solver alone: its two branching rules agree on every
    instance and the pool holds at least two instances of either verdict."""
    from dpll_independent import RULES

    truth = shared_verdicts(name, RULES[0])
    for rule in RULES[1:]:
        assert np.array_equal(truth, shared_verdicts(name, rule)), (name, rule)
    assert (truth == 1).sum() >= 2 and (truth == 2).sum() >= 2, (name, truth)
    return truth


def rewrites(pool, V, seed):
    """Four rewrites of every instance of `pool` (N, C, K) that keep satisfiability and change the search:
    name -> (pool', flip), flip (N, V) bool being the variables whose polarity was flipped (None: none were)."""
    rng = np.random.default_rng(seed)
    pool = np.asarray(pool, dtype=np.int32)
    N, C, K = pool.shape
    out = {}
    # a random renaming of the variables
    ren = np.empty_like(pool)
    for n in range(N):
        to = np.concatenate([[0], rng.permutation(V) + 1])
        ren[n] = np.sign(pool[n]) * to[np.abs(pool[n])]
    out["renamed"] = (ren, None)
    # the polarity of a random half of the variables flipped in every clause
    flip = np.zeros((N, V), dtype=bool)
    pol = np.empty_like(pool)
    for n in range(N):
        flip[n, rng.permutation(V)[:V // 2]] = True
        sign = np.concatenate([[1], np.where(flip[n], -1, 1)])
        pol[n] = pool[n] * sign[np.abs(pool[n])]
    out["polarity"] = (pol, flip)
    # the clause rows permuted, the slots of each row permuted
    perm = np.empty_like(pool)
    for n in range(N):
        rows = pool[n][rng.permutation(C)]
        perm[n] = np.stack([r[rng.permutation(K)] for r in rows])
    out["permuted"] = (perm, None)
    # ten clauses twice; in the copies a literal-0 slot, where there is one, repeats a literal of its clause
    dup = np.empty((N, C + 10, K), dtype=np.int32)
    for n in range(N):
        extra = pool[n][rng.choice(C, size=10, replace=False)].copy()
        for row in extra:
            real, null = np.flatnonzero(row != 0), np.flatnonzero(row == 0)
            if len(real) and len(null):
                row[null[0]] = row[rng.choice(real)]
        dup[n] = np.concatenate([pool[n], extra])[rng.permutation(C + 10)]
    out["duplicated"] = (dup, None)
    return out


# ------------------------------------------------------------------ levels past 255 ----
def chain(pairs=300):
    """(clauses (1, C, 3), V): pairs - 1 binary clauses [2i+1, 2i+2, 0], each twice, then with p, q, r the next
    three variables [p, q, 0], [-p, r, r], [-p, -r, -r].  By the header: each open pair scores 8 on both of its
    variables, p scores 4 + 2, q and r 4, so the first pairs - 1 decisions take the odd variables in order with
    phase 1 (count 8 against 0); level `pairs` decides p = 1 (4 against 2); the two trap clauses are the units r and
    -r of one pass; the open entry at level `pairs` flips, p = 0 makes q a unit, and the model is complete."""
    cl = []
    for i in range(pairs - 1):
        cl += [[2 * i + 1, 2 * i + 2, 0]] * 2
    p, q, r = 2 * pairs - 1, 2 * pairs, 2 * pairs + 1
    cl += [[p, q, 0], [-p, r, r], [-p, -r, -r]]
    return np.asarray([cl], dtype=np.int32), r


def chain_two_pops(pairs=298):
    """(clauses (1, C, 3), V): the chain's family with a conflict at level pairs + 2 that pops that level and flips
    the one below.  `pairs` binary clauses [2i+1, 2i+2, 0], four times each (16 per variable, so they go first and
    in order), then with a, a2, b, c, d the next five variables [a, a2, 0] twice and [-a, b, c], [-a, b, -c],
    [-a, -b, d], [-a, -b, -d].  By the header: after the pairs a scores 8 + 4 (a2 8, b 4, c and d 2) and is
    decided 1 at level pairs + 1 (8 against 4); nothing is unit; the four clauses are now binary, b scores 16 (c
    and d 8) and is decided 1 at level pairs + 2 (8 against 8); d and -d are units of one pass: conflict 1 flips
    the entry at pairs + 2 closed; b = 0 makes c and -c units of one pass: conflict 2 pops the closed entry and
    flips a at level pairs + 1; a = 0 makes a2 a unit, every clause is true: SAT, nodes pairs + 4, conflicts 2,
    propagations 1, the odd variables of the pairs and a2 set."""
    cl = []
    for i in range(pairs):
        cl += [[2 * i + 1, 2 * i + 2, 0]] * 4
    a, a2, b, c, d = (2 * pairs + k for k in range(1, 6))
    cl += [[a, a2, 0]] * 2 + [[-a, b, c], [-a, b, -c], [-a, -b, d], [-a, -b, -d]]
    return np.asarray([cl], dtype=np.int32), d
