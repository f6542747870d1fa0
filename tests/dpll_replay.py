"""Host replay of msat_dpll (include/marlsat.h): a plain NumPy/Python restatement of the header's algorithm on the
int32 clause array, one sample at a time, written for clarity.  The yardstick of tests/test_dpll_*.py.  It shares no
code with the library.  A pass judges all clauses in one NumPy expression (every clause against the assignment of the
pass's start, as the header has it); the search around it is plain Python.

A literal l > 0 is the code 2 (l - 1), true iff x[l - 1] == 1; l < 0 is the code 2 (-l - 1) + 1, true iff
x[-l - 1] == 0; l == 0 is the null literal: always false, no real slot.
"""
import numpy as np

UNKNOWN, SAT, UNSAT = 0, 1, 2
UNSET = -1


def _judge(code, real, x):
    """Every clause against x (V,) int8: (open (C,) bool: the clause has no true slot, free (C, K) bool: its
    unassigned real slots)."""
    val = x[code >> 1]
    free = real & (val == UNSET)
    true = real & (val != UNSET) & (((val ^ code) & 1) == 1)
    return ~true.any(axis=1), free


def replay_one(clauses, num_vars, cube=0, cube_bits=0, max_nodes=0, stats=None):
    """One sample: (status, x (V,) uint8, nodes, conflicts, propagations).  A dict passed as `stats` receives what
    the search went through: "max_level" (the largest L reached), "deepest_flip" (the deepest level at which an entry
    was flipped, 0 if none), "max_pops" (the most closed entries popped by one conflict) and "flips" (per flip, in
    order: (L when the conflict arose, the level flipped)).  The outputs do not depend on it."""
    if stats is not None:
        stats.update(max_level=0, deepest_flip=0, max_pops=0, flips=[])
    V = int(num_vars)
    lits = np.asarray(clauses, dtype=np.int64)
    real = lits != 0  # the real slots; a null slot's code is never looked at
    code = np.where(real, (np.abs(lits) - 1) * 2 + (lits < 0), 0)
    rows = np.arange(code.shape[0])
    x = np.full(V, UNSET, dtype=np.int8)
    level = np.zeros(V, dtype=np.int64)
    stack = []  # entry L-1: [variable, phase, closed]
    nodes = conflicts = props = 0

    def result(status):
        out = np.zeros(V, dtype=np.uint8)
        if status == SAT:
            out[:] = x == 1
        return status, out, nodes, conflicts, props

    while True:
        # step 1: synchronous passes
        conflict = False
        for _ in range(V + 1):
            open_, free = _judge(code, real, x)  # against the assignment at the start of the pass
            k = free.sum(axis=1)
            if (open_ & (k == 0)).any():
                conflict = True
                break
            first = code[rows, free.argmax(axis=1)]  # the code of the first unassigned real slot
            same = ((code == first[:, None]) | ~free).all(axis=1)
            units = np.unique(first[open_ & (k > 0) & same])
            if units.size == 0:
                break
            unit_vars = np.unique(units >> 1)
            if len(unit_vars) < len(units):  # some variable has both signs
                conflict = True
                break
            x[units >> 1] = 1 - (units & 1)  # the code becomes true
            level[units >> 1] = len(stack)
            props += len(unit_vars)
        else:
            raise AssertionError("more than V + 1 passes")

        if conflict:  # step 2
            conflicts += 1
            before = len(stack)
            while stack and stack[-1][2]:
                stack.pop()
            L = len(stack)
            if stats is not None:
                stats["max_pops"] = max(stats["max_pops"], before - L)
            if L == 0:
                return result(UNSAT)
            x[(x != UNSET) & (level >= L)] = UNSET
            if nodes == max_nodes:
                return result(UNKNOWN)
            nodes += 1
            if stats is not None:
                stats["deepest_flip"] = max(stats["deepest_flip"], L)
                stats["flips"].append((before, L))
            v, phase, _ = stack[-1]
            stack[-1] = [v, phase ^ 1, True]
            x[v], level[v] = phase ^ 1, L
            continue

        open_, free = _judge(code, real, x)
        if not open_.any():  # step 3
            return result(SAT)

        if nodes == max_nodes:  # step 4
            return result(UNKNOWN)
        counted = free & open_[:, None]  # the unassigned real slots of the open clauses, duplicates included
        weight = np.where(free.sum(axis=1) == 2, 4, 1)
        cnt = np.zeros(2 * V, dtype=np.int64)
        np.add.at(cnt, code[counted], np.broadcast_to(weight[:, None], code.shape)[counted])
        score = np.where(x == UNSET, cnt[0::2] + cnt[1::2], -1)
        v = int(score.argmax())  # the lowest index on ties
        assert score[v] > 0
        phase = 1 if cnt[2 * v] >= cnt[2 * v + 1] else 0
        L = len(stack) + 1
        nodes += 1
        closed = L <= cube_bits
        if closed:
            phase = (int(cube) >> (L - 1)) & 1
        stack.append([v, phase, closed])
        x[v], level[v] = phase, L
        if stats is not None:
            stats["max_level"] = max(stats["max_level"], L)


def replay(clauses, num_vars, problem_idx, cubes=None, cube_bits=0, max_nodes=0):
    """The five outputs of msat_dpll for the pool `clauses` (N, C, K) int32: status (S,) uint8, assign (S, V) uint8,
    nodes, conflicts, propagations (S,) int32."""
    clauses = np.asarray(clauses, dtype=np.int32)
    N = clauses.shape[0]
    pidx = np.clip(np.asarray(problem_idx, dtype=np.int64), 0, N - 1)
    S = len(pidx)
    cubes = np.zeros(S, np.int64) if cubes is None else np.asarray(cubes, dtype=np.int64)
    status = np.zeros(S, dtype=np.uint8)
    out_x = np.zeros((S, num_vars), dtype=np.uint8)
    nodes, conflicts, props = (np.zeros(S, dtype=np.int32) for _ in range(3))
    for s in range(S):
        status[s], out_x[s], nodes[s], conflicts[s], props[s] = replay_one(clauses[pidx[s]], num_vars, cubes[s],
                                                                          cube_bits, max_nodes)
    return status, out_x, nodes, conflicts, props


def combine(statuses):
    """The cube rule: SAT iff some cube is SAT, UNSAT iff every cube is UNSAT, else UNKNOWN."""
    statuses = list(statuses)
    if any(s == SAT for s in statuses):
        return SAT
    return UNSAT if all(s == UNSAT for s in statuses) else UNKNOWN
