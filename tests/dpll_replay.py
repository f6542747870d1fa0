"""Host replay of msat_dpll (include/marlsat.h): a plain NumPy/Python restatement of the header's algorithm on the
int32 clause array, one sample at a time, written for clarity.  The yardstick of tests/test_dpll_*.py.  It shares no
code with the library.

A literal l > 0 is the code 2 (l - 1), true iff x[l - 1] == 1; l < 0 is the code 2 (-l - 1) + 1, true iff
x[-l - 1] == 0; l == 0 is the null literal: always false, no real slot.
"""
import numpy as np

UNKNOWN, SAT, UNSAT = 0, 1, 2
UNSET = -1


def _judge(clause_codes, x):
    """One clause against x: (has a true slot, the codes of its unassigned real slots in slot order)."""
    true, free = False, []
    for c in clause_codes:
        v = c >> 1
        if x[v] == UNSET:
            free.append(c)
        elif (x[v] ^ c) & 1:
            true = True
    return true, free


def replay_one(clauses, num_vars, cube=0, cube_bits=0, max_nodes=0):
    """One sample: (status, x (V,) uint8, nodes, conflicts, propagations)."""
    V = int(num_vars)
    # real slots only: the codes of every clause, in slot order
    codes = [[(abs(int(l)) - 1) * 2 + (1 if l < 0 else 0) for l in cl if l != 0] for cl in np.asarray(clauses)]
    x = [UNSET] * V
    level = [0] * V
    stack = []  # entry L-1: [variable, phase, closed]
    nodes = conflicts = props = 0

    def result(status):
        out = np.zeros(V, dtype=np.uint8)
        if status == SAT:
            out[:] = [1 if b == 1 else 0 for b in x]
        return status, out, nodes, conflicts, props

    while True:
        # step 1: synchronous passes
        conflict = False
        for _ in range(V + 1):
            judged = [_judge(c, x) for c in codes]  # against the assignment at the start of the pass
            if any(not t and not free for t, free in judged):
                conflict = True
                break
            units = sorted({free[0] for t, free in judged if not t and free and all(f == free[0] for f in free)})
            if not units:
                break
            unit_vars = {c >> 1 for c in units}
            if len(unit_vars) < len(units):  # some variable has both signs
                conflict = True
                break
            for c in units:
                x[c >> 1] = 1 - (c & 1)  # the code becomes true
                level[c >> 1] = len(stack)
            props += len(unit_vars)
        else:
            raise AssertionError("more than V + 1 passes")

        if conflict:  # step 2
            conflicts += 1
            while stack and stack[-1][2]:
                stack.pop()
            L = len(stack)
            if L == 0:
                return result(UNSAT)
            for v in range(V):
                if x[v] != UNSET and level[v] >= L:
                    x[v] = UNSET
            if nodes == max_nodes:
                return result(UNKNOWN)
            nodes += 1
            v, phase, _ = stack[-1]
            stack[-1] = [v, phase ^ 1, True]
            x[v], level[v] = phase ^ 1, L
            continue

        judged = [_judge(c, x) for c in codes]
        opens = [free for t, free in judged if not t]
        if not opens:  # step 3
            return result(SAT)

        if nodes == max_nodes:  # step 4
            return result(UNKNOWN)
        cnt = [0] * (2 * V)
        for free in opens:
            w = 4 if len(free) == 2 else 1
            for c in free:
                cnt[c] += w
        best, v = -1, -1
        for u in range(V):
            if x[u] == UNSET and cnt[2 * u] + cnt[2 * u + 1] > best:
                best, v = cnt[2 * u] + cnt[2 * u + 1], u
        assert best > 0
        phase = 1 if cnt[2 * v] >= cnt[2 * v + 1] else 0
        L = len(stack) + 1
        nodes += 1
        closed = L <= cube_bits
        if closed:
            phase = (int(cube) >> (L - 1)) & 1
        stack.append([v, phase, closed])
        x[v], level[v] = phase, L


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
