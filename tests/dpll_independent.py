"""An independent complete SAT decision procedure on the int32 (C, K) clause array: the ground truth the UNSAT
verdicts of msat_dpll and of tests/dpll_replay.py are held against past brute force's 14 variables.

It shares no code and no search shape with the replay or with include/marlsat.h.  The clauses are first rewritten
by meaning (literal 0 dropped, a literal kept once per clause, tautologies and repeated clauses removed).  The
search is a depth-first walk over copies of a signed assignment vector (+1 true, -1 false, 0 free): there is no
level array, no decision stack of phases and nothing is ever unassigned; a branch that fails is dropped and its
sibling's copy is taken up.  Propagation is a vectorised NumPy pass that assigns every unit it sees and lets the
next pass find the clause two opposite units falsify.  Two branching rules, neither the header's:

  "short": the first literal of the first shortest open clause, tried true first;
  "occur": the free variable in the most open clauses (unweighted), the highest index on ties, tried false first.

`decide` checks every model it returns with dpll_cases.satisfied on the clauses as given.
"""
import numpy as np

SAT, UNSAT = 1, 2
RULES = ("short", "occur")


def normalise(clauses):
    """The clause set by meaning: (M, K) int32 rows of distinct literals, padded with 0 on the right, no
    tautology, no row twice.  An empty clause (a row of zeros) is kept: it makes the set unsatisfiable."""
    rows = set()
    for cl in np.asarray(clauses).tolist():
        lits = sorted({l for l in cl if l != 0}, key=lambda l: (abs(l), l))
        if any(-l in lits for l in lits):
            continue
        rows.add(tuple(lits))
    K = max(1, np.asarray(clauses).shape[1])
    out = np.zeros((len(rows), K), dtype=np.int32)
    for i, lits in enumerate(sorted(rows, key=lambda r: (len(r), r))):
        out[i, :len(lits)] = lits
    return out


def _propagate(a, var, sgn):
    """Unit propagation on the signed assignment `a` (changed in place).  False on a falsified clause, else
    (value of every slot, open-clause mask, free slots per clause) at the fixpoint."""
    while True:
        val = sgn * a[var]  # +1 true, -1 false, 0 free; a null slot has sgn 0 ...
        val[sgn == 0] = -1  # ... and is false
        open_ = ~(val == 1).any(axis=1)
        free = (val == 0).sum(axis=1)
        if (open_ & (free == 0)).any():
            return False
        unit = np.flatnonzero(open_ & (free == 1))
        if unit.size == 0:
            return val, open_, free
        slot = (val[unit] == 0).argmax(axis=1)
        a[var[unit, slot]] = sgn[unit, slot]  # opposite units: one wins, the other's clause is false next pass


def _branch(rule, a, var, sgn, val, open_, free):
    """(variable, first sign) of the next split; there is an open clause, and each has two or more free slots."""
    if rule == "short":
        width = np.where(open_, free, np.iinfo(np.int64).max)
        c = int(width.argmin())
        j = int((val[c] == 0).argmax())
        return int(var[c, j]), int(sgn[c, j])
    assert rule == "occur"
    hits = np.bincount(var[open_][val[open_] == 0], minlength=len(a))
    v = len(a) - 1 - int(hits[::-1].argmax())
    return v, -1


def solve(clauses, num_vars, rule="short"):
    """(SAT, x (V,) uint8, tree nodes) or (UNSAT, None, tree nodes) for the (C, K) int32 clause array."""
    cl = normalise(clauses)
    V = int(num_vars)
    nodes = 0
    if cl.shape[0] == 0:
        return SAT, np.zeros(V, dtype=np.uint8), nodes
    var = np.maximum(np.abs(cl) - 1, 0).astype(np.int64)
    sgn = np.sign(cl).astype(np.int8)
    todo = [np.zeros(V, dtype=np.int8)]
    while todo:
        a = todo.pop()
        nodes += 1
        fix = _propagate(a, var, sgn)
        if fix is False:
            continue
        val, open_, free = fix
        if not open_.any():
            return SAT, (a == 1).astype(np.uint8), nodes
        v, first = _branch(rule, a, var, sgn, val, open_, free)
        other = a.copy()
        other[v] = -first
        a[v] = first
        todo.append(other)
        todo.append(a)  # taken up next
    return UNSAT, None, nodes


def decide(clauses, num_vars, rule="short"):
    """solve() with the model checked on the clauses as given: (status, x or None)."""
    from dpll_cases import satisfied

    status, x, _ = solve(clauses, num_vars, rule)
    if status == SAT:
        assert x.shape == (num_vars,) and satisfied(x, np.asarray(clauses)).all(), "the independent model fails"
    return status, x


def verdicts(pool, num_vars, rule="short"):
    """(N,) uint8 of SAT / UNSAT over the pool (N, C, K)."""
    return np.array([decide(cl, num_vars, rule)[0] for cl in np.asarray(pool)], dtype=np.uint8)
