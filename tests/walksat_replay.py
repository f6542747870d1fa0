"""Host replay of msat_walksat (include/marlsat.h): a plain NumPy restatement of the algorithm on the int32
clause array, the yardstick of tests/test_walksat_*.py.  It shares no code with the library: clause truth is
written out here, the draws come from oracle.rng, and break counts are brute force (flip, recount, unflip).
"""
import numpy as np

from oracle.rng import philox4x32_10, reset_draws

_CHUNK = 256  # flip draws are made this many steps at a time


def clause_status(x, clauses):
    """(C,) bool: clause c of the (C, K) int32 literal array is satisfied by the 0/1 assignment x (V,).
    A literal l > 0 is true iff x[l-1] == 1, l < 0 iff x[-l-1] == 0, l == 0 never."""
    var = np.maximum(np.abs(clauses) - 1, 0)
    val = x[var].astype(np.int64)
    return (((clauses > 0) & (val == 1)) | ((clauses < 0) & (val == 0))).any(axis=1)


def noise_p32(noise):
    return min(int(noise * 2 ** 32), 2 ** 32 - 1)


class _Draws:
    """q(t) = philox4x32_10((counter lo, counter hi, s, 0x80000000 + t), seed lo, seed hi), words 0..2."""

    def __init__(self, seed, counter, s):
        self.k = (np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
        self.c = (np.uint32(counter & 0xFFFFFFFF), np.uint32((counter >> 32) & 0xFFFFFFFF))
        self.s = np.uint32(s)
        self.base, self.q = -1, None

    def __call__(self, t):
        if t // _CHUNK != self.base:
            self.base = t // _CHUNK
            c3 = ((0x80000000 + self.base * _CHUNK + np.arange(_CHUNK, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)
            self.q = philox4x32_10(self.c[0], self.c[1], self.s, c3, self.k[0], self.k[1])
        i = t % _CHUNK
        return int(self.q[0][i]), int(self.q[1][i]), int(self.q[2][i])


def replay_one(clauses, x0, s, max_flips, noise32, seed, counter):
    """One sample: (x (V,) uint8, solved, flips, num_unsat)."""
    clauses = np.asarray(clauses, dtype=np.int32)
    x = (np.asarray(x0).astype(np.uint8) & 1).copy()
    draws = _Draws(seed, counter, s)
    t = 0
    while True:
        sat = clause_status(x, clauses)
        unsat = np.flatnonzero(~sat)
        n = len(unsat)
        if n == 0:
            return x, 1, t, 0
        if t == max_flips:
            return x, 0, t, n
        q0, q1, q2 = draws(t)
        c = unsat[(q0 * n) >> 32]
        cand = [abs(int(l)) - 1 for l in clauses[c] if l != 0]  # the real slots, in slot order
        m = len(cand)
        if m > 0:
            breaks = []
            for v in cand:
                x[v] ^= 1
                breaks.append(int((sat & ~clause_status(x, clauses)).sum()))
                x[v] ^= 1
            b = min(breaks)
            j = breaks.index(b) if (b == 0 or q1 >= noise32) else (q2 * m) >> 32
            x[cand[j]] ^= 1
        t += 1


def replay(clauses, num_vars, problem_idx, max_flips, noise32, seed, counter, init_assign=None):
    """The four outputs of msat_walksat for the pool `clauses` (N, C, K) int32: assign (S, V) uint8,
    solved (S,) uint8, flips (S,) int32, num_unsat (S,) int32."""
    clauses = np.asarray(clauses, dtype=np.int32)
    N = clauses.shape[0]
    pidx = np.clip(np.asarray(problem_idx, dtype=np.int64), 0, N - 1)
    S = len(pidx)
    start = reset_draws(seed, counter, S, num_vars, N)[1] if init_assign is None else np.asarray(init_assign)
    out_x = np.zeros((S, num_vars), dtype=np.uint8)
    solved = np.zeros(S, dtype=np.uint8)
    flips = np.zeros(S, dtype=np.int32)
    nun = np.zeros(S, dtype=np.int32)
    for s in range(S):
        out_x[s], solved[s], flips[s], nun[s] = replay_one(clauses[pidx[s]], start[s], s, max_flips, noise32, seed,
                                                           counter)
    return out_x, solved, flips, nun
