"""Host replay of msat_pool_generate (include/marlsat.h) on oracle.rng.philox4x32_10 -- test infrastructure.

A NumPy restatement of the header's draw definition, written from the header and not from csrc/pool_gen.h:
``attempt_draw`` is one attempt of one instance (hidden bits, clauses), ``generate`` adds the retry rule and
gives what the entry point gives (clauses (N,C,K) int32, planted (N,V) uint8, attempts (N,) int32).
"""
from __future__ import annotations

import numpy as np

from oracle.rng import philox4x32_10

MAX_BLOCKS = 1 << 24
MAX_ATTEMPTS = 255


def _blocks(seed: int, counter: int, n: int, attempt: int, blocks: np.ndarray) -> np.ndarray:
    """(len(blocks), 4) uint32: q(attempt, b) for every b of blocks."""
    k0, k1 = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    c0, c1 = np.uint32(counter & 0xFFFFFFFF), np.uint32((counter >> 32) & 0xFFFFFFFF)
    c3 = (np.uint32(attempt << 24) | blocks.astype(np.uint32)).astype(np.uint32)
    return np.stack(philox4x32_10(c0, c1, np.uint32(n), c3, k0, k1), axis=-1)


def attempt_draw(seed: int, counter: int, n: int, attempt: int, V: int, C: int, K: int):
    """(clauses (C,K) int32, hidden (V,) uint8) of attempt `attempt` of instance n."""
    HB = (V + 127) // 128
    hw = _blocks(seed, counter, n, attempt, np.arange(HB))  # (HB, 4)
    v = np.arange(V)
    hidden = ((hw[v >> 7, (v >> 5) & 3] >> (v & 31).astype(np.uint32)) & 1).astype(np.uint8)
    q = _blocks(seed, counter, n, attempt, HB + np.arange(C)).astype(np.uint64)  # (C, 4)
    var = np.zeros((C, K), np.int64)
    for i in range(K):
        j = V - K + i
        t = ((q[:, i] * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        held = (var[:, :i] == t[:, None]).any(axis=1)
        var[:, i] = np.where(held, j, t)
    q3 = q[:, 3].astype(np.int64)
    anchor = ((q3 & 0xFFFF) * K) >> 16
    coin = (q3[:, None] >> (16 + np.arange(K))[None, :]) & 1
    pos = np.where(np.arange(K)[None, :] == anchor[:, None], hidden[var], coin)
    return np.where(pos == 1, var + 1, -(var + 1)).astype(np.int32), hidden


def has_isolated(clauses: np.ndarray, V: int) -> bool:
    return bool((np.bincount(np.abs(clauses).ravel() - 1, minlength=V) == 0).any())


def generate(N: int, V: int, C: int, K: int, seed: int, counter: int, reject_isolated: bool = True,
             max_attempts: int = 64):
    """What msat_pool_generate writes: an attempt is accepted iff rejection is off or no variable is isolated;
    attempts[n] = the accepted attempt or -1, and the outputs then hold the last attempt."""
    assert 1 <= K <= min(V, 3) and (V + 127) // 128 + C < MAX_BLOCKS and 1 <= max_attempts <= MAX_ATTEMPTS
    clauses = np.zeros((N, C, K), np.int32)
    planted = np.zeros((N, V), np.uint8)
    attempts = np.full((N,), -1, np.int32)
    for n in range(N):
        for a in range(max_attempts if reject_isolated else 1):
            clauses[n], planted[n] = attempt_draw(seed, counter, n, a, V, C, K)
            if not reject_isolated or not has_isolated(clauses[n], V):
                attempts[n] = a
                break
    return clauses, planted, attempts


def satisfied(clauses: np.ndarray, x: np.ndarray) -> np.ndarray:
    """(C,) bool: clause truth under assignment x (V,) for one instance's signed 1-based literals."""
    val = x[np.abs(clauses) - 1].astype(bool)
    return np.where(clauses > 0, val, ~val).any(axis=1)
