"""The device generator's draw on the host (no GPU).

marl-sat_amd/csrc/pool_gen.h holds the arithmetic pool_generate_kernel stores every word with (one Philox block per
clause and per 128 hidden bits, include/marlsat.h msat_pool_generate).  tests/pool_gen_check.cpp, a stand-alone
program built with the host compiler under ASan + UBSan (Makefile target pool_gen_check), prints the hidden bits
and clauses those functions give for (seed, counter, n, attempt, V, C, K); every word must equal
tests/pool_generate_replay.py, the NumPy restatement of the header on oracle.rng.philox4x32_10.  The properties of
the draw itself (distinct variables, the planted assignment satisfies every clause, the retry rule) are asserted on
the replay alone.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import pool_generate_replay as replay

# (V, C, K): 129 and 200 cross the 128-bit hidden block; (3, 5, 3) is V == K (every clause holds every variable);
# 257 and 600 are more variables (and 300 and 1800 more clauses) than the kernel's workgroup has lanes
SHAPES = [(20, 20, 3), (12, 20, 2), (6, 6, 1), (129, 300, 3), (3, 5, 3), (200, 860, 3), (257, 300, 3), (600, 1800, 3)]
SEED, COUNTER = 0x9E3779B97F4A7C15, (7 << 32) | 3  # both halves of the key and of the counter are in use


@pytest.fixture(scope="module")
def check_binary(tmp_path_factory):
    out = tmp_path_factory.mktemp("pool_gen_check")
    # built out of tree from the current sources, so a stale binary can never pass for them
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "marl-sat_amd"), "pool_gen_check", f"OBJDIR={out}"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return os.path.join(out, "asan", "pool_gen_check")


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([binary] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "pool_gen_check: ok" and lines[0].startswith("hidden")
    hidden = np.array(lines[0].split()[1:], dtype=np.uint8)
    clauses = np.array([l.split()[1:] for l in lines[1:-1]], dtype=np.int32)
    return clauses, hidden


@pytest.mark.parametrize("V,C,K", SHAPES)
def test_header_functions_equal_the_replay_word_for_word(check_binary, V, C, K):
    for n, attempt in ((0, 0), (5, 0), (5, 3), (1000003, 255)):
        clauses, hidden = _run(check_binary, SEED, COUNTER, n, attempt, V, C, K)
        want_cl, want_h = replay.attempt_draw(SEED, COUNTER, n, attempt, V, C, K)
        assert clauses.shape == (C, K) and hidden.shape == (V,)
        np.testing.assert_array_equal(hidden, want_h, err_msg=f"hidden bits n={n} attempt={attempt}")
        np.testing.assert_array_equal(clauses, want_cl, err_msg=f"clauses n={n} attempt={attempt}")


def test_bad_shapes_are_refused_by_the_program(check_binary):
    for args in ((1, 2, 0, 0, 2, 5, 3), (1, 2, 0, 0, 20, 5, 4), (1, 2, 0, 256, 20, 5, 3)):  # K > V, K > 3, attempt
        r = subprocess.run([check_binary] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "bad shape" in r.stderr


@pytest.mark.parametrize("V,C,K", SHAPES)
def test_replay_draws_planted_instances(V, C, K):
    """K distinct variables in [1, V] per clause; the planted assignment satisfies every clause; an accepted
    attempt leaves no variable isolated; attempts differ from one another and instances from one another."""
    N = 8
    # (6, 6, 1): six unit clauses cover six variables with probability 6!/6^6 = 1.5 %, so most rows exhaust
    # four attempts; (3, 5, 3) can never isolate a variable
    max_attempts = 4 if (V, C, K) == (6, 6, 1) else 64
    clauses, planted, attempts = replay.generate(N, V, C, K, SEED, COUNTER, True, max_attempts)
    var = np.abs(clauses)
    assert var.min() >= 1 and var.max() <= V
    srt = np.sort(var, axis=-1)
    assert (srt[..., 1:] != srt[..., :-1]).all(), "a variable twice in a clause"
    for n in range(N):
        assert replay.satisfied(clauses[n], planted[n]).all(), f"instance {n}: planted assignment fails a clause"
        if attempts[n] >= 0:
            assert not replay.has_isolated(clauses[n], V)
            want_cl, want_h = replay.attempt_draw(SEED, COUNTER, n, int(attempts[n]), V, C, K)
            for a in range(int(attempts[n])):  # every earlier attempt was rejected for an isolated variable
                assert replay.has_isolated(replay.attempt_draw(SEED, COUNTER, n, a, V, C, K)[0], V)
        else:
            assert replay.has_isolated(clauses[n], V)
            want_cl, want_h = replay.attempt_draw(SEED, COUNTER, n, max_attempts - 1, V, C, K)
        np.testing.assert_array_equal(clauses[n], want_cl)
        np.testing.assert_array_equal(planted[n], want_h)
    if (V, C, K) == (6, 6, 1):
        assert (attempts == -1).any()
    if (V, C, K) == (3, 5, 3):
        assert (attempts == 0).all()
    if V > 3:
        assert len({clauses[n].tobytes() for n in range(N)}) == N
    # rejection off: attempt 0 of every instance, whatever it isolates; a prefix of a longer call
    c0, p0, a0 = replay.generate(N, V, C, K, SEED, COUNTER, False, max_attempts)
    assert (a0 == 0).all()
    c1, p1, _ = replay.generate(3, V, C, K, SEED, COUNTER, False, max_attempts)
    np.testing.assert_array_equal(c0[:3], c1)
    np.testing.assert_array_equal(p0[:3], p1)


def test_replay_anchor_and_signs_are_spread():
    """Over many clauses the anchor visits every slot and the free signs are fair coins: the slot whose sign
    follows the hidden bit is not always the same one, and a free slot disagrees with the hidden bit about half
    the time (3,000 clauses x 2 free slots: 0.5 +- 4 sigma = 0.026)."""
    V, C, K = 50, 3000, 3
    clauses, hidden = replay.attempt_draw(SEED, COUNTER, 0, 0, V, C, K)
    agree = (clauses > 0) == hidden[np.abs(clauses) - 1].astype(bool)
    assert agree.any(axis=1).all()
    frac = (agree.sum() - C) / (2 * C)  # agreement among the two free slots, the anchor always agreeing
    assert abs(frac - 0.5) < 0.026, frac
    counts = np.bincount(np.abs(clauses).ravel() - 1, minlength=V)
    assert counts.min() > 0.6 * 3 * C / V and counts.max() < 1.4 * 3 * C / V  # 180 +- 13 per variable expected
