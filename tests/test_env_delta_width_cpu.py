"""Host-only checks of the width rule of the launches with an obs shadow (msat_env_step_delta):
msat_env_delta_launch_threads against the rule restated in tests/env_delta_width_worker.py (delta_lanes), beside
msat_env_launch_threads, which stays the full-write launches' rule and the bench's kernel label.  No GPU call."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT
import env_delta_width_worker as W

WORKER = os.path.join(ROOT, "tests", "env_delta_width_worker.py")


def _forced():
    v = os.environ.get("MARLSAT_ENV_THREADS", "")
    return int(v) if v.isdigit() and int(v) in (64, 128, 256, 512) else 0


def test_delta_rule_over_the_shape_grid():
    """The grid of tests/test_capi.py (A * D = 4096 | 4097, 16383 | 16384, uf200 with 10 and 25 agents), int32 and
    int8, B on both sides of every threshold of the plain rule and of 2048 and 4096 (the delta rule has no B threshold
    of its own: 256 lanes at every B from A * D = 16384 on, int32 only)."""
    assert {A * (2 * V + C) for V, C, A in W.GRID} >= {4096, 4097, 16383, 16384}
    assert (200, 860, 10) in W.GRID and (200, 860, 25) in W.GRID
    forced = _forced()
    seen = W.host_widths(forced)
    if not forced:
        # the delta rule departs from the plain one exactly where it is meant to, and nowhere else
        assert (256, 512) in seen
        assert {(d, p) for d, p in seen if d != p} == {(256, 512)}
        assert W.delta_lanes(25, 1260, 4096) == 256 and W.plain_lanes(25, 1260, 4096) == 512
        assert W.delta_lanes(25, 1260, 4096, int8=True) == 512
        assert W.delta_lanes(43, 381, 8) == W.plain_lanes(43, 381, 8) == 256  # A * D = 16383


@pytest.mark.parametrize("T", [64, 128, 256, 512])
def test_forced_width_wins_over_both_rules(T):
    """MARLSAT_ENV_THREADS=T (read once per process, hence the child): both exports report T for every desc."""
    r = subprocess.run([sys.executable, WORKER, "--host", str(T)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, MARLSAT_ENV_THREADS=str(T)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"delta width host forced {T} ok" in r.stdout


def test_carried_task_index_matches_division(tmp_path):
    """tests/task_index_check.cpp (host compiler, ASan + UBSan, its own main): the sparse task loop's carried
    (agent, source word) pair of csrc/obs_sparse.h against t / U, t % U for T in {64, 128, 256, 512}, U in [3, 200],
    A in [1, 65], every lane and pass; U > T, U dividing T, A U < T and A U a multiple of T are all met."""
    pkg = os.path.join(ROOT, "marl-sat_amd")
    # built out of tree from the current sources, so a stale binary can never pass for them
    b = subprocess.run(["make", "-C", pkg, "task_index_check", f"OBJDIR={tmp_path}"], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "asan", "task_index_check")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "task_index_check: ok" in r.stdout, r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_bad_descriptor_is_refused_with_a_text():
    from marlsat import _lib

    bad = W.desc(20, 91, 2, 4)
    bad.num_vars = 0
    assert _lib.lib.msat_env_delta_launch_threads(ctypes.byref(bad)) == -1
    assert "num_vars" in _lib.lib.msat_last_error().decode()
    bad = W.desc(20, 91, 2, 4)
    bad.obs_dtype = 3
    assert _lib.lib.msat_env_delta_launch_threads(ctypes.byref(bad)) == -1
    assert "obs_dtype" in _lib.lib.msat_last_error().decode()
