"""The sparse delta observation write's index arithmetic on the host (no GPU).

marl-sat_amd/csrc/obs_sparse.h holds the functions the env kernel's sparse path runs: the element evaluator
(obs_elem), the (agent, source word) task that turns a source diff into dirty chunks (sparse_task) and the list
entry of a chunk (sparse_entry).  tests/obs_sparse_check.cpp, a stand-alone program built with the host compiler
under ASan + UBSan (Makefile target obs_sparse_check), sweeps them over V in {1, 3, 31, 32, 33, 64} x C in
{1, 31, 32, 33, 70} x vars_per_agent in {1, 3, 8, V} x every element offset of both obs dtypes x old / new states
from "nothing changed" to "just under a quarter of V + C changed", against a brute-force get_obs: element values,
the dirty-chunk set (equal to differencing two brute-force images) and every chunk's values.
"""
import os
import subprocess

from conftest import ROOT


def test_sparse_chunk_derivation_matches_brute_force(tmp_path):
    pkg = os.path.join(ROOT, "marl-sat_amd")
    # built out of tree from the current sources, so a stale binary can never pass for them
    b = subprocess.run(["make", "-C", pkg, "obs_sparse_check", f"OBJDIR={tmp_path}"], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "asan", "obs_sparse_check")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "obs_sparse_check: ok" in r.stdout, r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
