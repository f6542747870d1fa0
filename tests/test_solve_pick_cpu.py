"""The policy solver's order on search records on the host (no GPU).

marl-sat_amd/csrc/solve_pick.h holds pick_before, the comparison msat_solve_pick's kernel reduces an instance's
tries with (a solved try first; solved: fewest steps, then fewest flips, then lowest try; unsolved: least
best_unsat, then least best_step, then lowest try).  tests/solve_pick_check.cpp, a stand-alone program built with
the host compiler under ASan + UBSan (Makefile target solve_pick_check), sweeps it over all records of a small
domain: a strict total order (irreflexive, antisymmetric, total on distinct tries, transitive), equal to the
stated lexicographic key, and the kernel's sentinel-and-replace fold picks the first element of a brute-force
sort in every visiting order.
"""
import os
import subprocess

from conftest import ROOT


def test_pick_order_is_total_and_matches_brute_force_sort(tmp_path):
    pkg = os.path.join(ROOT, "marl-sat_amd")
    # built out of tree from the current sources, so a stale binary can never pass for them
    b = subprocess.run(["make", "-C", pkg, "solve_pick_check", f"OBJDIR={tmp_path}"], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "asan", "solve_pick_check")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "solve_pick_check: ok" in r.stdout, r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
