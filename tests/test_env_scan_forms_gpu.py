"""The clause scan and the scatter of the env step, over the clause forms and launch shapes at which a literal read
can go wrong.  Round 12 retires every load of a running step at one point (retire_loads, behind the flips' barrier of
the kernels with an obs shadow) so that no register waits for the wave's own stores; branch-free literal reads (a
slice's three assignment words and a changed clause's three owners read together at a clamped index, NULL / ABSENT
codes and lanes past C masked afterwards) were built, measured and not kept (marl-sat_amd/csrc/env_kernels.hip;
DESIGN.md sections 4 and 10, profiles/archive_r12).  These tests hold for either form.

What an unclamped or unmasked read gets wrong is a value, so every check is bitwise against the NumPy oracle over
short auto-reset rollouts: assignment, clause status, clause_ntrue, unsatisfied count, reward / done / solved and the
whole obs block.  The checks are in tests/env_scan_forms_worker.py, run as a child process per group (the forced
width, the forced delta write and the library are read once per process):

  edges    C on both sides of a 64-clause slice and of the prefetch's 4 x T clauses, at forced 64 / 256 / 512 lanes
  forms    tests/irregular_pools.py: literal 0, a variable twice in a clause, 2- and 1-wide clauses, variables in no
           clause, agents of unequal size with a literal 0 (rem > 0)
  paths    PBRS, the single-agent delta reward and its state-only step, timed-out envs with the reset queue on,
           a solved env, obs only, a grouped launch of two small classes
  scatter  the forced delta, int32 and int8: steps past the quarter rule between sparse ones, steps that store nothing
  debug    one case per group on libmarlsat_debug.so (its bounds checks and read-back)
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "env_scan_forms_worker.py")


def _child(args, env):
    r = subprocess.run([sys.executable, WORKER] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MARLSAT_OBS_DELTA="2", **env))
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("T", [64, 256, 512])
def test_slice_and_prefetch_edges_at_forced_width(T):
    out = _child(["--group", "edges", "--threads", str(T)], {"MARLSAT_ENV_THREADS": str(T)})
    assert "scan forms edges ok" in out


@pytest.mark.parametrize("group", ["forms", "paths", "scatter"])
def test_scan_forms(group):
    assert f"scan forms {group} ok" in _child(["--group", group], {})


def test_scan_forms_on_the_debug_library():
    lib = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    assert os.path.exists(lib), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    out = _child(["--group", "debug"], {"MARLSAT_LIB": lib})
    assert "scan forms debug ok" in out and "libmarlsat_debug.so" in out
