"""The env step with an obs shadow, int32 observations and 16-byte groups on every path of one launch -- sparse steps,
resets in the step's workgroup and in reset workgroups, first writes, rows naming another instance, steps past the
quarter rule -- bitwise against the NumPy oracle: observations, outputs and state.  These kernels prefetch no rel word
(env_kernels.hip, PfDepth): every full write stages the whole table from the pool.  Each case runs in a child process
(tests/env_wave_step_worker.py, which lists what each group holds): the width override and the library are read once
per process.

  * at the delta rule's own width (no override) and at forced 64 and 256 lanes: small batches (B = 1, 3, 5, 8), the
    paths of one launch (reset workgroups, in-workgroup resets, a solved env, running envs; a whole-batch timeout with
    B > rq_cap), the shapes that break a wrong index (V20 C91, D % 4 != 0 with misaligned blocks, rem > 0 with
    literal-0 clauses, A = 1, a shape past every prefetch depth, a first step into a fresh tensor, rows naming
    another instance, invalidate_obs) and the reward / action modes;
  * the paths group on the debug library (bounds checks, the read-back of every unchanged element).
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "env_wave_step_worker.py")
GROUPS = ("small_batches", "paths", "shapes", "modes")
DROP = ("MARLSAT_ENV_THREADS", "MARLSAT_OBS_DELTA", "MARLSAT_LIB")


def _child(args, env):
    e = {k: v for k, v in os.environ.items() if k not in DROP}
    e.update(env)
    r = subprocess.run([sys.executable, WORKER] + args, capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("group", GROUPS)
def test_natural_width_matches_oracle(group):
    assert f"wave step {group} threads 0 ok" in _child(["--group", group], {})


@pytest.mark.parametrize("T", [64, 256])
@pytest.mark.parametrize("group", GROUPS)
def test_forced_width_matches_oracle(group, T):
    out = _child(["--group", group, "--threads", str(T)], {"MARLSAT_ENV_THREADS": str(T)})
    assert f"wave step {group} threads {T} ok" in out


def test_paths_on_the_debug_library():
    lib = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    assert os.path.exists(lib), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    out = _child(["--group", "paths", "--debug"], {"MARLSAT_LIB": lib})
    assert "wave step paths threads 0 ok" in out and "libmarlsat_debug.so" in out
