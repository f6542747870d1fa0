"""The env step with an obs shadow (msat_env_step_delta) at the width its own rule picks (env_delta_threads: 256 lanes
at 8 waves per SIMD for int32 observations of A * D >= 16384, the plain rule's width elsewhere) and at every forced
width, bitwise against the NumPy oracle.  Each group runs in a child process (tests/env_delta_width_worker.py): the
overrides are read once per process.

  * natural width, no override: the export reports the rule's value, then 12-step delta rollouts with autoreset on
    and off (sparse reward, mode-0 actions) on uf200 with 25 agents at B = 16, on A * D = 16384 (16 agents) at
    B = 8 and on A * D = 16383 (43 agents, forced delta) at B = 8.  SATEnv derives the agent count from
    vars_per_agent, so the two threshold shapes are (V, C) = (96, 832) and (86, 209): the same A, the same A * D as
    the host grid's (100, 824, 16) and (100, 181, 43), which no vars_per_agent gives.  The rule has no B threshold,
    so there is no large-B case;
  * forced 64 / 128 / 256 / 512 lanes with forced delta, on shapes that break a wrong task index: fewer tasks than
    lanes (V20 C91, 2 agents), more tasks per agent row than lanes at 64 (V64 C2080: U = 69), A * U = 512 a multiple
    of every width (V96 C832, 16 agents, U = 32), obs blocks misaligned by 1-3 elements, an all-no-op step that must
    store nothing, mode-1 steps across the quarter rule in both directions, and reset workgroups, in-workgroup
    resets, a solved env and running envs in one launch;
  * the uf200 natural-width case on the debug library (bounds checks, the read-back of untouched chunks).
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "env_delta_width_worker.py")


def _child(args, env, drop=()):
    e = dict(os.environ, **env)
    for k in drop:
        e.pop(k, None)
    r = subprocess.run([sys.executable, WORKER] + args, capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_natural_width_rollouts_match_oracle():
    assert "delta width natural ok" in _child(["--natural"], {}, drop=("MARLSAT_ENV_THREADS", "MARLSAT_OBS_DELTA"))


@pytest.mark.parametrize("T", [64, 128, 256, 512])
def test_forced_width_delta_matches_oracle(T):
    assert f"delta width forced {T} ok" in _child(["--forced", str(T)], {"MARLSAT_ENV_THREADS": str(T)})


def test_natural_width_on_the_debug_library():
    lib = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    assert os.path.exists(lib), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    out = _child(["--debug"], {"MARLSAT_LIB": lib}, drop=("MARLSAT_ENV_THREADS", "MARLSAT_OBS_DELTA"))
    assert "delta width debug ok" in out and "libmarlsat_debug.so" in out
