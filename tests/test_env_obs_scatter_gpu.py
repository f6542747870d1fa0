"""The sparse delta observation write of int32 observations: every changed element stored on its own, by the lane
that holds what decides it (marl-sat_amd/csrc/env_kernels.hip, scatter_obs).

  * clause status: the lane that evaluated clause c in the scan stores it into the rows of the owners of the clause's
    real literals -- and, for a clause that holds a literal 0, into the row of every agent i >= rem when the agents
    are of unequal size (the reference quirk the agent tables reproduce);
  * own variables: lane v stores element (owner of v, v);
  * neighbour variables: task (agent, word) stores the set bits of (x ^ shadow x) & nbr word.
No agent table is staged in LDS and no barrier follows the clause scan's.  A reset, a row that names another instance
and a step that flips more than a quarter of the V + C source bits keep the full write; the rollouts alternate between
the two on one tensor, bitwise against a full-write twin and the NumPy oracle.  The checks are in
tests/env_obs_scatter_worker.py; the forced widths and the debug library run it as a child process.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
import env_obs_scatter_worker as W

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "env_obs_scatter_worker.py")
ROLLOUT_SHAPES = ("v33c70", "v64c64", "v31c33", "v96c832", W.NULL_SHAPE)
CASES = [(s, am, off) for s in ROLLOUT_SHAPES for am in (0, 1) for off in (0, 1, 2, 3)]


@pytest.mark.parametrize("shape,action_mode,offset", CASES)
def test_scatter_rollout_matches_full_write_and_oracle(shape, action_mode, offset):
    few, many, resets, null_changed = W.rollout(shape, action_mode, offset)
    assert few >= 1 and resets >= W.B  # the sparse path ran, and every env was reset in between
    if action_mode == 1:
        assert many >= 1  # the quarter rule was crossed in both directions
    if shape == W.NULL_SHAPE:
        assert null_changed >= 1  # a sparse step changed a clause that holds a literal 0


@pytest.mark.parametrize("shape,offset", [("v33c70", 0), ("v33c70", 3), ("v96c832", 1), (W.NULL_SHAPE, 2)])
def test_noop_steps_store_nothing(shape, offset):
    W.noop_stores_nothing(shape, offset)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_flip_of_a_variable_in_no_clause_stores_one_element(offset):
    W.lone_variable_flip(offset)


def _child(args, env):
    r = subprocess.run([sys.executable, WORKER] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("T", [64, 512])
def test_scatter_at_forced_width(T):
    assert f"obs scatter threads {T} ok" in _child(["--threads", str(T)], {"MARLSAT_ENV_THREADS": str(T)})


def test_scatter_on_the_debug_library():
    lib = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    assert os.path.exists(lib), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    out = _child(["--debug"], {"MARLSAT_LIB": lib})
    assert "obs scatter debug ok" in out and "libmarlsat_debug.so" in out
