"""The delta step kernel compiled for one geometry (shadow::env_kernel<.., StaticShape<200, 860, 25>>, env_kernels.hip)
against the kernel of any shape and the NumPy oracle, bitwise.

uf200-860 with 25 agents and int32 observations takes the compiled shape by default and the kernel of any shape under
MARLSAT_ENV_STATIC=0; the switch is read once per process, so tests/env_static_shape_worker.py runs every case in one
child process per setting (a module fixture), checks each launch against the oracle there and records the whole obs
tensor, the shadow rows, every step output and every state array after it.  Here, per case: both children passed it,
and their records are bitwise equal.  The geometry is fixed by the specialisation; everything else is small
(B in {1, 3, 8, 12}, at most 6 launches, 4 instances).

  * running steps into a warm tensor (B = 1, 3, 8, 12); the first step into a fresh tensor; two states of different
    instances stepped into one tensor; invalidate_obs; planted step counters (reset workgroups and covered envs); a
    whole-batch timeout with B = 12 > rq_cap = 8; an env one flip from its planted solution; mode-1 actions across the
    quarter rule; PBRS; no auto-reset (the mode-1 kernel); an obs tensor misaligned by one element;
  * dispatch: msat_env_static_shape is 1 for (200, 860, 25) int32 and 0 for 20 agents, 861 clauses, 199 variables,
    int8 and 2-literal clauses (no GPU), and each neighbour still steps equal to the oracle;
  * a running and a reset case on the debug library (bounds checks, the read-back of every unchanged element), equal
    to the product library's records.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

WORKER = os.path.join(ROOT, "tests", "env_static_shape_worker.py")
DROP = ("MARLSAT_ENV_THREADS", "MARLSAT_ENV_STATIC", "MARLSAT_OBS_DELTA", "MARLSAT_OBS_DELTA_GROUP", "MARLSAT_LIB",
        "MARLSAT_RESET_QUEUE", "MARLSAT_ABLATE")
CASES = ("running_warm", "first_step_fresh", "two_states_one_tensor", "invalidate_obs", "timeouts",
         "whole_batch_timeout", "solved", "action_mode1", "pbrs", "no_autoreset", "misaligned", "neighbours")
DEBUG_CASES = ("running_warm", "timeouts")
DEBUG_LIB = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")


def _child(args, env):
    e = {k: v for k, v in os.environ.items() if k not in DROP}
    e.update(env)
    r = subprocess.run([sys.executable, WORKER] + args, capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _cases(tmp, tag, env, extra=()):
    """One child: (status per case, arrays by name)."""
    path = os.path.join(str(tmp), tag + ".npz")
    out = _child(["--dump", path] + list(extra), env)
    assert f"static shape cases done static={0 if env.get('MARLSAT_ENV_STATIC') == '0' else 1}" in out, out[-2000:]
    status = json.loads(next(ln for ln in out.splitlines() if ln.startswith("STATUS "))[7:])
    with np.load(path) as z:
        return status, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("static_shape")
    return {"static": _cases(tmp, "static", {}), "generic": _cases(tmp, "generic", {"MARLSAT_ENV_STATIC": "0"})}


def _equal_records(a, b, prefixes, what):
    keys_a = sorted(k for k in a if k.startswith(prefixes))
    keys_b = sorted(k for k in b if k.startswith(prefixes))
    assert keys_a and keys_a == keys_b, (what, keys_a[:4], keys_b[:4])
    for k in keys_a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"
    return len(keys_a)


# the record names of a case (tests/env_static_shape_worker.py: rollout / two_states names)
PREFIX = {"running_warm": ("running_warm",), "first_step_fresh": ("first_step_fresh.",),
          "two_states_one_tensor": ("two_states.",), "invalidate_obs": ("invalidate.",), "timeouts": ("timeouts.",),
          "whole_batch_timeout": ("whole_batch.",), "solved": ("solved.",), "action_mode1": ("action_mode1.",),
          "pbrs": ("pbrs.",), "no_autoreset": ("no_autoreset",), "misaligned": ("misaligned.",),
          "neighbours": ("neighbour_",)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_static_kernel_equals_generic_kernel_and_oracle(runs, case):
    for tag in ("static", "generic"):
        status = runs[tag][0]
        assert status.get(case) == "ok", f"{tag} process, case {case}: {status.get(case, 'not run')}"
    n = _equal_records(runs["static"][1], runs["generic"][1], PREFIX[case], case)
    assert n >= 12  # one launch leaves obs, shadow rows, 5 outputs and 7 state arrays at the least


@pytest.fixture(scope="module")
def debug_run(tmp_path_factory):
    assert os.path.exists(DEBUG_LIB), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    return _cases(tmp_path_factory.mktemp("static_shape_debug"), "debug", {"MARLSAT_LIB": DEBUG_LIB}, ["--debug"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEBUG_CASES)
def test_static_kernel_on_the_debug_library(runs, debug_run, case):
    status, arrays = debug_run
    assert status.get(case) == "ok", f"debug library, case {case}: {status.get(case, 'not run')}"
    _equal_records(arrays, runs["static"][1], PREFIX[case], f"debug {case}")


@pytest.mark.parametrize("static", ["1", "0"])
def test_dispatch_export_on_the_host(static):
    """msat_env_static_shape over the compiled shape and its neighbours, with the switch on and off: no GPU call."""
    out = _child(["--host"], {} if static == "1" else {"MARLSAT_ENV_STATIC": "0"})
    assert f"static shape host ok static={static}" in out
