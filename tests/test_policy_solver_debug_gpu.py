"""GPU: the policy solver on libmarlsat_debug.so (MSAT_DEBUG: every launch synchronised, every index of the track,
pick and sampling kernels checked against its buffer's extent), in a child process so that the library it loads is
the debug one.  The result must be that of the same script in this process (the product library)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib")

SCRIPT = r"""
import sys, numpy as np
sys.path[:0] = [{root!r}, {root!r} + '/marl-sat_amd']
from marlsat import _lib, SATEnv
from marlsat.learners.gnn import GNNActorCritic
from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner
from marlsat.random import Key
from marlsat.solvers.policy import solve_pool_with_policy
from marlsat.utils.generate_cnf_dataset import generate_problem_pool
env = SATEnv(23, 97, max_steps=16, vars_per_agent=8)  # V = 23: three agents of 8, 8, 7 variables
pool = env.make_pool(generate_problem_pool(23, 97, 5, size_id=0))
net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, 23, device="cuda", seed=4)
lr = MAPPOLearner(dict(NUM_ENVS=15, NUM_STEPS=1, MINIBATCH_SIZE=15), env, net, pool)
res = solve_pool_with_policy(lr, pool, tries=3, rounds=2, max_steps=16, temperature=0.7, finish_tries=4,
                             finish_flips=5000, max_batch=7, key=Key(5, 0))
np.savez({out!r}, **res)
print("policy solver ok", _lib.LIB_PATH)
"""


def _run_child(tmp_path, lib):
    out = str(tmp_path / (lib + ".npz"))
    env = dict(os.environ, MARLSAT_LIB=os.path.join(LIBDIR, lib), MARLSAT_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT.format(root=ROOT, out=out)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "policy solver ok" in r.stdout and lib in r.stdout
    return dict(np.load(out))


def test_debug_library_runs_the_policy_solver(tmp_path):
    path = os.path.join(LIBDIR, "libmarlsat_debug.so")
    assert os.path.exists(path), "libmarlsat_debug.so is not built (make -C marl-sat_amd debug)"
    dbg = _run_child(tmp_path, "libmarlsat_debug.so")
    out = str(tmp_path / "here.npz")
    exec(compile(SCRIPT.format(root=ROOT, out=out), "<policy solver script>", "exec"), {})  # this process's library
    ref = dict(np.load(out))
    assert dbg["solved"].all()
    for k in ref:
        np.testing.assert_array_equal(dbg[k], ref[k], err_msg=k)
