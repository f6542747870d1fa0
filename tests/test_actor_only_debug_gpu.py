"""GPU: one actor-only assemble + forward + backward on libmarlsat_debug.so (MSAT_DEBUG: every launch
synchronised, every index of the assembly kernel -- the rebased template reads included -- and of the actor pools
checked against its buffer's extent) with MARLSAT_DEBUG=1 (NaN-poisoned feature rows, planned totals compared with
msat_graph_bases), in a child process so that the library it loads is the debug one.  It must end clean with the
logits and gradients of the same script on the product library in this process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib")

SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {root!r} + '/marl-sat_amd', {root!r} + '/tests']
import irregular_pools as ip
from marlsat import _lib, SATEnv
from marlsat.learners import graphs
from marlsat.learners.gnn import GNNActorCritic
p = ip.get("quirks23")  # a padded slot, a clause-less agent between two ordinary graphs, isolated variables
env = SATEnv(p.V, p.C, max_steps=10, vars_per_agent=p.vpa)
A = env.num_agents
dpool = env.make_pool(p.pool)
tpl = graphs.DeviceTemplates(graphs.build_templates(p.pool, p.V, A), A, "cuda")
inst, x = torch.from_numpy(p.inst).cuda(), torch.from_numpy(p.x).cuda()
graphs.DEBUG_CHECKS = True
tot = graphs.batch_totals(tpl, inst, [0, len(p.inst)], actor_only=True)[0]
b = graphs.assemble(tpl, dpool.packed, dpool.static_var_features(), inst, x, totals=tot, actor_only=True)
assert (b.g0, b.G) == (1, A)
net = GNNActorCritic(64, 2, A, env.max_vars_per_agent, 0, p.V, device="cuda", seed=3)
logits, value, state = net.forward(b, critic=False, save=True)
assert value is None
dl = torch.where(torch.isfinite(logits), torch.linspace(-1, 1, logits.numel(), device="cuda").view_as(logits),
                 torch.zeros_like(logits)).contiguous()
net.grads.zero_()
net.backward(b, state, dl, None)
torch.cuda.synchronize()
assert torch.isfinite(net.grads).all()
np.savez({out!r}, logits=logits.cpu().numpy(), grads=net.grads.cpu().numpy())
print("actor-only ok", _lib.LIB_PATH)
"""


def test_debug_library_runs_an_actor_only_batch(tmp_path):
    assert os.path.exists(os.path.join(LIBDIR, "libmarlsat_debug.so")), \
        "libmarlsat_debug.so is not built (make -C marl-sat_amd debug)"
    out = str(tmp_path / "debug.npz")
    env = dict(os.environ, MARLSAT_LIB=os.path.join(LIBDIR, "libmarlsat_debug.so"), MARLSAT_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT.format(root=ROOT, out=out)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "actor-only ok" in r.stdout and "libmarlsat_debug.so" in r.stdout
    assert "MSAT_DEBUG" not in r.stderr
    dbg = dict(np.load(out))
    here = str(tmp_path / "here.npz")
    from marlsat.learners import graphs

    was = graphs.DEBUG_CHECKS
    try:
        exec(compile(SCRIPT.format(root=ROOT, out=here), "<actor-only script>", "exec"), {})  # the product library
    finally:
        graphs.DEBUG_CHECKS = was
    ref = dict(np.load(here))
    assert np.isfinite(ref["grads"]).all() and np.abs(ref["grads"]).max() > 0
    for k in ref:  # the same kernels with checks compiled in: the same bits
        np.testing.assert_array_equal(dbg[k].view(np.int32), ref[k].view(np.int32), err_msg=k)
