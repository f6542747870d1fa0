"""GPU: the device GNN actor-critic (forward, backward, critic-only batch, gathers) against the float64 oracle's
masked dense per-agent encoders (oracle/net.py) on the irregular pools of tests/irregular_pools.py: literal 0,
a variable twice in a clause, 2- and 1-wide clauses, variables in no clause, and an agent whose graph has var
rows only.  Same checks and the same bars as the regular cases of tests/test_gnn_gpu.py: outputs 1e-5
normwise, gradients 1e-4 of each tensor's maximum, and on every element 1e-5 |ref| + FWD_FACTOR / GRAD_FACTOR
x the float32 CPU oracle's error (+ the ReLU-kink allowance).  The PPO-loss check on these pools is
test_gnn_gpu.py::test_ppo_loss_and_grads_match_oracle[*-quirks23].

The parameters are oracle.net.init_params', biases included and non-zero, so a variable in no clause is not
the constant LayerNorm row of DESIGN.md section 5 (that hazard needs zero biases and is out of scope here).

Measured on an MI355X, worst err / bound over the three paths (1.0 = at the bar; normwise outputs, normwise
gradients, elementwise outputs, elementwise gradients):
  quirks23 H=64  mode 0: 0.19 0.013 0.45 0.21      quirks23 H=128 mode 0: 0.23 0.015 0.62 0.24
  k2       H=64  mode 0: 0.24 0.009 0.45 0.28      k1       H=64  mode 0: 0.75 0.018 0.52 0.34
  solo     H=64  mode 0: 0.10 0.018 0.39 0.23      quirks23 H=64  mode 1: 0.19 0.020 0.45 0.20
  k2       H=64  mode 1: 0.24 0.026 0.45 0.25
No case needed a bar of its own; k1's outputs (six unit clauses, two samples) come closest to one."""
import numpy as np
import pytest
import torch

import irregular_pools as ip
from test_gnn_gpu import _check_gathers, _forward_backward_check, _set_path, _setup

pytestmark = pytest.mark.gpu

CASES = [  # pool, H, mode
    ("quirks23", 64, 0), ("k2", 64, 0), ("k1", 64, 0), ("solo", 64, 0), ("quirks23", 128, 0),
    ("quirks23", 64, 1), ("k2", 64, 1),
]
L = 2


def _irregular_setup(name, H, mode, seed=0):
    p = ip.get(name)
    return p, _setup(p.V, p.C, p.vpa, H, L, len(p.inst), mode, seed=seed, pool=p.pool, inst=p.inst, x=p.x)


@pytest.mark.parametrize("path", ["default", "bf16x3", "fp32"])
@pytest.mark.parametrize("name,H,mode", CASES)
def test_forward_backward_match_oracle_on_irregular_pools(name, H, mode, path, monkeypatch, c_precision):
    """path: 'default' and 'bf16x3' with phi folded, 'fp32' in the reference's operation order (_set_path)."""
    _set_path(monkeypatch, path, c_precision)
    p, (net, b, P, batch, av, am, A, M) = _irregular_setup(name, H, mode)
    biases = [k for k in P if k.endswith("/bias")]
    assert biases and all(bool((P[k] != 0).all()) for k in biases)  # not the zero-bias hazard
    if name == "quirks23":
        nc = b.nc.cpu().numpy()
        assert (nc == 0).any() and (nc[0] > 0) and (nc[-1] > 0)
    report, norm, (logits, value) = _forward_backward_check(net, b, P, batch, av, am, L, mode,
                                                            f"irregular {name} {path} H={H} mode={mode}")
    # the -inf pattern is the action mask's, whatever the graphs look like
    fin = torch.isfinite(logits).cpu()
    want = torch.cat([am, torch.ones((A, 1), dtype=torch.bool)], -1)[None] if mode == 0 else am[None, :, :, None]
    assert torch.equal(fin, want.expand_as(fin))
    assert torch.isfinite(value).all()
    print(f"ratios {name} H={H} mode={mode} {path}: err / bound, normwise outputs {norm['outputs']:.3f} gradients "
          f"{norm['gradients']:.3f}; elementwise outputs {norm['elementwise outputs']:.3f} gradients "
          f"{norm['elementwise gradients']:.3f}")


@pytest.mark.parametrize("name", ["quirks23", "k2", "k1", "solo"])
def test_critic_only_batch_equals_full_on_irregular_pools(name):
    from marlsat import SATEnv
    from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates

    p, (net, b, P, batch, av, am, A, M) = _irregular_setup(name, 64, 0)
    _, v_full, _ = net.forward(b)
    env = SATEnv(p.V, p.C, 10, vars_per_agent=p.vpa)
    dpool = env.make_pool(p.pool)
    tpl = DeviceTemplates(build_templates(p.pool, p.V, A), A, "cuda")
    bc = assemble(tpl, dpool.packed, dpool.static_var_features(), torch.from_numpy(p.inst).cuda(),
                  torch.from_numpy(p.x).cuda(), critic_only=True)
    assert bc.G == 1 and bc.Nc == len(p.inst) * p.C
    _, v_crit, _ = net.forward(bc, actor=False)
    assert torch.isfinite(v_full).all() and torch.equal(v_full, v_crit)


def test_gathers_and_degree_features_on_quirks23():
    """The gather kernels and count features on a batch with -1 slots inside real clause rows, var rows with an
    empty incidence list and a graph without clause rows."""
    p, (net, b, P, batch, av, am, A, M) = _irregular_setup("quirks23", 64, 0)
    slots, ptr, nc = b.slots.cpu().numpy(), b.ptr.cpu().numpy(), b.nc.cpu().numpy()
    assert ((slots == -1).any(1) & (slots >= 0).any(1)).any() and (slots == -1).all(1).any()
    assert (np.diff(ptr) == 0).any() and (nc == 0).any()
    assert (b.cdeg[:, :2].cpu().numpy().max(1) >= 2).any()  # a variable twice in a clause counts 2
    _check_gathers(b)
