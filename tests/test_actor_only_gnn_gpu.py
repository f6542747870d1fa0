"""GPU: the network on an actor-only graph batch (assemble(actor_only=True)) against the same network on the
full batch of the same samples: the logits are expected bit for bit on every precision path and in both action
modes, because each row's arithmetic (its MFMA row, its gather sums, its LayerNorm, its agent's pools) reads no
other row, and the actor-only batch holds exactly the full batch's rows of graphs 1..A.

One caveat, not met here: on 'fp16x2' a 128-row tile flagged for the bf16x3 fixup is recomputed whole, so a row
can change path with its tile mates, and the tiles of the two batches hold different rows.  oracle.net.init_params'
networks at these shapes gave equal bits on an MI355X in every case below, the H = 128 fp16x2 ones included.

Also: the guards -- the critic head (forward or backward) on an actor-only batch and the actor head on a
critic-only batch raise instead of pooling another graph's rows."""
import numpy as np
import pytest
import torch

import irregular_pools as ip
from test_gnn_gpu import _set_path, _setup

pytestmark = pytest.mark.gpu

L = 2
CASES = [  # name, H
    ("uf20", 64),  # uf20-91 with agents of 7, 7, 6 over 4 instances
    ("quirks23", 64),
    ("quirks23", 128),  # the register-A MFMA GRU kernels (H = 128 only)
]
_POOLS = {}


def _samples(name):
    """(V, C, vpa, pool, inst, x), built once."""
    if name not in _POOLS:
        if name == "uf20":
            from marlsat.utils.generate_cnf_dataset import generate_problem_pool

            V, C, S = 20, 91, 5
            pool = generate_problem_pool(V, C, 4, size_id=7)
            rng = np.random.default_rng(20)
            inst = np.array([0, 1, 2, 3, 1], np.int32)  # every instance, one twice
            _POOLS[name] = (V, C, 7, pool, inst, rng.integers(0, 2, (S, V)).astype(np.uint8))
        else:
            p = ip.get(name)
            _POOLS[name] = (p.V, p.C, p.vpa, p.pool, p.inst, p.x)
    return _POOLS[name]


def _batches(name, H, mode):
    from marlsat import SATEnv
    from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates

    V, C, vpa, pool, inst, x = _samples(name)
    net, full, P, batch, av, am, A, M = _setup(V, C, vpa, H, L, len(inst), mode, pool=pool, inst=inst, x=x)
    env = SATEnv(V, C, 10, vars_per_agent=vpa)
    dpool = env.make_pool(pool)
    tpl = DeviceTemplates(build_templates(pool, V, A), A, "cuda")
    mk = lambda **kw: assemble(tpl, dpool.packed, dpool.static_var_features(), torch.from_numpy(inst).cuda(),
                               torch.from_numpy(x).cuda(), **kw)
    return net, full, mk, A, M, V


@pytest.mark.parametrize("path", ["default", "bf16x3", "fp32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,H", CASES)
def test_actor_only_logits_equal_full_batch_bitwise(name, H, mode, path, monkeypatch, c_precision):
    _set_path(monkeypatch, path, c_precision)
    net, full, mk, A, M, V = _batches(name, H, mode)
    if name == "uf20":
        assert (A, M, V - (A - 1) * M) == (3, 7, 6)  # agents of 7, 7, 6: a padded slot
    act = mk(actor_only=True)
    assert (act.g0, act.G, full.g0, full.G) == (1, A, 0, A + 1)
    assert 0 < act.Nv < full.Nv and 0 < act.Nc < full.Nc
    want, value, _ = net.forward(full)
    got, none, _ = net.forward(act, critic=False)
    assert none is None and got.shape == want.shape and torch.isfinite(value).all()
    fin = torch.isfinite(want)
    assert fin.any() and torch.equal(fin, torch.isfinite(got))
    diff = (got[fin] - want[fin]).abs().max().item()
    print(f"{name} H={H} mode={mode} {path}: max |actor-only - full| logit = {diff:.3e}")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"logits differ, max {diff:.3e}"
    if path == "default" and H == 128:  # no weight split left fp16's range (that would send every tile to the fixup)
        assert int(net._h2bad.sum()) == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_heads_refuse_a_batch_without_their_graphs(mode):
    net, full, mk, A, M, V = _batches("uf20", 64, mode)
    act, crit = mk(actor_only=True), mk(critic_only=True)
    with pytest.raises(ValueError, match="actor-only"):
        net.forward(act)  # critic=True is the default
    with pytest.raises(ValueError, match="actor-only"):
        net.forward(act, actor=False, critic=True)
    with pytest.raises(ValueError, match="critic-only"):
        net.forward(crit)
    logits, _, state = net.forward(act, critic=False, save=True)
    dl = torch.zeros_like(logits)
    with pytest.raises(ValueError, match="actor-only"):
        net.backward(act, state, dl, torch.zeros((act.S,), device="cuda"))
    _, value, cstate = net.forward(crit, actor=False, save=True)
    with pytest.raises(ValueError, match="critic-only"):
        net.backward(crit, cstate, dl, torch.zeros_like(value))
    # what each batch is for still runs
    net.grads.zero_()
    net.backward(act, state, dl, None)
    net.backward(crit, cstate, None, torch.zeros_like(value))
    assert torch.isfinite(net.grads).all()
