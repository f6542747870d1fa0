"""GPU: GNNAssignmentPredictor (learners/assign_gnn.py: the shared encoder and a 2-wide head over the variable rows)
against the float64 oracle (tests/assign_oracle.py on oracle/net.py) on the same fp32 parameters: the (S * V, 2)
logits and every parameter gradient for a random dlogits, on the three precision paths.

Bars: those of tests/test_single_gnn_gpu.py, imported (outputs 1e-5 normwise and the fp32-yardstick elementwise bar
of tests/test_gnn_gpu.py; gradients _yard_close)."""
import numpy as np
import pytest
import torch

import assign_oracle as ao
from oracle import net as onet
from test_gnn_gpu import FWD_FACTOR, _close_norm, _close_yard, _set_path
from test_single_gnn_gpu import _yard_close

pytestmark = pytest.mark.gpu

H, L, S = 64, 2, 3


def _pool(V, C, n=4):
    """uf20-91 from the planted generator; any other shape irregular: random literals (variables repeat within a
    clause), a literal 0 and a variable with both signs in one clause; the last V slots name every variable once."""
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    if (V, C) == (20, 91):
        return generate_problem_pool(V, C, n, size_id=7)
    assert 3 * C >= V + 6
    rng = np.random.default_rng(V * 100 + C)
    cl = rng.integers(1, V + 1, (n, C, 3))
    for i in range(n):
        cl[i].reshape(-1)[3 * C - V:] = rng.permutation(V) + 1
    cl = cl * rng.choice([-1, 1], (n, C, 3))
    cl[:, 0, 2] = 0
    cl[:, 1, 1] = -cl[:, 1, 0]
    return cl.astype(np.int32)


def _net(seed=0):
    from marlsat.learners.assign_gnn import GNNAssignmentPredictor

    net = GNNAssignmentPredictor(H, L, device="cuda", seed=seed)
    tree32 = {k: v.float().numpy() for k, v in onet.init_params(ao.assign_param_shapes(H, L), seed=seed + 1).items()}
    net.load_flax(tree32)
    return net, tree32


def _batch(V, C, seed=0):
    from marlsat import SATEnv
    from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates

    pool = _pool(V, C)
    dpool = SATEnv(V, C, max_steps=10, vars_per_agent=V).make_pool(pool)
    tpl = DeviceTemplates(build_templates(pool, V, 1), 1, "cuda")
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, pool.shape[0], S).astype(np.int32)
    x = rng.integers(0, 2, (S, V)).astype(np.uint8)
    mk = lambda **kw: assemble(tpl, dpool.packed, dpool.static_var_features(), torch.from_numpy(inst).cuda(),
                               torch.from_numpy(x).cuda(), **kw)
    return mk, ao.graph_args(pool, inst, x, V, C)


def _check(net, tree32, b, args, V, label):
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tree32.items()}
    onet.RELU_LOG = log = []
    try:
        ref = ao.assign_logits(P, L, *args)  # (S, V, 2)
    finally:
        onet.RELU_LOG = None
    logits, value, state = net.forward(b, save=True)
    assert value is None and tuple(logits.shape) == (S * V, 2)
    rl = ref.detach().numpy().reshape(S * V, 2)
    _close_norm(logits.cpu().numpy(), rl, 1e-5, "logits")
    w = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    obj = (ref * w).sum()
    kink, _ = onet.kink_bound(obj, P, log)
    obj.backward()
    P32 = {k: v.detach().float().requires_grad_(True) for k, v in P.items()}
    y = ao.assign_logits(P32, L, *(a.float() for a in args))
    (y * w.float()).sum().backward()
    report, elem = [], {}
    _close_yard(logits.cpu().numpy(), rl, y.detach().numpy().reshape(S * V, 2), FWD_FACTOR, "logits", report,
                worst=elem)
    net.grads.zero_()
    net.backward(b, state, w.float().reshape(S * V, 2).cuda().contiguous(), None)
    got = net.to_flax(grads=True)
    assert set(got) == set(P)
    failures, worst = [], ("", 0.0)
    for k, p in P.items():
        g64 = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
        g32 = P32[k].grad.double().numpy() if P32[k].grad is not None else np.zeros(p.shape)
        r = _yard_close(got[k], g64, g32, f"{label} grad {k}", kink[k], failures)
        worst = max(worst, (k, r), key=lambda t: t[1])
    print(f"{label}: outputs err / bound {({k: round(v, 3) for k, v in elem.items()})}, worst gradient ratio "
          f"{worst[1]:.3g} ({worst[0]})")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("path", ["default", "bf16x3", "fp32"])
@pytest.mark.parametrize("V,C", [(20, 91), (7, 5)])
def test_forward_backward_match_oracle(V, C, path, monkeypatch, c_precision):
    _set_path(monkeypatch, path, c_precision)
    net, tree32 = _net()
    mk, args = _batch(V, C)
    b = mk(critic_only=True)
    assert (b.g0, b.G, b.Nv) == (0, 1, S * V)
    _check(net, tree32, b, args, V, f"assign {path} V={V}")


def test_one_network_serves_two_sizes(monkeypatch, c_precision):
    """The same object, the same parameter buffer: V = 20 and then V = 13."""
    _set_path(monkeypatch, "default", c_precision)
    net, tree32 = _net()
    before = net.params.clone()
    for V, C in ((20, 91), (13, 40)):
        mk, args = _batch(V, C)
        _check(net, tree32, mk(critic_only=True), args, V, f"assign sizes V={V}")
    assert torch.equal(net.params.view(torch.int32), before.view(torch.int32))
    from marlsat.learners import params as Pm

    assert all("V" not in k for k in Pm.assign_layout(H, L))
    assert net.params.numel() == Pm.offsets(Pm.assign_layout(H, L))[1]


def test_critic_and_other_batches_raise():
    net, _ = _net()
    mk, _ = _batch(20, 91)
    b = mk(critic_only=True)
    with pytest.raises(ValueError, match="no critic"):
        net.forward(b, critic=True)
    _, _, state = net.forward(b, save=True)
    with pytest.raises(ValueError, match="no critic"):
        net.backward(b, state, torch.zeros((S * 20, 2), device="cuda"), torch.zeros((S,), device="cuda"))
    full = mk()
    assert full.G == 2
    with pytest.raises(ValueError, match="critic-only"):
        net.forward(full)
    with pytest.raises(ValueError, match="critic-only"):
        net.forward(mk(actor_only=True))
