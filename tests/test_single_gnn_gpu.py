"""GPU: GNNSingleActorCritic (learners/single_gnn.py: one encoder pass, both heads) against the float64 oracle
(tests/single_oracle.py on oracle/net.py) on the same fp32 parameters: logits (S, V), value (S,) and every parameter
gradient for random cotangents, on the three precision paths.

Bars, the project's: outputs as tests/test_gnn_gpu.py (1e-5 normwise, and elementwise 1e-5 |ref| + FWD_FACTOR x the
error of the same oracle in float32 on the CPU); gradients as tests/test_bc_learner_gpu.py's _yard_close, restated
here (1e-4 normwise, and elementwise 1e-5 |ref| + 4 x E32 + the ReLU-kink allowance)."""
import numpy as np
import pytest
import torch

import irregular_pools as ip
import single_oracle as so
from oracle import net as onet
from oracle.sat_env import OracleSATEnv
from test_gnn_gpu import FWD_FACTOR, _close_norm, _close_yard, _set_path

pytestmark = pytest.mark.gpu

GRAD_FACTOR = 4.0  # tests/test_gnn_gpu.py
CASES = [(12, 40, 64, 2), (23, 97, 64, 2), (20, 91, 128, 2)]  # V, C, H, L


def _yard_close(dev, ref, yard, what, extra, failures):
    """Both gradient bars for one tensor (tests/test_bc_learner_gpu.py); a miss is appended to ``failures``."""
    dev, ref, yard = (np.asarray(a, np.float64) for a in (dev, ref, yard))
    assert np.isfinite(dev).all(), what
    err = np.abs(dev - ref)
    scale = max(np.abs(ref).max(), 1e-12)
    e32 = np.abs(yard - ref).max()
    bound = 1e-5 * np.abs(ref) + GRAD_FACTOR * e32 + np.asarray(extra, np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    if err.max() > 0.5e-4 * scale or worst > 0.5:
        print(f"  {what}: max err {err.max():.3g}, max |ref| {scale:.3g} (normwise {err.max() / scale:.3g}), fp32 oracle "
              f"err {e32:.3g}, elementwise ratio {worst:.3g}")
    if err.max() > 1e-4 * scale:
        failures.append(f"{what}: normwise {err.max():.3g} / {scale:.3g} = {err.max() / scale:.3g} > 1e-4")
    if not (err <= bound).all():
        failures.append(f"{what}: elementwise max err {err.max():.3g}, worst ratio {worst:.3g}")
    return worst


def _setup(V, C, H, L, S, seed=0, pool=None, inst=None, x=None):
    from marlsat import SATEnv
    from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates
    from marlsat.learners.single_gnn import GNNSingleActorCritic
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    if pool is None:
        pool = generate_problem_pool(V, C, 4, size_id=7)
    env = SATEnv(V, C, max_steps=10, vars_per_agent=V)
    assert env.num_agents == 1
    dpool = env.make_pool(pool)
    net = GNNSingleActorCritic(H, L, V, device="cuda", seed=seed)
    tree32 = {k: v.float().numpy() for k, v in onet.init_params(so.single_param_shapes(H, L), seed=seed + 1).items()}
    net.load_flax(tree32)
    tpl = DeviceTemplates(build_templates(pool, V, 1), 1, "cuda")
    rng = np.random.default_rng(seed)
    if inst is None:
        inst = rng.integers(0, pool.shape[0], S).astype(np.int32)
        x = rng.integers(0, 2, (S, V)).astype(np.uint8)
    mk = lambda **kw: assemble(tpl, dpool.packed, dpool.static_var_features(), torch.from_numpy(inst).cuda(),
                               torch.from_numpy(x).cuda(), **kw)
    ora = OracleSATEnv(V, C, 10, vars_per_agent=V)
    _, ost = ora.reset(pool[inst], x.astype(np.int32))
    Ap, An = onet.dense_graph(pool[inst], V)
    args = (torch.from_numpy(ora.static_var_features(pool[inst])).double(), torch.from_numpy(x).double(),
            torch.from_numpy(ora.clause_features(ost)).double(), Ap, An)
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tree32.items()}
    return net, mk, P, args


def _check(net, b, P, args, L, label):
    onet.RELU_LOG = log = []
    try:
        ref_l, ref_v = so.single_forward(P, L, args)
    finally:
        onet.RELU_LOG = None
    logits, value, state = net.forward(b, save=True)
    assert tuple(logits.shape) == tuple(ref_l.shape) and tuple(value.shape) == tuple(ref_v.shape)
    rl, rv = ref_l.detach().numpy(), ref_v.detach().numpy()
    _close_norm(logits.cpu().numpy(), rl, 1e-5, "logits")
    _close_norm(value.cpu().numpy(), rv, 1e-5, "value")
    g = torch.Generator().manual_seed(3)
    wl = torch.randn(ref_l.shape, generator=g, dtype=torch.float64)
    wv = torch.randn(ref_v.shape, generator=g, dtype=torch.float64)
    obj = (ref_l * wl).sum() + (ref_v * wv).sum()
    kink, _ = onet.kink_bound(obj, P, log)
    obj.backward()
    P32 = {k: v.detach().float().requires_grad_(True) for k, v in P.items()}
    y_l, y_v = so.single_forward(P32, L, tuple(a.float() for a in args))
    ((y_l * wl.float()).sum() + (y_v * wv.float()).sum()).backward()
    report, elem = [], {}
    _close_yard(logits.cpu().numpy(), rl, y_l.detach().numpy(), FWD_FACTOR, "logits", report, worst=elem)
    _close_yard(value.cpu().numpy(), rv, y_v.detach().numpy(), FWD_FACTOR, "value", report, worst=elem)
    net.grads.zero_()
    net.backward(b, state, wl.float().cuda().contiguous(), wv.float().cuda().contiguous())
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
    return logits, value


@pytest.mark.parametrize("path", ["default", "bf16x3", "fp32"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("V,C,H,L", CASES)
def test_forward_backward_match_oracle(V, C, H, L, S, path, monkeypatch, c_precision):
    _set_path(monkeypatch, path, c_precision)
    net, mk, P, args = _setup(V, C, H, L, S)
    b = mk(critic_only=True)
    assert (b.g0, b.G, b.Nv) == (0, 1, S * V)
    _check(net, b, P, args, L, f"single {path} V={V} H={H} S={S}")


def test_irregular_pool_matches_oracle(monkeypatch, c_precision):
    """quirks23: literal 0 slots, a variable twice in a clause, an all-zero clause, variables in no clause."""
    _set_path(monkeypatch, "default", c_precision)
    p = ip.get("quirks23")
    net, mk, P, args = _setup(p.V, p.C, 64, 2, len(p.inst), pool=p.pool, inst=p.inst, x=p.x)
    _check(net, mk(critic_only=True), P, args, 2, "single quirks23")


def test_heads_only_forward_and_flags():
    """actor / critic alone return the other as None and the same bits as the joint forward."""
    net, mk, P, args = _setup(12, 40, 64, 2, 3)
    b = mk(critic_only=True)
    lg, val, _ = net.forward(b)
    la, none_v, _ = net.forward(b, critic=False)
    none_l, vc, _ = net.forward(b, actor=False)
    assert none_v is None and none_l is None
    assert torch.equal(la.view(torch.int32), lg.view(torch.int32)) and torch.equal(vc.view(torch.int32),
                                                                                  val.view(torch.int32))


def test_flax_round_trip_is_bitwise():
    from marlsat.learners import params as Pm
    from marlsat.learners.single_gnn import GNNSingleActorCritic

    a = GNNSingleActorCritic(64, 2, 12, device="cuda", seed=5)
    flat = a.params.cpu().numpy()
    tree = a.to_flax()
    assert "actor_dense_1/kernel" in tree and "critic_output/bias" in tree and "agent_id_embedding/embedding" not in tree
    assert np.array_equal(Pm.single_from_flax(tree, 64, 2).view(np.int32), flat.view(np.int32))
    b = GNNSingleActorCritic(64, 2, 12, device="cuda", seed=6)
    assert not torch.equal(a.params, b.params)
    b.load_flax(tree)
    assert torch.equal(a.params.view(torch.int32), b.params.view(torch.int32))
    tab, size = Pm.offsets(Pm.single_layout(64, 2))
    assert size == a.params.numel() and all(o % 4 == 0 for o, _ in tab.values())


def test_a_batch_with_other_graphs_raises():
    net, mk, P, args = _setup(12, 40, 64, 2, 3)
    full = mk()  # graph 0 and the one agent's graph: G = 2
    assert full.G == 2
    with pytest.raises(ValueError, match="critic-only"):
        net.forward(full)
    with pytest.raises(ValueError, match="critic-only"):
        net.forward(mk(actor_only=True), critic=False)
    b = mk(critic_only=True)
    _, _, state = net.forward(b, save=True)
    with pytest.raises(ValueError, match="critic-only"):
        net.backward(full, state, torch.zeros((3, 12), device="cuda"), torch.zeros((3,), device="cuda"))
