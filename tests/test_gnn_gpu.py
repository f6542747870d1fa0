"""GPU parity of the device GNN actor-critic (forward, backward, PPO loss) vs the
torch-CPU oracle of the reference network (oracle/net.py), float64 on the same
fp32 parameters.  Tolerances: forward outputs 1e-5 normwise (|err| <= 1e-5 * max|ref| per
tensor: the phi-folded encoder re-associates fp32 products, so near-zero elements carry
~1e-6 absolute error in either association); gradients 1e-4 relative to the gradient
tensor's max magnitude (fp32 accumulation over L GRU steps and thousands of rows); and on every
element, forward and gradients, |err| <= 1e-5 |ref| + k x the error of the same oracle run in
float32 on the CPU (k = FWD_FACTOR / GRAD_FACTOR, the depth tests' bar)."""
import numpy as np
import pytest
import torch

from oracle import net as onet
from oracle.sat_env import OracleSATEnv

pytestmark = pytest.mark.gpu

CASES = [  # V, C, vpa, H, L, S, action_mode
    (12, 40, 4, 64, 2, 5, 0),
    (20, 91, 10, 64, 3, 4, 0),
    (23, 97, 10, 64, 2, 3, 0),  # padded agent slots
    (16, 60, 4, 64, 2, 4, 1),
    (20, 91, 10, 128, 2, 3, 0),
]


def _setup(V, C, vpa, H, L, S, mode, seed=0, pool=None, inst=None, x=None):
    """pool (N, C, K) int32, inst (S,) int32, x (S, V) uint8: the instances and samples to run on (default:
    generated 3-SAT instances and random samples)."""
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates
    from marlsat import SATEnv
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    if pool is None:
        pool = generate_problem_pool(V, C, 4, size_id=7)
    N = pool.shape[0]
    env = SATEnv(V, C, max_steps=10, vars_per_agent=vpa)
    A, M = env.num_agents, env.max_vars_per_agent
    dpool = env.make_pool(pool)
    net = GNNActorCritic(H, L, A, M, mode, V, device="cuda", seed=seed)
    tree64 = onet.init_params(onet.param_shapes(H, L, A, M, mode), seed=seed + 1)
    tree32 = {k: v.float().numpy() for k, v in tree64.items()}
    net.load_flax(tree32)
    tpl = DeviceTemplates(build_templates(pool, V, A), A, "cuda")
    rng = np.random.default_rng(seed)
    if inst is None:
        inst = rng.integers(0, N, S).astype(np.int32)
        x = rng.integers(0, 2, (S, V)).astype(np.uint8)
    assert inst.shape == (S,) and x.shape == (S, V)
    b = assemble(tpl, dpool.packed, dpool.static_var_features(), torch.from_numpy(inst).cuda(),
                 torch.from_numpy(x).cuda())
    # oracle inputs
    ora = OracleSATEnv(V, C, 10, vars_per_agent=vpa)
    _, ost = ora.reset(pool[inst], x.astype(np.int32))
    Ap, An = onet.dense_graph(pool[inst], V)
    batch = {"svf": torch.from_numpy(ora.static_var_features(pool[inst])).double(),
             "x": torch.from_numpy(x).double(), "cf": torch.from_numpy(ora.clause_features(ost)).double(),
             "A_pos": Ap, "A_neg": An}
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tree32.items()}
    av = torch.from_numpy(ora.agent_vars.astype(np.int64))
    am = torch.from_numpy(ora.action_mask)
    return net, b, P, batch, av, am, A, M


def _close(dev, ref, rtol, atol, what):
    dev = np.asarray(dev, np.float64)
    ref = np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(dev)), what + " (inf pattern)"
    err = np.abs(dev[fin] - ref[fin])
    bound = rtol * np.abs(ref[fin]) + atol
    assert (err <= bound).all(), f"{what}: max err {err.max():.3g}, worst ratio {(err / bound).max():.3g}"


def _close_norm(dev, ref, rtol, what):
    ref = np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    _close(dev, ref, 0.0, rtol * max(np.abs(ref[fin]).max(), 1e-12), what)


# the default path with one switch off (profiles/parity_switch_probe.py's table): the branches gnn.py selects
# when the fp16x2 families are not all on -- fp32 packed rows under the dual launches, and the non-dual fp16x2
# products (msat_gemm_wgrad_h2 when only the data gradients fall back, msat_gemm_h2 when only the weight
# gradients do)
SINGLE_SWITCH = {"planes0": {"use_planes": False}, "gru_x3": {"use_gru_h2": False},
                 "dgrad_x3": {"use_dgrad_h2": False}, "wgrad_x3": {"use_wgrad_h2": False}}
SINGLE_SWITCH_CASES = [(20, 91, 10, 128, 2, 3, 0), (16, 60, 4, 64, 2, 4, 1)]
assert all(c in CASES for c in SINGLE_SWITCH_CASES)


@pytest.mark.parametrize(
    "V,C,vpa,H,L,S,mode,fuse,path",
    [c + fp for fp in ((True, "default"), (True, "bf16x3"), (True, "fp32"), (False, "bf16x3"), (False, "fp32"))
     for c in CASES] + [c + (True, path) for path in SINGLE_SWITCH for c in SINGLE_SWITCH_CASES])
def test_forward_backward_match_oracle(V, C, vpa, H, L, S, mode, fuse, path, monkeypatch, c_precision):
    """fuse: phi folded into the GRU input matrices (else the reference order); path: the arithmetic
    (_set_path: fp16x2 / bf16x3 split kernels at H = 128, packed backward rows; fp32 MFMA; or the default
    path with one switch of SINGLE_SWITCH off)."""
    from marlsat.learners.gnn import GNNActorCritic

    _set_path(monkeypatch, path, c_precision)
    monkeypatch.setattr(GNNActorCritic, "fuse_phi", fuse)
    net, b, P, batch, av, am, A, M = _setup(V, C, vpa, H, L, S, mode)
    _forward_backward_check(net, b, P, batch, av, am, L, mode, f"small {path} fuse={fuse} V={V} H={H} L={L} mode={mode}")


def _forward_backward_check(net, b, P, batch, av, am, L, mode, label):
    """Logits, value and every parameter gradient (random cotangents) of the device network on batch b against
    the float64 oracle on `batch`, at the bars of the module docstring.  Returns (report, norm, (logits, value)):
    report = [(tensor, err / fp32-oracle err)], worst first; norm = the worst err / bound (1.0 = at the bar) of
    the normwise and of the elementwise bars, over the outputs and over the gradients."""
    args = (batch["svf"], batch["x"], batch["cf"], batch["A_pos"], batch["A_neg"])
    onet.RELU_LOG = log = []
    try:
        ref_logits = onet.actor_logits(P, L, *args, av, am, mode)
        ref_value = onet.critic(P, L, *args)
    finally:
        onet.RELU_LOG = None
    logits, value, state = net.forward(b, save=True)
    rl, rv = ref_logits.detach().numpy(), ref_value.detach().numpy()
    norm = {"outputs": max(_norm_ratio(logits.cpu().numpy(), rl, 1e-5), _norm_ratio(value.cpu().numpy(), rv, 1e-5)),
            "gradients": 0.0}
    _close_norm(logits.cpu().numpy(), rl, 1e-5, "logits")
    _close_norm(value.cpu().numpy(), rv, 1e-5, "value")
    # random cotangents
    g = torch.Generator().manual_seed(3)
    wl = torch.randn(ref_logits.shape, generator=g, dtype=torch.float64)
    wl = torch.where(torch.isfinite(ref_logits), wl, torch.zeros_like(wl))
    wv = torch.randn(ref_value.shape, generator=g, dtype=torch.float64)
    obj = (torch.where(torch.isfinite(ref_logits), ref_logits, torch.zeros_like(ref_logits)) * wl).sum() + \
        (ref_value * wv).sum()
    kink, _ = onet.kink_bound(obj, P, log)
    obj.backward()
    # the elementwise bar of the depth tests as well: |err| <= 1e-5 |ref| + factor x the fp32 CPU oracle's error
    y_l, y_v, y_g = _fp32_yardstick(P, L, args, av, am, mode, wl, wv)
    report, elem = [], {}
    _close_yard(logits.cpu().numpy(), rl, y_l, FWD_FACTOR, "logits", report, worst=elem)
    _close_yard(value.cpu().numpy(), rv, y_v, FWD_FACTOR, "value", report, worst=elem)
    norm["elementwise outputs"] = max(elem.values())
    net.grads.zero_()
    net.backward(b, state, wl.float().cuda().contiguous(), wv.float().cuda().contiguous())
    got = net.to_flax(grads=True)
    for name, p in P.items():
        ref = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
        scale = max(np.abs(ref).max(), 1e-12)
        norm["gradients"] = max(norm["gradients"], _norm_ratio(got[name], ref, 1e-4))
        _close(got[name], ref, 0.0, 1e-4 * scale, f"grad {name}")
        _close_yard(got[name], ref, y_g[name], GRAD_FACTOR, f"grad {name}", report, kink[name], worst=elem)
    norm["elementwise gradients"] = max(v for k, v in elem.items() if k.startswith("grad"))
    report.sort(key=lambda t: -t[1])
    print(f"{label}: err / fp32-oracle err, worst", [(w, round(r, 2)) for w, r in report[:4]],
          "worst err / bound", {k: round(v, 3) for k, v in norm.items()})
    return report, norm, (logits, value)


def _norm_ratio(dev, ref, rtol):
    """max |dev - ref| over (rtol x max |ref|) on the finite elements of ref: 1.0 = at the normwise bar."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref) & np.isfinite(dev)
    if not fin.any():
        return 0.0
    return float(np.abs(dev[fin] - ref[fin]).max() / (rtol * max(np.abs(ref[fin]).max(), 1e-12)))


DEPTH_CASES = [  # the reference's depth (MAPPO_CONFIG.yaml:23-24: H = 128, L = 16)
    (50, 218, 10, 128, 16, 4, 0),  # uf50-218, 5 agents (BASELINE config 2)
    (100, 430, 10, 128, 16, 2, 0),  # uf100-430, 10 agents (config 3)
    (23, 97, 10, 128, 16, 3, 1),  # mode 1, agents of 8, 8, 7 vars: a padded slot
]


# elementwise bar of the depth tests: |err| <= 1e-5 |ref| + factor x E32 (E32 = the largest error of the
# same oracle run in float32 on the CPU).  Measured on MI355X (profiles/r03_parity_depth.txt): forward
# outputs <= FWD ratio, gradients up to ~3.9 x on the device fp32 path itself (two independent fp32
# summation orders: the elementwise maximum of one can exceed the other's by that much)
FWD_FACTOR = 2.0
GRAD_FACTOR = 4.0


def _fp32_yardstick(P, L, args, av, am, mode, wl, wv):
    """The same oracle evaluated in float32 on the CPU: the reference's own arithmetic class.  Returns
    its logits, value and parameter gradients for the cotangents (wl, wv)."""
    P32 = {k: v.detach().float().requires_grad_(True) for k, v in P.items()}
    a32 = tuple(a.float() for a in args)
    lg = onet.actor_logits(P32, L, *a32, av, am, mode)
    v = onet.critic(P32, L, *a32)
    obj = (torch.where(torch.isfinite(lg), lg, torch.zeros_like(lg)) * wl.float()).sum() + (v * wv.float()).sum()
    obj.backward()
    grads = {k: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape, np.float32)) for k, p in P32.items()}
    return lg.detach().numpy(), v.detach().numpy(), grads


def _close_yard(dev, ref, yard, factor, what, report, kink=None, worst=None):
    """|dev - ref| <= 1e-5 |ref| + factor * max|yard - ref| (+ kink) elementwise (yard: the fp32 CPU
    oracle; kink: oracle.net.kink_bound's allowance for ReLU inputs within fp32 noise of 0).  worst: a dict that
    receives, under `what`, the largest err / bound over the elements (1.0 = at the bar)."""
    dev, ref, yard = (np.asarray(a, np.float64) for a in (dev, ref, yard))
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(dev)), what + " (inf pattern)"
    e32 = np.abs(yard[fin] - ref[fin]).max() if fin.any() else 0.0
    err = np.abs(dev[fin] - ref[fin])
    extra = np.zeros_like(ref) if kink is None else np.asarray(kink, np.float64)
    plain = extra[fin] == 0  # the ratio is reported over the elements without a ReLU-kink allowance
    report.append((what, float(err[plain].max() / max(e32, 1e-300)) if plain.any() else 0.0))
    bound = 1e-5 * np.abs(ref[fin]) + factor * e32 + extra[fin]
    if worst is not None:
        worst[what] = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), f"{what}: max err {err.max():.3g}, worst ratio {(err / bound).max():.3g}"


def _set_path(monkeypatch, path, c_precision):
    """'default': the bench's kernels (phi folded, fp16x2 GRU forward / data / weight gradients with
    dual launches); 'bf16x3': phi folded, the fp16x2 kernels off (the bf16x3 register-A GRU forward,
    bf16x3 data and weight gradients: the fallback wherever fp16's range fails; MARLSAT_PRECISION=bf16x3);
    'fp32': the reference operation order on fp32 MFMA kernels (MARLSAT_PRECISION=fp32 + FUSE_PHI=0);
    a key of SINGLE_SWITCH: 'default' with that one switch off (its kernels' fp32-accurate fallback)."""
    from marlsat.learners.gnn import GNNActorCritic

    fast = path != "fp32"
    monkeypatch.setattr(GNNActorCritic, "fuse_phi", fast)
    monkeypatch.setattr(GNNActorCritic, "use_x3", fast)
    monkeypatch.setattr(GNNActorCritic, "use_gru_x3", fast)
    h2 = path == "default" or path in SINGLE_SWITCH
    for sw in ("use_gru_h2", "use_dgrad_h2", "use_wgrad_h2"):
        monkeypatch.setattr(GNNActorCritic, sw, h2)
    for sw, v in SINGLE_SWITCH.get(path, {}).items():
        monkeypatch.setattr(GNNActorCritic, sw, v)
    # the C-side weight-gradient choice (gemm.hip, msat_set_precision): it follows use_wgrad_h2
    c_precision({"bf16x3": "bf16x3", "fp32": "fp32", "wgrad_x3": "bf16x3"}.get(path, "fp16x2"))


@pytest.mark.parametrize("path", ["default", "bf16x3", "fp32"])
@pytest.mark.parametrize("V,C,vpa,H,L,S,mode", DEPTH_CASES)
def test_depth16_matches_oracle(V, C, vpa, H, L, S, mode, path, monkeypatch, c_precision):
    """The reference's depth L = 16 at H = 128 on uf50 / uf100 / mode 1, on the kernels the bench
    runs ("default": phi folded, fp16x2 GRU forward and data / weight gradients, dual launches), on
    the bf16x3 path those kernels fall back to, and on the reference-order fp32 path, against the
    float64 oracle.

    Bar: normwise 1e-5 (max |err| <= 1e-5 max |ref| per tensor) AND elementwise
    |err| <= 1e-5 |ref| + atol, atol = FWD_FACTOR (forward) / GRAD_FACTOR (gradients) x the largest error of the same
    oracle run in float32 on the CPU.  A pure elementwise 1e-5 relative bar is beyond fp32 itself:
    the float32 oracle misses it on 1-5 % of the logits at these depths (profiles/archive_r02/probe_parity_depth.py,
    profiles/r02_parity_depth.txt), so the fp32 rounding of the reference's own arithmetic is the
    yardstick for the elements near zero.  Gradients also allow oracle.net.kink_bound: a ReLU input
    within 3e-5 (relative) of 0 may land on either side in fp32, and the two sides' gradients
    differ by a whole term (profiles/archive_r02/probe_head_bisect.py: one flipped flip-head unit moved its bias
    gradient by 5e-3)."""
    _set_path(monkeypatch, path, c_precision)
    _depth_check(V, C, vpa, H, L, S, mode, path)


# BASELINE config 4's network: uf200-860, VARS_PER_AGENT 8 -> 25 agents of m = 8, one sample (the
# float64 oracle runs 25 dense masked per-agent encoders of 200 x 860 at the reference depth)
UF200_CASE = (200, 860, 8, 128, 16, 1, 0)


@pytest.mark.parametrize("path", ["default", "fp32"])
def test_uf200_network_matches_oracle(path, monkeypatch, c_precision):
    """Config 4 (uf200, A = 25, m = 8) at H = 128, L = 16 against the float64 oracle, same bar as
    test_depth16_matches_oracle."""
    _set_path(monkeypatch, path, c_precision)
    _depth_check(*UF200_CASE, path)


def _depth_check(V, C, vpa, H, L, S, mode, path):
    net, b, P, batch, av, am, A, M = _setup(V, C, vpa, H, L, S, mode, seed=11)
    args = (batch["svf"], batch["x"], batch["cf"], batch["A_pos"], batch["A_neg"])
    onet.RELU_LOG = log = []
    try:
        ref_l = onet.actor_logits(P, L, *args, av, am, mode)
        ref_v = onet.critic(P, L, *args)
    finally:
        onet.RELU_LOG = None
    g = torch.Generator().manual_seed(5)
    wl = torch.randn(ref_l.shape, generator=g, dtype=torch.float64)
    wl = torch.where(torch.isfinite(ref_l), wl, torch.zeros_like(wl))
    wv = torch.randn(ref_v.shape, generator=g, dtype=torch.float64)
    obj = (torch.where(torch.isfinite(ref_l), ref_l, torch.zeros_like(ref_l)) * wl).sum() + (ref_v * wv).sum()
    kink, n_kink = onet.kink_bound(obj, P, log)
    obj.backward()
    y_l, y_v, y_g = _fp32_yardstick(P, L, args, av, am, mode, wl, wv)
    logits, value, state = net.forward(b, save=True)
    rl, rv = ref_l.detach().numpy(), ref_v.detach().numpy()
    report = []
    _close_norm(logits.cpu().numpy(), rl, 1e-5, "logits")
    _close_norm(value.cpu().numpy(), rv, 1e-5, "value")
    _close_yard(logits.cpu().numpy(), rl, y_l, FWD_FACTOR, "logits", report)
    _close_yard(value.cpu().numpy(), rv, y_v, FWD_FACTOR, "value", report)
    net.grads.zero_()
    net.backward(b, state, wl.float().cuda().contiguous(), wv.float().cuda().contiguous())
    got = net.to_flax(grads=True)
    for name, p in P.items():
        ref = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
        _close_yard(got[name], ref, y_g[name], GRAD_FACTOR, f"grad {name}", report, kink[name])
    fwd = {w: round(r, 2) for w, r in report[:2]}
    report.sort(key=lambda t: -t[1])
    print(f"depth16 {path} V={V} mode={mode}: {n_kink} ReLU inputs within 3e-5 of 0; err / fp32-oracle err: "
          f"forward {fwd}; worst gradients", [(w, round(r, 2)) for w, r in report[:5] if w.startswith("grad")])


def test_critic_only_batch_matches_full():
    from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates

    net, b, P, batch, av, am, A, M = _setup(20, 91, 10, 64, 2, 4, 0)
    _, v_full, _ = net.forward(b)
    # rebuild the same samples as a critic-only batch
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool
    from marlsat import SATEnv

    pool = generate_problem_pool(20, 91, 4, size_id=7)
    env = SATEnv(20, 91, 10, vars_per_agent=10)
    dpool = env.make_pool(pool)
    tpl = DeviceTemplates(build_templates(pool, 20, env.num_agents), env.num_agents, "cuda")
    rng = np.random.default_rng(0)
    inst = rng.integers(0, 4, 4).astype(np.int32)
    x = rng.integers(0, 2, (4, 20)).astype(np.uint8)
    bc = assemble(tpl, dpool.packed, dpool.static_var_features(), torch.from_numpy(inst).cuda(),
                  torch.from_numpy(x).cuda(), critic_only=True)
    _, v_crit, _ = net.forward(bc, actor=False)
    assert torch.equal(v_full, v_crit)


@pytest.mark.parametrize("mode,padded,pool", [(0, False, None), (1, False, None), (0, True, None),
                                              (0, True, "quirks23"), (1, True, "quirks23")],
                         ids=["0", "1", "0-padded", "0-quirks23", "1-quirks23"])
def test_ppo_loss_and_grads_match_oracle(mode, padded, pool):
    """pool: a pool of tests/irregular_pools.py in place of the generated instances (quirks23: literal 0, repeated
    variables, a variable in no clause, an agent whose graph has no clause row; agents of 8, 8 and 7)."""
    from marlsat import _lib

    V, C, vpa, H, L, S = (20, 91, 10, 64, 2, 6) if mode == 0 else (16, 60, 4, 64, 2, 6)
    if padded:  # agents of 8, 8 and 7 variables: masked lanes in the loss, a -inf logit column, zeroed my_emb slots
        V, C = 23, 97
    kw = {}
    if pool is not None:
        import irregular_pools

        ir = irregular_pools.get(pool)
        V, C, vpa, S = ir.V, ir.C, ir.vpa, len(ir.inst)
        kw = dict(pool=ir.pool, inst=ir.inst, x=ir.x)
    net, b, P, batch, av, am, A, M = _setup(V, C, vpa, H, L, S, mode, seed=5, **kw)
    assert padded == (not bool(am.all()))
    cfg = {"CLIP_EPS": 0.12, "VF_CLIP": 0.5, "ENT_COEF": 0.005, "VF_COEF": 0.5}
    rng = np.random.default_rng(9)
    with torch.no_grad():
        lg = onet.actor_logits(P, L, batch["svf"], batch["x"], batch["cf"], batch["A_pos"], batch["A_neg"], av, am, mode)
        vv = onet.critic(P, L, batch["svf"], batch["x"], batch["cf"], batch["A_pos"], batch["A_neg"])
        probs = torch.softmax(onet._live_rows(lg), -1)  # a padded mode-1 slot (both logits -inf) draws either action
        act = torch.distributions.Categorical(probs=probs).sample(generator=None) if False else \
            torch.multinomial(probs.reshape(-1, probs.shape[-1]), 1, generator=torch.Generator().manual_seed(1)) \
            .reshape(probs.shape[:-1])
        lp = torch.log_softmax(lg, -1).gather(-1, act[..., None])[..., 0]
    old_lp = lp + torch.from_numpy(rng.normal(0, 0.1, lp.shape))  # ratios both inside and outside the clip range
    if mode == 1:
        old_lp = torch.where(torch.isfinite(lp), old_lp, torch.zeros_like(old_lp))
    bt = dict(batch, action=act, log_prob=old_lp, gae=torch.from_numpy(rng.normal(0, 1, S)),
              value=vv + torch.from_numpy(rng.normal(0, 0.4, S)), targets=vv + torch.from_numpy(rng.normal(0, 1, S)))
    total, (vl, la, ent), _, _ = onet.ppo_loss(P, L, bt, cfg, av, am, mode)
    total.backward()
    logits, value, state = net.forward(b, save=True)
    dlog = torch.empty_like(logits)
    dval = torch.empty_like(value)
    R = S * A
    rows = torch.empty(2 * R + S, device="cuda")
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    cu = lambda t, dt=torch.float32: t.to(dt).contiguous().cuda()
    # keep every device temporary referenced until the kernel has run (a tensor freed before the
    # launch is enqueued can be handed to the next allocation and overwritten first)
    d_act, d_olp, d_gae = cu(act, torch.int32), cu(old_lp), cu(bt["gae"])
    d_vold, d_tgt = cu(bt["value"]), cu(bt["targets"])
    assert int(d_act.min()) >= 0 and int(d_act.max()) < (M + 1 if mode == 0 else 2)
    _lib.check(_lib.lib.msat_ppo_loss(
        logits.data_ptr(), S, A, M, mode, net.base, net.rem, d_act.data_ptr(), d_olp.data_ptr(),
        d_gae.data_ptr(), value.data_ptr(), d_vold.data_ptr(), d_tgt.data_ptr(),
        cfg["CLIP_EPS"], cfg["VF_CLIP"], cfg["ENT_COEF"], cfg["VF_COEF"], S, dlog.data_ptr(), dval.data_ptr(),
        rows.data_ptr(), sums.data_ptr(), _lib.stream_ptr()), "ppo_loss")
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    n_act = S * A
    n_ent = S * A if mode == 0 else S * A * M
    np.testing.assert_allclose(s[0] / S, float(vl), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(s[1] / n_act, float(la), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(s[2] / n_ent, float(ent), rtol=1e-5, atol=1e-7)
    net.grads.zero_()
    net.backward(b, state, dlog, dval)
    got = net.to_flax(grads=True)
    for name, p in P.items():
        ref = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
        scale = max(np.abs(ref).max(), 1e-12)
        _close(got[name], ref, 0.0, 2e-4 * scale, f"grad {name}")


def test_adam_matches_optax_formula():
    from marlsat.learners.gnn import GNNActorCritic
    from oracle.net import adam_update

    net = GNNActorCritic(64, 1, 2, 10, 0, 20, device="cuda")
    p0 = net.params.clone()
    g = torch.randn_like(net.params)
    state = {"count": 0, "m": {"p": torch.zeros(net.size, dtype=torch.float64)},
             "v": {"p": torch.zeros(net.size, dtype=torch.float64)}}
    pr = {"p": p0.double().cpu()}
    for step in range(3):
        net.grads.copy_(g * (step + 1))
        net.adam_step(1e-3 * (step + 1))
        pr, state = adam_update(pr, {"p": (g * (step + 1)).double().cpu()}, state, 1e-3 * (step + 1))
    np.testing.assert_allclose(net.params.cpu().numpy(), pr["p"].numpy(), rtol=1e-5, atol=1e-6)


def test_fused_encoder_matches_reference_order_uf50():
    """BASELINE MAPPO sizes (uf50-218, H=128, L=16): the phi-folded encoder against the
    reference-order encoder on the same batch (both fp32 on the device)."""
    from marlsat.learners.gnn import GNNActorCritic

    net, b, P, batch, av, am, A, M = _setup(50, 218, 10, 128, 16, 6, 0, seed=2)
    out = {}
    for fuse in (False, True):
        GNNActorCritic.fuse_phi = fuse
        try:
            logits, value, state = net.forward(b, save=True)
            g = torch.Generator(device="cuda").manual_seed(4)
            dl = torch.where(torch.isfinite(logits), torch.randn(logits.shape, device="cuda", generator=g),
                             torch.zeros_like(logits)).contiguous()
            dv = torch.randn(value.shape, device="cuda", generator=g).contiguous()
            net.grads.zero_()
            net.backward(b, state, dl, dv)
            out[fuse] = (logits.clone(), value.clone(), net.to_flax(grads=True))
        finally:
            GNNActorCritic.fuse_phi = True
    (l0, v0, g0), (l1, v1, g1) = out[False], out[True]
    _close_norm(l1.cpu().numpy(), l0.cpu().numpy(), 1e-5, "logits")
    _close_norm(v1.cpu().numpy(), v0.cpu().numpy(), 1e-5, "value")
    for name in g0:
        scale = max(np.abs(g0[name]).max(), 1e-12)
        _close(g1[name], g0[name], 0.0, 1e-4 * scale, f"grad {name}")


def test_gathers_and_degree_features():
    """msat_clause_gather2 (split / merged) and msat_var_gather2 with distinct pos / neg sources
    against dense incidence products, and the assembled count features (vfeat[:, 4:6], cdeg)."""
    net, b, P, batch, av, am, A, M = _setup(20, 91, 10, 64, 2, 5, 0)
    _check_gathers(b)


def _check_gathers(b):
    from marlsat import _lib

    H, Nv, Nc = 64, b.Nv, b.Nc
    slots = b.slots.cpu().numpy()
    Ap = np.zeros((Nv, Nc))
    An = np.zeros((Nv, Nc))
    for c in range(Nc):
        for sl in slots[c]:
            if sl >= 0:
                (An if sl & 1 else Ap)[sl >> 1, c] += 1
    np.testing.assert_array_equal(b.vfeat[:, 4].cpu().numpy(), Ap.sum(1))
    np.testing.assert_array_equal(b.vfeat[:, 5].cpu().numpy(), An.sum(1))
    np.testing.assert_array_equal(b.cdeg[:, 0].cpu().numpy(), Ap.sum(0))
    np.testing.assert_array_equal(b.cdeg[:, 1].cpu().numpy(), An.sum(0))
    assert float(b.vfeat[:, 6:].abs().max()) == 0 and float(b.cdeg[:, 2:].abs().max()) == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    Xp, Xn = (torch.randn(Nv, H, device="cuda", generator=g) for _ in range(2))
    Yp, Yn = (torch.randn(Nc, H, device="cuda", generator=g) for _ in range(2))
    s = _lib.stream_ptr()
    d = lambda t: t.double().cpu().numpy()
    G = torch.empty(Nc, 2 * H, device="cuda")
    _lib.check(_lib.lib.msat_clause_gather2(Xp.data_ptr(), Xn.data_ptr(), H, b.slots.data_ptr(), G.data_ptr(), 2 * H,
                                            Nc, H, 0, 0, s), "clause_gather2")
    np.testing.assert_allclose(d(G), np.concatenate([Ap.T @ d(Xp), An.T @ d(Xn)], 1), rtol=1e-6, atol=1e-5)
    Gm = torch.randn(Nc, H, device="cuda", generator=g)
    Gm0 = Gm.clone()
    _lib.check(_lib.lib.msat_clause_gather2(Xp.data_ptr(), Xn.data_ptr(), H, b.slots.data_ptr(), Gm.data_ptr(), H,
                                            Nc, H, 1, 1, s), "clause_gather2 merged")
    np.testing.assert_allclose(d(Gm), d(Gm0) + Ap.T @ d(Xp) + An.T @ d(Xn), rtol=1e-6, atol=1e-5)
    Vp, Vn = torch.randn(Nv, H, device="cuda", generator=g), torch.randn(Nv, H, device="cuda", generator=g)
    Vp0, Vn0 = Vp.clone(), Vn.clone()
    _lib.check(_lib.lib.msat_var_gather2(Yp.data_ptr(), Yn.data_ptr(), H, b.ptr.data_ptr(), b.inc.data_ptr(),
                                         Vp.data_ptr(), Vn.data_ptr(), H, Nv, H, 1, s), "var_gather2")
    np.testing.assert_allclose(d(Vp), d(Vp0) + Ap @ d(Yp), rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(d(Vn), d(Vn0) + An @ d(Yn), rtol=1e-6, atol=1e-5)
