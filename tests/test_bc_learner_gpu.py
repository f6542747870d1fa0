"""GPU: behavioural-cloning training on the device (learners/bc_learner.BCLearner and the runner) against the
float64 oracle: greedy labels, every Adam step's loss / gradient / update, micro-batching, the short last
minibatch, the invalid-label error, a decreasing loss, and the runner end to end (checkpoint -> inject_bc).

Bars: the loss 1e-5 relative; gradients 1e-4 normwise and elementwise 1e-5 |ref| + GRAD_FACTOR x E32 + kink
(E32: the same oracle in float32 on the CPU; tests/test_gnn_gpu.py); the Adam step against oracle.net.adam_update
in float64 on the device's own gradient (tests/test_mappo_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import net as onet
from oracle.sat_env import OracleSATEnv
from oracle.single_env import compute_joint_labels_parallel_greedy as oracle_labels

pytestmark = pytest.mark.gpu

GRAD_FACTOR = 4.0  # tests/test_gnn_gpu.py
SHAPES = [  # V, C, vars_per_agent, H, L
    (12, 40, 4, 64, 2),
    (23, 97, 10, 64, 2),  # agents of 8, 8 and 7 variables: a padded slot, a -inf logit
    (20, 91, 10, 128, 2),
]


@pytest.fixture
def precision_path(request):
    """One precision path for the test (gnn.set_precision), the process's own restored afterwards."""
    from marlsat.learners import gnn

    prev = gnn.set_precision(request.param)
    yield request.param
    gnn.restore_precision(prev)


def _cfg(H, L, MB, lr=3e-3, **kw):
    return dict(MINIBATCH_SIZE=MB, LEARNING_RATE=lr, ANNEAL_LR=True, NUM_UPDATES=10, GNN_HIDDEN_DIM=H,
                GNN_NUM_MESSAGE_PASSING_STEPS=L, action_mode=0, **kw)


_DATA = {}


def _dataset(V, C, vpa, n_problems=4, per=2, level=3, pool=None):
    """Planted problems, corrupted planted solutions and their oracle labels (host; computed once per shape).
    pool: the name of a pool of tests/irregular_pools.py whose first n_problems instances are the problems (the
    planted assignments of other instances are then merely the points that get corrupted)."""
    from marlsat.runners.behavioral_cloning import corrupt
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses, generate_sat_solution, has_isolated_variable

    if (V, C, vpa, pool) in _DATA:
        return _DATA[(V, C, vpa, pool)]
    clauses, sols, seed = [], [], 7000
    if pool is not None:
        import irregular_pools

        ir = irregular_pools.get(pool)
        assert (ir.V, ir.C) == (V, C) and not any(has_isolated_variable(cl[cl != 0], V) for cl in ir.pool)
        clauses = list(ir.pool[:n_problems])
        sols = [generate_sat_solution(V, seed + i) for i in range(n_problems)]
    while len(clauses) < n_problems:
        cl = generate_sat_clauses(V, C, seed=seed)
        if not has_isolated_variable(cl, V):
            clauses.append(cl)
            sols.append(generate_sat_solution(V, seed))
        seed += 1
    clauses, sols = np.stack(clauses), np.stack(sols)
    x = corrupt(sols, per, level, seed=5)
    pidx = np.repeat(np.arange(n_problems, dtype=np.int32), per)
    ora = OracleSATEnv(V, C, 4, vars_per_agent=vpa)
    labels = np.stack([oracle_labels(ora, clauses[p], x[i].astype(np.int32), 0.0) for i, p in enumerate(pidx)])
    _DATA[(V, C, vpa, pool)] = (clauses, pidx, x, labels, ora)
    return _DATA[(V, C, vpa, pool)]


def _learner(V, C, vpa, H, L, MB, n=None, micro_bytes=None, seed=4, lr=3e-3, pool=None):
    from marlsat import SATEnv
    from marlsat.learners.bc_learner import BCLearner
    from marlsat.learners.gnn import GNNActorCritic

    clauses, pidx, x, labels, ora = _dataset(V, C, vpa, pool=pool)
    n = len(pidx) if n is None else n
    env = SATEnv(V, C, max_steps=4, vars_per_agent=vpa)
    net = GNNActorCritic(H, L, env.num_agents, env.max_vars_per_agent, 0, V, device="cuda", seed=seed)
    learner = BCLearner(_cfg(H, L, MB, lr), env, net, env.make_pool(clauses), micro_bytes=micro_bytes)
    learner.set_data(pidx[:n], x[:n], labels[:n])
    return learner, net, env


def _unflat(net, flat_params):
    from marlsat.learners import params as Pm

    return Pm.to_flax(flat_params.detach().cpu().numpy(), net.H, net.L, net.A, net.M, net.mode, net.E)


def _oracle_batch(V, C, vpa, rows, pool=None):
    clauses, pidx, x, labels, ora = _dataset(V, C, vpa, pool=pool)
    p, xx = pidx[rows], x[rows]
    _, ost = ora.reset(clauses[p], xx.astype(np.int32))
    Ap, An = onet.dense_graph(clauses[p], V)
    args = (torch.from_numpy(ora.static_var_features(clauses[p])).double(), torch.from_numpy(xx.astype(np.float64)),
            torch.from_numpy(ora.clause_features(ost)).double(), Ap, An)
    av = torch.from_numpy(ora.agent_vars.astype(np.int64))
    am = torch.from_numpy(ora.action_mask)
    return args, av, am, torch.from_numpy(labels[rows]).long()


def _oracle_loss(P, L, args, av, am, lab, dtype):
    """-mean(log_softmax(actor_logits)[labels]) (behavioral_cloning.py:243-256) with parameters P."""
    lg = onet.actor_logits(P, L, *(a.to(dtype) for a in args), av, am, 0)
    return -onet.log_softmax(lg).gather(-1, lab[..., None])[..., 0].mean()


def _yard_close(dev, ref, yard, what, extra, failures):
    """Both gradient bars for one tensor; a miss is appended to ``failures`` (asserted once per trace, so that one
    run reports every step and tensor)."""
    dev, ref, yard = (np.asarray(a, np.float64) for a in (dev, ref, yard))
    assert np.isfinite(dev).all(), what
    err = np.abs(dev - ref)
    scale = max(np.abs(ref).max(), 1e-12)
    e32 = np.abs(yard - ref).max()
    bound = 1e-5 * np.abs(ref) + GRAD_FACTOR * e32 + np.asarray(extra, np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    if err.max() > 0.5e-4 * scale or worst > 0.5:  # the figures of every tensor past half a bar, before asserting
        print(f"  {what}: max err {err.max():.3g}, max |ref| {scale:.3g} (normwise {err.max() / scale:.3g}), fp32 oracle "
              f"err {e32:.3g}, elementwise ratio {worst:.3g}")
    if err.max() > 1e-4 * scale:
        failures.append(f"{what}: normwise {err.max():.3g} / {scale:.3g} = {err.max() / scale:.3g} > 1e-4")
    if not (err <= bound).all():
        failures.append(f"{what}: elementwise max err {err.max():.3g}, worst ratio {worst:.3g}")
    return worst


def _check_trace(learner, net, shape, tag, pool=None):
    """Every recorded Adam step against the float64 oracle at the recorded parameters."""
    V, C, vpa, H, L = shape
    trace = learner.trace
    assert len(trace) == len(learner.minibatch_losses)
    m = v = None
    failures = []
    for s, rec in enumerate(trace):
        rows = rec["idx"].numpy().astype(np.int64)
        args, av, am, lab = _oracle_batch(V, C, vpa, rows, pool=pool)
        P_s = _unflat(net, rec["params"])
        P64 = {k: torch.tensor(a, dtype=torch.float64, requires_grad=True) for k, a in P_s.items()}
        onet.RELU_LOG = log = []
        try:
            loss64 = _oracle_loss(P64, L, args, av, am, lab, torch.float64)
        finally:
            onet.RELU_LOG = None
        kink, _ = onet.kink_bound(loss64, P64, log)
        loss64.backward()
        P32 = {k: torch.tensor(a, dtype=torch.float32, requires_grad=True) for k, a in P_s.items()}
        _oracle_loss(P32, L, args, av, am, lab, torch.float32).backward()
        ref_l, dev_l = float(loss64.detach()), float(learner.minibatch_losses[s])
        assert abs(dev_l - ref_l) <= 1e-5 * abs(ref_l), f"{tag} step {s}: loss {dev_l} vs {ref_l}"
        g_dev = _unflat(net, rec["grads"])
        worst = ("", 0.0)
        for k, p in P64.items():
            g64 = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
            g32 = P32[k].grad.double().numpy() if P32[k].grad is not None else np.zeros(p.shape)
            if k.startswith("critic"):
                assert not g64.any() and not np.asarray(g_dev[k]).any(), f"{tag} step {s}: critic gradient {k}"
                continue
            r = _yard_close(g_dev[k], g64, g32, f"{tag} step {s} grad {k}", kink[k], failures)
            worst = max(worst, (k, r), key=lambda t: t[1])
        print(f"{tag} step {s}: rows {rows.tolist()}, loss err / |loss| {abs(dev_l - ref_l) / abs(ref_l):.3g}, "
              f"worst gradient ratio {worst[1]:.3g} ({worst[0]})")
        # optax.adam in float64 on the device's own gradient
        g = rec["grads"].double().cpu()
        if m is None:
            m, v = torch.zeros_like(g), torch.zeros_like(g)
        pr, st = onet.adam_update({"p": rec["params"].double().cpu()}, {"p": g},
                                  {"count": s, "m": {"p": m}, "v": {"p": v}}, rec["lr"])
        m, v = st["m"]["p"], st["v"]["p"]
        nxt = trace[s + 1]["params"] if s + 1 < len(trace) else net.params
        np.testing.assert_allclose(nxt.double().cpu().numpy(), pr["p"].numpy(), rtol=1e-5, atol=1e-7,
                                   err_msg=f"{tag} Adam step {s}")
        assert rec["lr"] == 3e-3  # the constant LEARNING_RATE: ANNEAL_LR is ignored
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("V,C,vpa,H,L", SHAPES)
def test_device_labels_equal_oracle_labels(V, C, vpa, H, L):
    from marlsat import SATEnv
    from marlsat.runners.behavioral_cloning import compute_joint_labels

    clauses, pidx, x, labels, ora = _dataset(V, C, vpa)
    env = SATEnv(V, C, max_steps=4, vars_per_agent=vpa)
    got = compute_joint_labels(env, env.make_pool(clauses), pidx, x, 0.0).cpu().numpy()
    assert np.array_equal(got, labels)
    assert (labels != env.max_vars_per_agent).any()  # corrupted solutions: some agent has an improving flip


@pytest.mark.parametrize("precision_path", ["fp16x2", "bf16x3", "fp32"], indirect=True)
@pytest.mark.parametrize("V,C,vpa,H,L", SHAPES)
def test_every_adam_step_matches_oracle(V, C, vpa, H, L, precision_path):
    """N = 7 samples in minibatches of 3: three Adam steps, the last on a single sample whose mean is over its
    own size.  The critic receives no gradient and does not move.

    Closest to a bar, measured on an MI355X: the one-sample step of (20, 91, 10, 128, 2) on fp16x2, the one-element
    actor_flip_head_output/bias gradient (5.6e-4, a sum of softmax residuals of 0.5 that cancel): 4.0e-8 off,
    0.72 of the 1e-4 normwise bar, where the float32 CPU oracle is 4.9e-8 off.  msat_bc_loss evaluates its softmax in
    fp64 for this element (2.8e-7 off with the PPO kernels' fp32 logsumexp).  Every other tensor,
    step, shape and path is below 0.65 of either bar."""
    learner, net, env = _learner(V, C, vpa, H, L, MB=3, n=7)
    learner.trace = []
    p0 = net.to_flax()
    out = learner.train_epoch(torch.Generator().manual_seed(7))
    assert [len(r["idx"]) for r in learner.trace] == [3, 3, 1]
    assert sorted(torch.cat([r["idx"] for r in learner.trace]).tolist()) == list(range(7))
    assert out["loss"] == pytest.approx(float(np.mean(learner.minibatch_losses)), rel=1e-12)
    assert 0.0 <= out["accuracy"] <= 1.0
    _check_trace(learner, net, (V, C, vpa, H, L), f"{precision_path} V{V} H{H}")
    p1 = net.to_flax()
    critic = [k for k in p0 if k.startswith("critic")]
    assert critic and len(critic) < len(p0)
    bits = lambda a: np.asarray(a, np.float32).view(np.int32)
    for k in critic:
        assert np.array_equal(bits(p0[k]), bits(p1[k])), k
    moved = [k for k in p0 if not np.array_equal(bits(p0[k]), bits(p1[k]))]
    assert {k.split("/")[0].split("_")[0] for k in moved} >= {"encoder", "actor", "agent"}


def test_every_adam_step_matches_oracle_on_an_irregular_pool():
    """The same three Adam steps on the 2-wide pool of tests/irregular_pools.learner_pool: literal 0, [v, v] and
    [v, -v] rows (the labels are the oracle's greedy ones on those clauses).  The network starts from zero biases,
    so the pool has no variable outside every clause."""
    from marlsat import SATEnv
    from marlsat.runners.behavioral_cloning import compute_joint_labels

    V, C, vpa, H, L = 12, 40, 4, 64, 2
    clauses, pidx, x, labels, ora = _dataset(V, C, vpa, pool="learner")
    assert clauses.shape == (4, C, 2) and (clauses[1] == 0).any()
    env = SATEnv(V, C, max_steps=4, vars_per_agent=vpa)
    got = compute_joint_labels(env, env.make_pool(clauses), pidx, x, 0.0).cpu().numpy()
    assert np.array_equal(got, labels) and (labels != env.max_vars_per_agent).any()
    learner, net, env = _learner(V, C, vpa, H, L, MB=3, n=7, pool="learner")
    learner.trace = []
    learner.train_epoch(torch.Generator().manual_seed(7))
    assert [len(r["idx"]) for r in learner.trace] == [3, 3, 1]
    _check_trace(learner, net, (V, C, vpa, H, L), "irregular V12 H64", pool="learner")


def test_micro_batches_meet_the_same_bars():
    """An activation budget of 2 samples: minibatches of 4 and 3 run as micro-batches of 2 + 2 and 2 + 1."""
    shape = SHAPES[1]
    V, C, vpa, H, L = shape
    probe, _, _ = _learner(V, C, vpa, H, L, MB=4, n=7)
    assert probe.micro == 4
    rows = probe.tpl.mean_full_rows
    from marlsat.learners.base import activation_bytes_per_sample

    budget = 2.5 * activation_bytes_per_sample(rows, H, L)
    learner, net, env = _learner(V, C, vpa, H, L, MB=4, n=7, micro_bytes=budget)
    assert learner.micro == 2
    learner.trace = []
    learner.train_epoch(torch.Generator().manual_seed(8))
    assert [len(r["idx"]) for r in learner.trace] == [4, 3]
    _check_trace(learner, net, shape, "micro")


def test_label_at_masked_slot_raises():
    V, C, vpa, H, L = SHAPES[1]
    learner, net, env = _learner(V, C, vpa, H, L, MB=4)
    lab = learner.data["labels"].clone()
    assert env.max_vars_per_agent == 8 and env.num_agents == 3
    lab[5, 2] = 7  # the third agent owns 7 variables: slot 7 is padded (-inf)
    learner.set_data(learner.data["pidx"], learner.data["x"], lab)
    with pytest.raises(ValueError, match=r"1 label\(s\).*masked"):
        learner.train_epoch(torch.Generator().manual_seed(1))
    lab[5, 2] = 9  # beyond the no-op
    learner.set_data(learner.data["pidx"], learner.data["x"], lab)
    with pytest.raises(ValueError, match="out-of-range"):
        learner.train_epoch(torch.Generator().manual_seed(1))


def test_loss_decreases_as_the_oracles_does():
    """Full-batch epochs (N = MINIBATCH_SIZE: one Adam step per epoch, whatever the permutation).  The float64
    oracle, taking its own Adam steps on the CPU, must end strictly below its starting loss for this seed and step
    count; then so must the device."""
    V, C, vpa, H, L = SHAPES[0]
    n, epochs, lr, seed = 6, 4, 3e-3, 4
    learner, net, env = _learner(V, C, vpa, H, L, MB=n, n=n, seed=seed, lr=lr)
    args, av, am, lab = _oracle_batch(V, C, vpa, np.arange(n))
    params = {k: torch.tensor(a, dtype=torch.float64) for k, a in net.to_flax().items()}
    state = {"count": 0, "m": {k: torch.zeros_like(p) for k, p in params.items()},
             "v": {k: torch.zeros_like(p) for k, p in params.items()}}
    ref = []
    for _ in range(epochs):
        Pk = {k: p.clone().requires_grad_(True) for k, p in params.items()}
        loss = _oracle_loss(Pk, L, args, av, am, lab, torch.float64)
        loss.backward()
        ref.append(float(loss.detach()))
        grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in Pk.items()}
        params, state = onet.adam_update(params, grads, state, lr)
    assert ref[-1] < ref[0], ref
    gen = torch.Generator().manual_seed(2)
    dev = [learner.train_epoch(gen)["loss"] for _ in range(epochs)]
    print(f"loss per epoch: oracle {ref}, device {dev}")
    assert dev[-1] < dev[0], (dev, ref)
    assert dev[0] == pytest.approx(ref[0], rel=1e-5)


def test_runner_end_to_end(tmp_path):
    """run(): 2 epochs on 8 generated uf20-91 problems with planted .sol files; the written bc_model_2 injects
    into a fresh network (encoder, actor, embedding = the trained ones bitwise; critic = the fresh init); both logs
    parse in the reference's formats and every line marked solved carries a valid solution."""
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.runners import behavioral_cloning as bcr
    from marlsat.utils import checkpoints as ck
    from marlsat.utils.data_parser import parse_cnf
    from marlsat.utils.generate_cnf_dataset import generate_cnf_dataset_sat

    V, C = 20, 91
    cnf, sol, save = (str(tmp_path / d) for d in ("cnf", "sol", "bc"))
    generate_cnf_dataset_sat(8, V, C, cnf, seed=1, sol_dir=sol)
    config = {
        "SEED": 3, "CNF_DATA_DIR": cnf,
        "environment": {"NUM_VARS": V, "NUM_CLAUSES": C, "MAX_STEPS": 8, "VARS_PER_AGENT": 10, "action_mode": 0},
        "network": {"GNN_HIDDEN_DIM": 64, "GNN_NUM_MESSAGE_PASSING_STEPS": 2},
        "training": {"NUM_UPDATES": 2, "MINIBATCH_SIZE": 16, "LEARNING_RATE": 1e-3, "NUM_ENVS": 4, "NUM_STEPS": 2},
        "bc_training": {"MODE": "parallel_joint", "NUM_SAMPLES_PER_EXPERT": 5, "CORRUPTION_LEVEL": 3,
                        "SOL_DATA_DIR": sol, "SAVE_PATH": save},
    }
    lines = []
    res = bcr.run(config, log=lines.append)
    assert res["num_samples"] == 40 and res["samples_per_second"] > 0
    assert any("solved" in l for l in lines) and any("samples/s" in l for l in lines)
    # the checkpoint
    trained = res["network"].to_flax()
    st = ck.restore_checkpoint(save, "bc_model_", None)
    assert st is not None and os.path.exists(os.path.join(save, "bc_model_2")) and set(st) == {"params"}
    fresh = GNNActorCritic(64, 2, 2, 10, 0, V, device="cuda", seed=99)
    init = {k: a.copy() for k, a in fresh.to_flax().items()}
    ck.inject_bc(fresh, st)
    after = fresh.to_flax()
    kinds = set()
    for k in trained:
        bits = lambda a: np.asarray(a, np.float32).view(np.int32)
        if k.startswith("critic"):
            assert np.array_equal(bits(after[k]), bits(init[k])), k
            assert not np.array_equal(bits(init[k]), bits(trained[k])) or not init[k].any(), k
            kinds.add("critic")
        else:
            assert k.startswith("encoder") or "actor" in k or "agent_id_embedding" in k, k
            assert np.array_equal(bits(after[k]), bits(trained[k])), k
            kinds.add(k.split("/")[0].split("_")[0])
    assert {"critic", "encoder", "actor", "agent"} <= kinds
    # bc_training_log.txt: epoch,loss with epoch + 1 and a .6f loss
    log = open(os.path.join(save, "bc_training_log.txt")).read().splitlines()
    assert log[0] == "epoch,loss" and len(log) == 3
    for e, line in enumerate(log[1:]):
        ep, loss = line.split(",")
        assert int(ep) == e + 1 and len(loss.split(".")[1]) == 6 and float(loss) > 0
    assert float(log[2].split(",")[1]) == pytest.approx(res["last_epoch"]["loss"], abs=1e-6)
    # solver_solutions_log.txt
    sl = open(os.path.join(save, "solver_solutions_log.txt")).read().splitlines()
    assert sl[0] + "\n" == bcr.SOLVER_LOG_HEADER and len(sl) == 9
    n_solved = 0
    for line, name in zip(sl[1:], sorted(os.listdir(cnf))):
        f = line.split(", ")
        assert len(f) == 5 and f[0] == name and f[1] in ("True", "False") and f[3] in ("True", "False")
        assert 1 <= int(f[2]) <= 8
        if f[1] == "True":
            n_solved += 1
            assert f[3] == "True" and len(f[4]) == V and set(f[4]) <= {"0", "1"}
            _, _, cl = parse_cnf(os.path.join(cnf, name))
            x = np.array([int(c) for c in f[4]], dtype=np.int32)
            _, nun = OracleSATEnv.satisfaction(x[None], np.asarray(cl, dtype=np.int32)[None])
            assert int(nun[0]) == 0, name
        else:
            assert f[3] == "False" and f[4] == "N/A" and int(f[2]) == 8
    assert res["solve_rate"] == pytest.approx(n_solved / 8)
