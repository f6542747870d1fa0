"""GPU: the assignment predictor's learner (learners/assign_learner.AssignLearner) against the oracles: one epoch
over N = 5 uf20-91 samples in minibatches of 2 (a short last one), every Adam step from ``trace``.

Bars, those of tests/test_single_ppo_learner_gpu.py: each step's loss 1e-5 relative to the float64 oracle at the
traced parameters, its gradient by _yard_close (tests/test_single_gnn_gpu.py), the update against
oracle.net.adam_update in float64 on the device's own gradient (rtol 1e-5, atol 1e-7; eps 1e-8 here)."""
import numpy as np
import pytest
import torch

import assign_oracle as ao
from oracle import net as onet
from test_single_gnn_gpu import _yard_close

pytestmark = pytest.mark.gpu

V, C, H, L = 20, 91, 64, 2
N, MB = 5, 2
LR = 1e-3


def _data():
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses, generate_sat_solution

    seeds = [9100 + i for i in range(4)]
    pool = np.stack([generate_sat_clauses(V, C, 3, s) for s in seeds])
    sols = np.stack([generate_sat_solution(V, s) for s in seeds]).astype(np.uint8)
    pidx = np.array([0, 1, 2, 3, 1], np.int32)  # an instance twice, under two inputs
    rng = np.random.default_rng(2)
    x = np.zeros((N, V), np.uint8)
    x[3:] = rng.integers(0, 2, (2, V))
    return pool, pidx, x, sols[pidx]


def _learner(micro_bytes=None, seed=4):
    from marlsat import SATEnv
    from marlsat.learners.assign_gnn import GNNAssignmentPredictor
    from marlsat.learners.assign_learner import AssignLearner

    pool, pidx, x, lab = _data()
    env = SATEnv(V, C, max_steps=4, vars_per_agent=V)
    net = GNNAssignmentPredictor(H, L, device="cuda", seed=seed)
    lr = AssignLearner(dict(BATCH_SIZE=MB, LEARNING_RATE=LR), net, env.make_pool(pool), micro_bytes=micro_bytes)
    lr.set_data(pidx, x, lab)
    return lr, net, env, (pool, pidx, x, lab)


def _oracle_loss(P, args, lab, dtype):
    to = lambda t: t.to(dtype) if t.is_floating_point() else t
    lg = ao.assign_logits(P, L, *(to(a) for a in args))
    return ao.assign_loss(lg, torch.from_numpy(lab.astype(np.int64)), lg.shape[0]), lg


def _check_epoch(learner, net, env, data, stats, tag):
    from marlsat.learners import params as Pm

    pool, pidx, x, lab = data
    recs = learner.trace
    assert [len(r["idx"]) for r in recs] == [2, 2, 1]
    assert sorted(torch.cat([r["idx"] for r in recs]).tolist()) == list(range(N))
    m = v = None
    failures, losses, accs, solved_all = [], [], [], []
    for s, rec in enumerate(recs):
        rows = rec["idx"].numpy().astype(np.int64)
        assert rec["lr"] == LR
        P_s = Pm.assign_to_flax(rec["params"].cpu().numpy(), H, L)
        P64 = {k: torch.tensor(a, dtype=torch.float64, requires_grad=True) for k, a in P_s.items()}
        args = ao.graph_args(pool, pidx[rows], x[rows], V, C)
        onet.RELU_LOG = log = []
        try:
            total64, lg64 = _oracle_loss(P64, args, lab[rows], torch.float64)
        finally:
            onet.RELU_LOG = None
        kink, _ = onet.kink_bound(total64, P64, log)
        total64.backward()
        P32 = {k: torch.tensor(a, dtype=torch.float32, requires_grad=True) for k, a in P_s.items()}
        _oracle_loss(P32, args, lab[rows], torch.float32)[0].backward()
        ref_loss = float(total64.detach())
        dev_loss = float(learner.minibatch_losses[s])
        assert abs(dev_loss - ref_loss) <= 1e-5 * abs(ref_loss), f"{tag} step {s}: loss {dev_loss} vs {ref_loss}"
        g_dev = Pm.assign_to_flax(rec["grads"].cpu().numpy(), H, L)
        worst = ("", 0.0)
        for k, p in P64.items():
            g64 = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
            g32 = P32[k].grad.double().numpy() if P32[k].grad is not None else np.zeros(p.shape)
            r = _yard_close(g_dev[k], g64, g32, f"{tag} step {s} grad {k}", kink[k], failures)
            worst = max(worst, (k, r), key=lambda t: t[1])
        # the prediction is the traced parameters' (before the update); away from ties it is the oracle's arg-max
        l = lg64.detach().numpy()
        pred = rec["pred"].numpy()
        clear = np.abs(l[..., 1] - l[..., 0]) > 1e-4 * np.abs(l).max()
        assert np.array_equal(pred[clear], (l[..., 1] > l[..., 0]).astype(np.uint8)[clear]) and clear.mean() > 0.9
        _, nun = env._calculate_satisfaction_explicit(pred, pool[pidx[rows]])
        assert np.array_equal(rec["solved"].numpy() != 0, nun.cpu().numpy() == 0), f"{tag} step {s}: solved flags"
        solved_all.append(rec["solved"].numpy())
        losses.append(dev_loss)
        accs.append(float((pred == lab[rows]).mean()))
        print(f"{tag} step {s}: loss {dev_loss:.6f} (oracle {ref_loss:.6f}), worst gradient ratio {worst[1]:.3g} "
              f"({worst[0]}), unsat {nun.cpu().numpy().tolist()}")
        # optax.adam (eps 1e-8) in float64 on the device's own gradient
        g = rec["grads"].double().cpu()
        if m is None:
            m, v = torch.zeros_like(g), torch.zeros_like(g)
        pr, st = onet.adam_update({"p": rec["params"].double().cpu()}, {"p": g},
                                  {"count": s, "m": {"p": m}, "v": {"p": v}}, LR, eps=1e-8)
        m, v = st["m"]["p"], st["v"]["p"]
        nxt = recs[s + 1]["params"] if s + 1 < len(recs) else net.params
        np.testing.assert_allclose(nxt.double().cpu().numpy(), pr["p"].numpy(), rtol=1e-5, atol=1e-7,
                                   err_msg=f"{tag} Adam step {s}")
    assert not failures, "\n".join(failures)
    # the epoch's figures: unweighted means of the minibatch means (the short one counts as much as the others)
    assert stats["loss"] == pytest.approx(np.mean(losses), rel=1e-12)
    assert stats["var_acc"] == pytest.approx(np.mean(accs), rel=1e-12)
    assert stats["sol_acc"] == pytest.approx(np.concatenate(solved_all).sum() / N)


@pytest.fixture
def precision_path(request):
    from marlsat.learners import gnn

    prev = gnn.set_precision(request.param)
    yield request.param
    gnn.restore_precision(prev)


@pytest.mark.parametrize("precision_path", ["fp16x2", "fp32"], indirect=True)
def test_every_adam_step_of_an_epoch_matches_oracle(precision_path):
    learner, net, env, data = _learner()
    assert learner.micro == MB
    learner.trace = []
    stats = learner.train_epoch(torch.Generator().manual_seed(7))
    assert net.adam_count == 3
    _check_epoch(learner, net, env, data, stats, precision_path)


def test_micro_batches_meet_the_same_bars():
    """An activation budget of one sample: minibatches of 2 run as two micro-batches."""
    from marlsat.learners import gnn
    from marlsat.learners.base import activation_bytes_per_sample

    prev = gnn.set_precision("fp16x2")
    try:
        rows = V + C
        budget = 1.5 * activation_bytes_per_sample(rows, H, L)
        learner, net, env, data = _learner(micro_bytes=budget)
        assert learner.micro == 1
        learner.trace = []
        stats = learner.train_epoch(torch.Generator().manual_seed(7))
        _check_epoch(learner, net, env, data, stats, "micro")
    finally:
        gnn.restore_precision(prev)


def test_evaluate_updates_nothing_and_predict_is_slab_independent():
    learner, net, env, (pool, pidx, x, lab) = _learner()
    before = net.params.clone()
    ev = learner.evaluate(np.arange(N))
    assert torch.equal(net.params.view(torch.int32), before.view(torch.int32)) and net.adam_count == 0
    assert len(learner.minibatch_losses) == 3 and ev["loss"] == pytest.approx(learner.minibatch_losses.mean())
    assert 0.0 <= ev["var_acc"] <= 1.0 and 0.0 <= ev["sol_acc"] <= 1.0
    one = learner.predict(pidx, x, slab=N)
    three = learner.predict(pidx, x, slab=2)
    for a, b in zip(one, three):
        assert torch.equal(a, b)
    pred, unsat, solved = (t.cpu().numpy() for t in one)
    _, nun = env._calculate_satisfaction_explicit(pred, pool[pidx])
    assert np.array_equal(unsat, nun.cpu().numpy()) and np.array_equal(solved != 0, unsat == 0)
    # evaluate's accuracy is of these predictions (same parameters)
    accs = [(pred[i:i + MB] == lab[i:i + MB]).mean() for i in range(0, N, MB)]
    assert ev["var_acc"] == pytest.approx(np.mean(accs))


def test_invalid_labels_raise_after_the_epoch():
    learner, net, env, (pool, pidx, x, lab) = _learner()
    bad = lab.copy()
    bad[2, 5] = 2
    bad[4, 0] = 7
    learner.set_data(pidx, x, bad)
    with pytest.raises(ValueError, match="2 .*invalid"):
        learner.train_epoch(torch.Generator().manual_seed(7))
    assert net.adam_count == 3  # after the epoch's read, as BCLearner
