"""GPU: the single-agent PPO learner (learners/single_ppo_learner.SinglePPOLearner) against the oracles.

* Rollout replay: the recorded actions through oracle.single_env.OracleSatEnv with oracle.rng.reset_draws for every
  reset -- rewards bitwise, done / solved / stored (instance, assignment) exact, and the time-out at the reference's
  step (the pre-increment rule of sat_env.py:106), not one early.
* Every Adam step of one cycle from ``trace``: the minibatch's normalised advantages, the loss terms (1e-5 relative;
  the policy term relative to the mean magnitude of its rows, see _check_cycle),
  the gradient before the clip (_yard_close of tests/test_bc_learner_gpu.py, restated in tests/test_single_gnn_gpu.py;
  the output bias' gradient, exactly 0 by the softmax's shift invariance, against its rounding bound instead),
  the norm and the clipped gradient given the device's own gradient (the bars of tests/test_clip_global_norm_gpu.py),
  the Adam update with eps 1e-5 against oracle.net.adam_update in float64 on the device's gradient (rtol 1e-5,
  atol 1e-7), and the learning rate of every step.
* evaluate: (solved, length, return) against a NumPy replay of the recorded greedy actions."""
import numpy as np
import pytest
import torch

import single_oracle as so
from oracle import mappo as om
from oracle import net as onet
from oracle.rng import reset_draws
from oracle.sat_env import OracleSATEnv
from oracle.single_env import OracleSatEnv
from test_single_gnn_gpu import _yard_close

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
C_BONUS = 2.5
SHAPES = [(12, 40, 64, 2), (20, 91, 128, 2)]  # V, C, H, L: the first and third shape of tests/test_single_gnn_gpu.py


@pytest.fixture
def precision_path(request):
    from marlsat.learners import gnn

    prev = gnn.set_precision(request.param)
    yield request.param
    gnn.restore_precision(prev)


def _cfg(B, T, K=2, E=2, cycles=1, **kw):
    c = dict(NUM_ENVS=B, NUM_STEPS=T, NUM_MINIBATCHES=K, UPDATE_EPOCHS=E, NUM_CYCLES=cycles, LR=3e-3, ANNEAL_LR=True,
             GAMMA=0.99, GAE_LAMBDA=0.95, CLIP_EPS=0.2, VF_COEF=0.5, ENT_COEF=0.01)
    c.update(kw)
    return c


_POOLS = {}


def _pool(V, C, N=4):
    from marlsat.utils.generate_cnf_dataset import generate_problem_pool

    if (V, C, N) not in _POOLS:
        _POOLS[(V, C, N)] = generate_problem_pool(V, C, N, size_id=11, skip_isolated=True)
    return _POOLS[(V, C, N)]


def _learner(V, C, H, L, cfg, max_steps, micro_bytes=None, seed=4):
    from marlsat.learners.single_gnn import GNNSingleActorCritic
    from marlsat.learners.single_ppo_learner import SinglePPOLearner, make_single_env

    pool = _pool(V, C)
    env = make_single_env(V, C, max_steps, C_BONUS)
    net = GNNSingleActorCritic(H, L, V, device="cuda", seed=seed)
    return SinglePPOLearner(cfg, env, net, env.make_pool(pool), micro_bytes=micro_bytes), net, pool


def _replay(learner, pool, V, C, max_steps):
    """The rollout's transitions through the oracle env; returns the number of (time-out, solved) dones."""
    tr = {k: v.cpu().numpy() for k, v in learner.tr.items()}
    T, B = tr["reward"].shape
    N = pool.shape[0]
    resets = [r for r in learner.trace if r["kind"] == "reset"]
    steps = [r for r in learner.trace if r["kind"] == "step"]
    assert len(resets) == 1 and [r["t"] for r in steps] == list(range(T))
    ora = OracleSatEnv(V, C, 3, c_bonus=C_BONUS, max_steps=max_steps)
    pidx, x = reset_draws(resets[0]["key"].seed, resets[0]["key"].counter, B, V, N)
    ost = ora.reset(pool[pidx], x.astype(np.int32))
    timeouts = solves = 0
    for t in range(T):
        np.testing.assert_array_equal(tr["pidx"][t], pidx, err_msg=f"t={t} instance")
        np.testing.assert_array_equal(tr["x"][t], ost["x"], err_msg=f"t={t} assignment")
        assert ((tr["action"][t] >= 0) & (tr["action"][t] < V)).all()
        step0 = ost["step"].copy()
        ost, r, d = ora.step(ost, tr["action"][t])
        solved = ost["u"] == np.float32(0.0)
        assert np.array_equal(tr["reward"][t].view(np.int32), r.view(np.int32)), f"t={t} reward"
        np.testing.assert_array_equal(tr["done"][t] != 0, d, err_msg=f"t={t} done")
        np.testing.assert_array_equal(tr["solved"][t] != 0, solved, err_msg=f"t={t} solved")
        # the pre-increment rule: an unsolved env is done on the step it takes at step count max_steps, not before
        np.testing.assert_array_equal(d & ~solved, (step0 >= max_steps) & ~solved, err_msg=f"t={t} time-out")
        timeouts += int((d & ~solved).sum())
        solves += int(solved.sum())
        key = steps[t]["key"]
        npidx, nx = reset_draws(key.seed, key.counter, B, V, N)  # the auto-reset's draws, used where done
        pidx = np.where(d, npidx, pidx).astype(np.int32)
        fresh = ora.reset(pool[npidx], nx.astype(np.int32))
        ost = {"x": np.where(d[:, None], fresh["x"], ost["x"]), "step": np.where(d, fresh["step"], ost["step"]),
               "u": np.where(d, fresh["u"], ost["u"]), "clauses": pool[pidx]}
    return timeouts, solves, pidx, ost


def test_rollout_replays_through_the_oracle_env():
    from marlsat.random import PRNGKey

    V, C, H, L = SHAPES[0]
    B, T, max_steps = 4, 5, 2
    learner, net, pool = _learner(V, C, H, L, _cfg(B, T, K=2), max_steps)
    learner.trace = []
    rs = learner.rollout(learner.init_runner_state(PRNGKey(3)))
    assert rs.env_state.reset_queue is None
    timeouts, solves, pidx, ost = _replay(learner, pool, V, C, max_steps)
    print(f"rollout replay: {timeouts} time-outs, {solves} solved steps")
    # T = 5 > max_steps + 1: every env that is not solved first times out on its third step and is reset
    assert timeouts >= 1
    done = learner.tr["done"].cpu().numpy() != 0
    solved = learner.tr["solved"].cpu().numpy() != 0
    assert not (done[:max_steps] & ~solved[:max_steps]).any() and (done[max_steps] | solved[:max_steps].any(0)).all()
    # the state the rollout left is the oracle's
    np.testing.assert_array_equal(rs.env_state.problem_idx.cpu().numpy(), pidx)
    np.testing.assert_array_equal(rs.env_state.variable_assignments.cpu().numpy(), ost["x"])
    np.testing.assert_array_equal(rs.env_state.step.cpu().numpy(), ost["step"])
    stats = learner.rollout_stats()
    assert stats["train_ep_num"] == int(done.sum()) + B
    assert stats["train_solve_rate"] == pytest.approx(float((done & solved).sum()) / (int(done.sum()) + B))


def _oracle_args(pool, V, C, pidx, x):
    ora = OracleSATEnv(V, C, 10, vars_per_agent=V)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    Ap, An = onet.dense_graph(pool[pidx], V)
    return (torch.from_numpy(ora.static_var_features(pool[pidx])).double(), torch.from_numpy(x.astype(np.float64)),
            torch.from_numpy(ora.clause_features(ost)).double(), Ap, An)


def _oracle_total(P, L, args, batch, cfg, dtype):
    to = lambda t: t.to(dtype) if t.is_floating_point() else t
    lg, val = so.single_forward(P, L, tuple(to(a) for a in args))
    terms = so.single_terms(lg, val, batch["action"], to(batch["old_logp"]), to(batch["adv"]), to(batch["targets"]),
                            float(np.float32(cfg["CLIP_EPS"])))
    MB = lg.shape[0]
    lg.retain_grad()  # d total / d logits, for the bound on the output bias' gradient (_check_cycle)
    return so.single_total(terms, float(np.float32(cfg["ENT_COEF"])), float(np.float32(cfg["VF_COEF"])), MB), terms, lg


def _check_cycle(learner, net, pool, shape, cfg, tag, count0=0):
    """Every recorded Adam step of the cycle against the oracles."""
    from marlsat.learners import params as Pm

    V, C, H, L = shape
    tr = {k: v.cpu().numpy() for k, v in learner.tr.items()}
    T, B = tr["reward"].shape
    N, MB = T * B, T * B // cfg["NUM_MINIBATCHES"]
    # GAE, not normalised: the oracle's scan on the device's own values, bitwise (tests/test_gae_gpu.py)
    oadv, otgt = om.gae(tr["reward"], tr["value"], tr["done"], learner.last_val.cpu().numpy(), cfg["GAMMA"],
                        cfg["GAE_LAMBDA"])
    adv, tgt = learner.adv.cpu().numpy(), learner.targets.cpu().numpy()
    np.testing.assert_array_equal(adv, oadv)
    np.testing.assert_array_equal(tgt, otgt)
    flat = lambda a: a.reshape((N,) + a.shape[2:])
    recs = [r for r in learner.trace if r["kind"] == "adam"]
    steps = cfg["UPDATE_EPOCHS"] * cfg["NUM_MINIBATCHES"]
    assert len(recs) == steps == len(learner.minibatch_terms) == len(learner.grad_norms)
    total_steps = cfg["NUM_CYCLES"] * steps
    for e in range(cfg["UPDATE_EPOCHS"]):  # every epoch is a permutation cut into equal minibatches
        rows = torch.cat([r["idx"] for r in recs[e * cfg["NUM_MINIBATCHES"]:(e + 1) * cfg["NUM_MINIBATCHES"]]])
        assert sorted(rows.tolist()) == list(range(N))
    m = v = None
    failures, clipped_steps = [], 0
    for s, rec in enumerate(recs):
        rows = rec["idx"].numpy().astype(np.int64)
        assert len(rows) == MB and rec["count"] == count0 + s
        # learning rate: the schedule at the Adam steps already taken
        want_lr = so.single_lr(count0 + s, cfg["LR"], cfg["ANNEAL_LR"], total_steps)
        assert rec["lr"] == want_lr, (s, rec["lr"], want_lr)
        # the minibatch's advantages, standardised over the whole minibatch
        adv_n = rec["adv_n"].cpu().numpy()
        ref_n = so.standardize_pop(flat(adv)[rows])
        assert np.abs(adv_n - ref_n).max() <= 2.0 ** -22 * np.abs(ref_n).max(), f"{tag} step {s}: advantages"
        # loss terms and the gradient before the clip, at the recorded parameters
        P_s = Pm.single_to_flax(rec["params"].cpu().numpy(), H, L)
        P64 = {k: torch.tensor(a, dtype=torch.float64, requires_grad=True) for k, a in P_s.items()}
        batch = {"action": torch.from_numpy(flat(tr["action"])[rows]), "old_logp": torch.from_numpy(
            flat(tr["log_prob"])[rows]).double(), "adv": torch.from_numpy(adv_n).double(),
            "targets": torch.from_numpy(flat(tgt)[rows]).double()}
        args = _oracle_args(pool, V, C, flat(tr["pidx"])[rows], flat(tr["x"])[rows])
        onet.RELU_LOG = log = []
        try:
            total64, terms, lg64 = _oracle_total(P64, L, args, batch, cfg, torch.float64)
        finally:
            onet.RELU_LOG = None
        kink, _ = onet.kink_bound(total64, P64, log)
        total64.backward()
        P32 = {k: torch.tensor(a, dtype=torch.float32, requires_grad=True) for k, a in P_s.items()}
        _oracle_total(P32, L, args, batch, cfg, torch.float32)[0].backward()
        ref_terms = np.array([float(t.detach().mean()) for t in terms[:3]])
        dev_terms = learner.minibatch_terms[s]
        # 1e-5 relative.  vl and ent are means of one-signed terms.  The policy term is not: at ratio 1 it is
        # -mean(adv_n), which the standardisation makes 0, so in the first epoch its exact value is the rounding of
        # the stored log-probabilities (1e-7 here) and "relative to itself" has no meaning for any fp32 pipeline;
        # its scale is the mean magnitude of the rows it averages.
        scale = np.array([float(terms[0].detach().abs().mean()), abs(ref_terms[1]), abs(ref_terms[2])])
        assert (np.abs(dev_terms - ref_terms) <= 1e-5 * scale).all(), \
            f"{tag} step {s}: terms {dev_terms} vs {ref_terms} (scales {scale})"
        ref_total = (ref_terms[0] + float(np.float32(cfg["VF_COEF"])) * ref_terms[1]
                     - float(np.float32(cfg["ENT_COEF"])) * ref_terms[2])  # the coefficients as the device gets them
        assert ref_total == pytest.approx(float(total64.detach()), rel=1e-12)
        near = so.near_kink(terms[3].detach().numpy(), cfg["CLIP_EPS"], np.ones(MB, bool), tol=1e-5)
        g_dev = Pm.single_to_flax(rec["grads"].cpu().numpy(), H, L)
        worst = ("", 0.0)
        for k, p in P64.items():
            g64 = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
            g32 = P32[k].grad.double().numpy() if P32[k].grad is not None else np.zeros(p.shape)
            if k == "actor_output/bias":
                # This bias adds one constant to every logit of a row and the loss sees the logits through their
                # softmax alone, so its exact gradient -- the sum of all dlogits -- is 0 (float64: 1e-17).  A bar
                # relative to that reference has no meaning; what the device holds is the sum of MB * V dlogits that
                # were each rounded to fp32 once (2^-24 |d| apiece), summed in fp32: within 2^-23 * sum |dlogits|.
                bound = 2.0 ** -23 * float(lg64.grad.abs().sum())
                assert np.abs(g64).max() <= 1e-12 * float(lg64.grad.abs().sum())
                if not np.abs(g_dev[k]).max() <= bound:
                    failures.append(f"{tag} step {s} grad {k}: |{np.abs(g_dev[k]).max():.3g}| > {bound:.3g}")
                continue
            r = _yard_close(g_dev[k], g64, g32, f"{tag} step {s} grad {k}", kink[k], failures)
            worst = max(worst, (k, r), key=lambda t: t[1])
        # the norm and the clip, given the device's own gradient
        g = rec["grads"].cpu().numpy()
        ref_c, ref_norm, touched = so.clip_global_norm(g, rec["max_norm"])
        norm = float(rec["norm"].item())
        assert abs(norm - ref_norm) <= ULP * ref_norm and learner.grad_norms[s] == np.float32(norm)
        assert abs(ref_norm - float(np.float32(rec["max_norm"]))) > 1e-6 * ref_norm  # the decision is not at the edge
        got_c = rec["clipped"].cpu().numpy()
        if touched:
            clipped_steps += 1
            assert (np.abs(got_c.astype(np.float64) - ref_c) <= ULP * np.abs(ref_c)).all(), f"{tag} step {s}: clip"
        else:
            assert np.array_equal(got_c.view(np.int32), g.view(np.int32)), f"{tag} step {s}: untouched gradient"
        terr = (np.abs(dev_terms - ref_terms) / scale).max()
        print(f"{tag} step {s}: lr {rec['lr']:.3g}, terms err / scale {terr:.2g}, norm "
              f"{norm:.4g} (max {rec['max_norm']:g}, clipped {touched}), worst gradient ratio {worst[1]:.3g} "
              f"({worst[0]}), rows near a clip edge {int(near.sum())}")
        # optax.adam(eps = 1e-5) in float64 on the device's own clipped gradient
        gc = rec["clipped"].double().cpu()
        if m is None:
            m, v = torch.zeros_like(gc), torch.zeros_like(gc)
        pr, st = onet.adam_update({"p": rec["params"].double().cpu()}, {"p": gc},
                                  {"count": count0 + s, "m": {"p": m}, "v": {"p": v}}, rec["lr"], eps=1e-5)
        m, v = st["m"]["p"], st["v"]["p"]
        nxt = recs[s + 1]["params"] if s + 1 < len(recs) else net.params
        np.testing.assert_allclose(nxt.double().cpu().numpy(), pr["p"].numpy(), rtol=1e-5, atol=1e-7,
                                   err_msg=f"{tag} Adam step {s}")
        if rec["lr"] == 0.0:  # past the schedule's end: the parameters stay, bit for bit
            assert torch.equal(nxt.view(torch.int32), rec["params"].view(torch.int32))
    assert not failures, "\n".join(failures)
    return clipped_steps, steps


CYCLES = [  # shape, precision path, MAX_GRAD_NORM, Adam steps taken before the cycle
    (0, "fp16x2", 1e-3, 0),  # tiny: the clip is active in every step
    (0, "fp32", 1e6, 2),  # huge: never active; counts 2..5 of 4: the schedule's end and past it (lr = 0)
    (1, "fp16x2", None, 0),  # the reference's 1.0 under ANNEAL_LR
    (1, "fp32", None, 0),
]


@pytest.mark.parametrize("shape_no,precision_path,max_norm,count0", CYCLES,
                         indirect=["precision_path"], ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in CYCLES])
def test_every_adam_step_of_a_cycle_matches_oracle(shape_no, precision_path, max_norm, count0):
    from marlsat.random import PRNGKey

    shape = SHAPES[shape_no]
    V, C, H, L = shape
    cfg = _cfg(4, 3, K=2, E=2, MAX_GRAD_NORM=max_norm)
    learner, net, pool = _learner(V, C, H, L, cfg, max_steps=6)
    assert learner.MB == 6 and learner.micro == 6
    net.adam_count = count0
    learner.trace = []
    rs, stats = learner.train_cycle(learner.init_runner_state(PRNGKey(5)), torch.Generator().manual_seed(7))
    assert net.adam_count == count0 + 4
    clipped, steps = _check_cycle(learner, net, pool, shape, cfg, f"{precision_path} V{V} H{H}", count0)
    if max_norm == 1e-3:
        assert clipped == steps
    if max_norm == 1e6:
        assert clipped == 0
        assert [r["lr"] for r in learner.trace if r["kind"] == "adam"] == [3e-3 * 0.5, 3e-3 * 0.25, 0.0, 0.0]
    t = learner.minibatch_terms
    assert stats["loss_policy"] == pytest.approx(t[:, 0].mean()) and stats["entropy"] == pytest.approx(t[:, 2].mean())
    assert stats["loss_total"] == pytest.approx((t[:, 0] + 0.5 * t[:, 1] - 0.01 * t[:, 2]).mean())
    assert 0.0 < stats["entropy"] <= np.log(V) + 1e-6


def test_micro_batches_meet_the_same_bars():
    """An activation budget of 2 samples: minibatches of 6 run as micro-batches of 2 + 2 + 2."""
    from marlsat.learners import gnn
    from marlsat.learners.base import activation_bytes_per_sample
    from marlsat.random import PRNGKey

    prev = gnn.set_precision("fp16x2")
    try:
        shape = SHAPES[0]
        V, C, H, L = shape
        cfg = _cfg(4, 3, K=2, E=2)
        probe, _, _ = _learner(V, C, H, L, cfg, max_steps=6)
        rows = probe.tpl.mean_full_rows - probe.tpl.mean_actor_rows
        assert rows == V + C
        budget = 2.5 * activation_bytes_per_sample(rows, H, L)
        learner, net, pool = _learner(V, C, H, L, cfg, max_steps=6, micro_bytes=budget)
        assert learner.micro == 2
        learner.trace = []
        learner.train_cycle(learner.init_runner_state(PRNGKey(5)), torch.Generator().manual_seed(7))
        _check_cycle(learner, net, pool, shape, cfg, "micro")
    finally:
        gnn.restore_precision(prev)


def test_indivisible_minibatches_and_a_foreign_env_raise():
    from marlsat import SATEnv
    from marlsat.learners.single_gnn import GNNSingleActorCritic
    from marlsat.learners.single_ppo_learner import SinglePPOLearner

    V, C, H, L = SHAPES[0]
    with pytest.raises(ValueError, match="divisible"):
        _learner(V, C, H, L, _cfg(4, 3, K=5), max_steps=6)
    env = SATEnv(V, C, 6, vars_per_agent=4)
    with pytest.raises(ValueError, match="single-agent"):
        SinglePPOLearner(_cfg(4, 3), env, GNNSingleActorCritic(H, L, V, device="cuda"), env.make_pool(_pool(V, C)))


@pytest.mark.parametrize("env_max_steps,early_exit", [(4, True), (2, False), (2, True)])
def test_evaluate_matches_a_numpy_replay(env_max_steps, early_exit):
    """3 instances from planted solutions with one variable flipped, 4 greedy steps.  With the env's own limit at 2
    every env has finished on its third step: the fourth (early_exit=False) changes nothing."""
    from marlsat.envs.multi_agent_sat_env import ProblemPool
    from marlsat.learners.single_gnn import GNNSingleActorCritic
    from marlsat.learners.single_ppo_learner import SinglePPOLearner, make_single_env
    from marlsat.random import PRNGKey

    V, C, H, L = SHAPES[0]
    n, max_steps = 3, 4
    env = make_single_env(V, C, env_max_steps, C_BONUS)
    dpool = ProblemPool.generate(env, n, PRNGKey(21))
    pool = dpool.clauses.cpu().numpy()
    x0 = dpool.planted.cpu().numpy().copy()
    x0[np.arange(n), [1, 5, 9]] ^= 1
    net = GNNSingleActorCritic(H, L, V, device="cuda", seed=2)
    learner = SinglePPOLearner(_cfg(n, 1, K=1, E=1), env, net, dpool)
    rec = []
    out = learner.evaluate(np.arange(n), max_steps, key=PRNGKey(1), assignments=x0, record=rec, early_exit=early_exit)
    ora = OracleSatEnv(V, C, 3, c_bonus=C_BONUS, max_steps=env_max_steps)
    ost = ora.reset(pool, x0.astype(np.int32))
    rews, dones, solveds = [], [], []
    for t, (a, r, d, sv) in enumerate(rec):
        ost, orr, od = ora.step(ost, a)
        assert np.array_equal(r.view(np.int32), orr.view(np.int32)) and np.array_equal(d != 0, od), t
        np.testing.assert_array_equal(sv != 0, ost["u"] == np.float32(0.0))
        rews.append(orr), dones.append(od), solveds.append(sv != 0)
    ret, ln, sv, fin = so.episode_track(np.stack(rews), np.stack(dones), np.stack(solveds))
    ln = np.where(fin != 0, ln, max_steps)
    ep = learner.eval_episodes
    assert np.array_equal(ep["return"].view(np.int32), ret.view(np.int32))
    np.testing.assert_array_equal(ep["len"], ln)
    np.testing.assert_array_equal(ep["solved"], sv)
    np.testing.assert_array_equal(ep["finished"], fin)
    assert out == {"eval_solve_rate": pytest.approx(float(sv.mean())), "eval_avg_len": pytest.approx(float(ln.mean())),
                   "eval_avg_return": pytest.approx(float(ret.mean()), rel=1e-6), "eval_episodes": n}
    print(f"evaluate env limit {env_max_steps}: {len(rec)} steps, lengths {ln.tolist()}, solved {sv.tolist()}")
    if env_max_steps == 2:
        assert fin.all() and (ln <= 3).all()
        assert len(rec) == (max(ln) if early_exit else max_steps)
        if not early_exit:  # a step after every env had finished: rewards flowed, nothing was counted
            assert len(rec) == 4 and np.abs(rec[3][1]).max() > 0
    else:
        assert len(rec) <= max_steps and (ln[fin == 0] == max_steps).all()
