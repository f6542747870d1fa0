"""CPU tests: the oracle against the reference's golden vectors + hand-built KATs."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import mappo as om
from oracle.rng import philox4x32_10, reset_draws
from oracle.sat_env import OracleSATEnv, create_agent_groups


def _golden():
    return np.load(os.path.join(GOLDEN, "clause_truth.npz"), allow_pickle=False)


def test_generator_matches_reference_bytes():
    from marlsat.utils.generate_cnf_dataset import generate_sat_cnf

    for r in json.load(open(os.path.join(GOLDEN, "generator.json"))):
        text = generate_sat_cnf(r["V"], r["C"], r["k"], seed=r["seed"])
        assert hashlib.sha256(text.encode()).hexdigest() == r["sha256"], (r["V"], r["C"], r["seed"])
        if "text" in r:
            assert text == r["text"]


@pytest.mark.parametrize("case", range(7))
def test_oracle_clause_truth_vs_reference_checkers(case):
    g = _golden()
    cl, xs = g[f"c{case}_clauses"], g[f"c{case}_x"]
    B = xs.shape[0]
    status, nun = OracleSATEnv.satisfaction(xs.astype(np.int32), np.broadcast_to(cl, (B,) + cl.shape))
    np.testing.assert_array_equal(status.astype(np.uint8), g[f"c{case}_clause_sat"])
    np.testing.assert_array_equal((nun == 0).astype(np.uint8), g[f"c{case}_formula_sat"])
    np.testing.assert_array_equal((nun == 0).astype(np.uint8), g[f"c{case}_verify"])


def test_oracle_quirk_literals_vs_reference_checker():
    # literal 0 is false; a repeated var behaves as one literal (check_sat.py:20-40)
    g = _golden()
    cl, xs = g["quirk_clauses"], g["quirk_x"]
    status, _ = OracleSATEnv.satisfaction(xs.astype(np.int32), np.broadcast_to(cl, (xs.shape[0],) + cl.shape))
    np.testing.assert_array_equal(status.astype(np.uint8), g["quirk_clause_sat"])


def test_agent_groups_partition():
    # env:296-312 explicit grouping and :313-338 auto grouping
    g = create_agent_groups(200, 8)
    assert len(g) == 25 and all(len(v) == 8 for v in g.values())
    g = create_agent_groups(50, 10)
    assert len(g) == 5
    g = create_agent_groups(35, 7)
    assert len(g) == 5
    g = create_agent_groups(23, 10)  # ceil(23/10)=3 agents: 8,8,7
    assert [len(v) for v in g.values()] == [8, 8, 7]
    g = create_agent_groups(200, None)  # factor 4 divides 200 -> 50 agents of 4
    assert len(g) == 50 and all(len(v) == 4 for v in g.values())
    g = create_agent_groups(21, None)  # 4 does not divide 21 -> max(2, int(sqrt(21)))=4 agents
    assert [len(v) for v in g.values()] == [6, 5, 5, 5]


def test_oracle_env_known_answer():
    """Hand-derived 6-var / 4-clause instance, 2 agents (vars 0-2, 3-5)."""
    env = OracleSATEnv(6, 4, max_steps=3, vars_per_agent=3)
    cl = np.array([[[1, -2, 3], [-1, 4, 5], [-4, -5, -6], [2, 6, -3]]], np.int32)
    x = np.array([[1, 0, 0, 0, 0, 0]], np.int32)
    obs, st = env.reset(cl, x)
    # clause truth: c0: 1 true -> sat; c1: -1 false, 4,5 false -> unsat; c2: sat; c3: -3 true -> sat
    np.testing.assert_array_equal(st.clauses_satisfied_status[0], [True, False, True, True])
    assert st.num_unsatisfied[0] == 1
    # agent 0 owns vars 0,1,2 -> related clauses: c0,c1,c3 ; agent 1: c1,c2,c3
    np.testing.assert_array_equal(st.agent_clause_masks[0], [[1, 1, -1, 1], [-1, 1, 1, 1]])
    # neighbours of agent 0: vars of c0,c1,c3 not own -> 3,4,5 ; agent 1: vars 0,1,2
    np.testing.assert_array_equal(st.agent_neighbor_masks[0], [[-1, -1, -1, 1, 1, 1], [1, 1, 1, -1, -1, -1]])
    exp0 = [1, 0, 0, -1, -1, -1] + [1, 0, -1, 1] + [-1, -1, -1, 0, 0, 0]
    exp1 = [-1, -1, -1, 0, 0, 0] + [-1, 0, 1, 1] + [1, 0, 0, -1, -1, -1]
    np.testing.assert_array_equal(obs[0], [exp0, exp1])
    # agent 1 flips var 3 (local idx 0) -> c1 sat, c2 still sat (-5) -> solved
    obs, st2, r, d, info = env.step(st, np.array([[3, 0]]))  # agent 0: action 3 == no-op
    assert st2.variable_assignments[0].tolist() == [1, 0, 0, 1, 0, 0]
    assert info["solved"][0] and d[0] and r[0] == 1.0 and info["episode_step"][0] == 1
    # timeout path: no-ops until max_steps
    obs, s, r, d, info = env.step(st, np.array([[3, 3]]))
    assert not d[0] and r[0] == 0.0
    obs, s, r, d, info = env.step(s, np.array([[3, 3]]))
    obs, s, r, d, info = env.step(s, np.array([[3, 3]]))
    assert d[0] and not info["solved"][0] and info["episode_step"][0] == 3


def test_oracle_flip_decode_edge_cases():
    env = OracleSATEnv(5, 2, max_steps=10, vars_per_agent=3)  # ceil(5/3)=2 agents: [0,1,2], [3,4]; M=3
    x = np.zeros((1, 5), np.int32)
    # agent 1 has 2 vars: action 2 (a padded slot) is a no-op, action 3 (== M) no-op
    assert env.decode_flips(x, np.array([[0, 2]])).tolist() == [[1, 0, 0, 0, 0]]
    assert env.decode_flips(x, np.array([[3, 1]])).tolist() == [[0, 0, 0, 0, 1]]
    # negative index: jnp normalises -1 -> M-1 = 2 (agent 0 var 2; agent 1 padded -> no flip)
    assert env.decode_flips(x, np.array([[-1, -1]])).tolist() == [[0, 0, 1, 0, 0]]


def test_oracle_mode1_integer_xor_semantics():
    """env:246-250: mode 1 XORs the raw action integer into the int32 assignment; env:135-144: a
    literal is true only for x == 1 (positive) or x == 0 (negative).  An action of 2 or -1 therefore
    leaves a value for which both polarities are false (the device facade refuses such actions)."""
    env = OracleSATEnv(4, 2, max_steps=10, vars_per_agent=2, action_mode=1)  # agents [0,1], [2,3]
    x = np.array([[0, 1, 1, 0]], np.int32)
    new = env.decode_flips(x, np.array([[[2, 1], [-1, 0]]]))
    assert new.tolist() == [[2, 0, -2, 0]]
    cl = np.array([[[1, -1, 3], [-3, 2, 4]]], np.int32)
    status, nun = OracleSATEnv.satisfaction(new, cl)
    assert status.tolist() == [[False, False]] and nun.tolist() == [2]


def test_oracle_pbrs_reward():
    env = OracleSATEnv(6, 4, max_steps=5, vars_per_agent=3, reward_mode=1, r_clause=0.25, r_sat=2.0, gamma=0.5)
    cl = np.array([[[1, -2, 3], [-1, 4, 5], [-4, -5, -6], [2, 6, -3]]], np.int32)
    _, st = env.reset(cl, np.array([[1, 0, 0, 0, 0, 0]], np.int32))
    _, _, r, _, _ = env.step(st, np.array([[3, 0]]))
    # u: 1 -> 0 ; r = 0.5*0 - (-1) + 0.25*1 + 2.0
    assert r[0] == np.float32(3.25)


def test_gae_oracle_matches_closed_form():
    T, B = 5, 3
    rng = np.random.default_rng(0)
    r = rng.standard_normal((T, B)).astype(np.float32)
    v = rng.standard_normal((T, B)).astype(np.float32)
    d = rng.integers(0, 2, (T, B)).astype(bool)
    lv = rng.standard_normal(B).astype(np.float32)
    adv, tgt = om.gae(r, v, d, lv, 0.99, 0.95)
    # float64 closed-form recursion
    a = np.zeros(B)
    nv = lv.astype(np.float64)
    for t in range(T - 1, -1, -1):
        nd = 1.0 - d[t]
        a = r[t] + 0.99 * nv * nd - v[t] + 0.99 * 0.95 * nd * a
        np.testing.assert_allclose(adv[t], a, rtol=1e-5, atol=1e-6)
        nv = v[t]
    np.testing.assert_allclose(tgt, adv + v)


def test_philox_known_answers():
    # Random123 philox4x32-10 KATs
    out = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(o) for o in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    out = philox4x32_10(f, f, f, f, f, f)
    assert [int(o) for o in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    out = philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(o) for o in out] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_reset_draws_statistics():
    pidx, x = reset_draws(seed=123, counter=7, num_envs=4096, num_vars=200, num_problems=10)
    assert pidx.min() >= 0 and pidx.max() < 10
    assert abs(np.bincount(pidx, minlength=10) / 4096 - 0.1).max() < 0.03
    assert abs(x.mean() - 0.5) < 0.01


# ------------------------------------------------------------ PPO loss oracle (oracle/net.py) ----
def _net_case(V, C, vpa, H, L, S, mode, seed=5):
    """Oracle-side set-up of tests/test_gnn_gpu.py::_setup (no device): parameters, batch, agent tables."""
    import torch

    from marlsat.utils.generate_cnf_dataset import generate_problem_pool
    from oracle import net as onet

    pool = generate_problem_pool(V, C, 4, size_id=7)
    ora = OracleSATEnv(V, C, 10, vars_per_agent=vpa)
    A, M = ora.agent_vars.shape
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, 4, S).astype(np.int32)
    x = rng.integers(0, 2, (S, V)).astype(np.uint8)
    _, ost = ora.reset(pool[inst], x.astype(np.int32))
    Ap, An = onet.dense_graph(pool[inst], V)
    batch = {"svf": torch.from_numpy(ora.static_var_features(pool[inst])).double(),
             "x": torch.from_numpy(x).double(), "cf": torch.from_numpy(ora.clause_features(ost)).double(),
             "A_pos": Ap, "A_neg": An}
    tree = onet.init_params(onet.param_shapes(H, L, A, M, mode), seed=seed + 1)
    P = {k: v.clone().requires_grad_(True) for k, v in tree.items()}
    av = torch.from_numpy(ora.agent_vars.astype(np.int64))
    am = torch.from_numpy(ora.action_mask)
    with torch.no_grad():
        lg = onet.actor_logits(P, L, batch["svf"], batch["x"], batch["cf"], Ap, An, av, am, mode)
        vv = onet.critic(P, L, batch["svf"], batch["x"], batch["cf"], Ap, An)
        probs = torch.softmax(torch.where(torch.isfinite(lg).any(-1, keepdim=True), lg, torch.zeros(())), -1)
        act = torch.multinomial(probs.reshape(-1, probs.shape[-1]), 1, generator=torch.Generator().manual_seed(1)) \
            .reshape(probs.shape[:-1])
        lp = onet.log_softmax(lg).gather(-1, act[..., None])[..., 0]
    old_lp = lp + torch.from_numpy(rng.normal(0, 0.1, lp.shape))
    if mode == 1:
        old_lp = torch.where(am[None].expand_as(lp), old_lp, torch.zeros_like(old_lp))
    bt = dict(batch, action=act, log_prob=old_lp, gae=torch.from_numpy(rng.normal(0, 1, S)),
              value=vv + torch.from_numpy(rng.normal(0, 0.4, S)), targets=vv + torch.from_numpy(rng.normal(0, 1, S)))
    return P, bt, av, am


def _ppo_loss_before_split(P, L, batch, cfg, agent_vars, action_mask, action_mode):
    """oracle.net.ppo_loss as it stood before ppo_terms: torch.clamp for both clips and the entropy
    selected by torch.where(p > 0, ...) (finite gradients only where no logit is -inf)."""
    import torch

    from oracle import net as onet

    svf, x, cf, A_pos, A_neg = batch["svf"], batch["x"], batch["cf"], batch["A_pos"], batch["A_neg"]
    logits = onet.actor_logits(P, L, svf, x, cf, A_pos, A_neg, agent_vars, action_mask, action_mode)
    value = onet.critic(P, L, svf, x, cf, A_pos, A_neg)
    lp = torch.gather(torch.log_softmax(logits, -1), -1, batch["action"].long()[..., None])[..., 0]
    gae = batch["gae"][:, None]
    if action_mode == 0:
        ratio = torch.exp(lp - batch["log_prob"])
    else:
        valid = action_mask[None].expand_as(lp)
        zero = torch.zeros((), dtype=lp.dtype)
        ratio = torch.exp(torch.where(valid, lp, zero).sum(-1) - torch.where(valid, batch["log_prob"], zero).sum(-1))
    eps = cfg["CLIP_EPS"]
    loss_actor = -torch.minimum(ratio * gae, torch.clamp(ratio, 1.0 - eps, 1.0 + eps) * gae).mean()
    lpa = torch.log_softmax(logits, -1)
    p = lpa.exp()
    ent = (-torch.where(p > 0, p * lpa, torch.zeros_like(p)).sum(-1)).mean()
    vold = batch["value"]
    vclip = vold + (value - vold).clamp(-cfg["VF_CLIP"], cfg["VF_CLIP"])
    vl = 0.5 * torch.maximum((value - batch["targets"]) ** 2, (vclip - batch["targets"]) ** 2).mean()
    return loss_actor - cfg["ENT_COEF"] * ent + cfg["VF_COEF"] * vl, (vl, loss_actor, ent)


PPO_CFG = {"CLIP_EPS": 0.12, "VF_CLIP": 0.5, "ENT_COEF": 0.005, "VF_COEF": 0.5}


def test_clip_gradient_splits_ties():
    """jnp.clip's VJP: 0.5 at either bound, 0.25 where both bounds meet x, 1 inside, 0 outside."""
    import torch

    from oracle import net as onet

    x = torch.tensor([0.5, 1.5, 1.0, 0.2, 1.7], dtype=torch.float64, requires_grad=True)
    y = onet.clip(x, 0.5, 1.5)
    assert y.tolist() == [0.5, 1.5, 1.0, 0.5, 1.5]
    y.sum().backward()
    assert x.grad.tolist() == [0.5, 0.5, 1.0, 0.0, 0.0]
    z = torch.tensor([1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53], dtype=torch.float64, requires_grad=True)
    onet.clip(z, 1.0, 1.0).sum().backward()
    assert z.grad.tolist() == [0.25, 0.0, 0.0]
    # the same bounds as tensors, and in float32
    w = torch.tensor([-0.5, 0.5], dtype=torch.float32, requires_grad=True)
    onet.clip(w, torch.tensor(-0.5), torch.tensor(0.5)).sum().backward()
    assert w.grad.tolist() == [0.5, 0.5]


def test_value_loss_gradient_at_ties():
    """maximum(a1, a2) at a1 == a2 sends half the gradient each way: v == v_old gives the unclipped
    gradient (v - t) / n, and v - v_old == +-VF_CLIP exactly gives 0.75 (v - t) / n."""
    import torch

    from oracle import net as onet

    a = torch.tensor([2.0, 3.0], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([2.0, 1.0], dtype=torch.float64, requires_grad=True)
    torch.maximum(a, b).sum().backward()
    assert a.grad.tolist() == [0.5, 1.0] and b.grad.tolist() == [0.5, 0.0]
    vo = torch.tensor([1.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    v = torch.tensor([1.0, 1.5, 0.5, 1.25], dtype=torch.float64, requires_grad=True)
    t = torch.tensor([0.25, 0.25, 2.0, 3.0], dtype=torch.float64)
    lg = torch.zeros((4, 1, 2), dtype=torch.float64)
    bt = {"action": torch.zeros((4, 1), dtype=torch.long), "log_prob": torch.full((4, 1), -np.log(2.0)),
          "gae": torch.zeros(4, dtype=torch.float64), "value": vo, "targets": t}
    cfg = dict(PPO_CFG, VF_COEF=1.0)
    total, (vl, _, _), _, _, vt = onet.ppo_terms(lg, v, bt, cfg, None, 0)
    total.backward()
    np.testing.assert_array_equal(vt.detach().numpy(), 0.5 * (v.detach().numpy() - t.numpy()) ** 2)
    want = np.array([1.0, 0.75, 0.75, 1.0]) * (v.detach().numpy() - t.numpy()) / 4
    np.testing.assert_array_equal(v.grad.numpy(), want)


def test_entropy_masks_without_nan():
    import torch

    from oracle import net as onet

    ninf = float("-inf")
    lg = torch.tensor([[0.3, ninf, -1.2, 0.0], [ninf, ninf, ninf, ninf], [1.0, 2.0, 3.0, 4.0]], dtype=torch.float64,
                      requires_grad=True)
    h = onet.entropy(lg)
    ref = []
    for row in lg.detach().tolist():
        fin = np.array([v for v in row if v > ninf])
        if fin.size:
            p = np.exp(fin - fin.max())
            p /= p.sum()
            ref.append(-(p * np.log(p)).sum())
        else:
            ref.append(0.0)
    np.testing.assert_allclose(h.detach().numpy(), ref, rtol=1e-14, atol=0)
    (h * torch.tensor([1.0, 2.0, 3.0])).sum().backward()
    g = lg.grad.numpy()
    assert np.isfinite(g).all()
    assert g[0, 1] == 0.0 and (g[1] == 0.0).all() and (g[0, [0, 2, 3]] != 0).all()
    # dH/dl_j = -p_j (log p_j + H) on the live entries
    p = torch.softmax(lg.detach()[0, [0, 2, 3]], 0).numpy()
    np.testing.assert_allclose(g[0, [0, 2, 3]], -p * (np.log(p) + ref[0]), rtol=1e-12, atol=1e-16)


@pytest.mark.parametrize("V,C,vpa,mode", [(23, 97, 10, 0), (23, 97, 10, 1)])
def test_ppo_gradients_finite_with_padded_slots(V, C, vpa, mode):
    """Agents of 8, 8 and 7 variables: before the entropy masked its product, every actor_* gradient
    of the mode-0 case was NaN (the loss itself was finite)."""
    import torch

    from oracle import net as onet

    P, bt, av, am = _net_case(V, C, vpa, 16, 2, 3, mode)
    assert not bool(am.all())
    total, parts, _, _ = onet.ppo_loss(P, 2, bt, PPO_CFG, av, am, mode)
    total.backward()
    assert np.isfinite(float(total.detach())) and all(np.isfinite(float(t.detach())) for t in parts)
    for name, p in P.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        if name.startswith("actor_"):
            assert float(p.grad.abs().max()) > 0, name


@pytest.mark.parametrize("V,C,vpa,mode", [(20, 91, 10, 0), (16, 60, 4, 1)])
def test_ppo_loss_split_keeps_unpadded_results(V, C, vpa, mode):
    import torch

    from oracle import net as onet

    P, bt, av, am = _net_case(V, C, vpa, 32, 2, 4, mode)
    assert bool(am.all())
    old_total, old_parts = _ppo_loss_before_split(P, 2, bt, PPO_CFG, av, am, mode)
    old_grads = torch.autograd.grad(old_total, list(P.values()), allow_unused=True)
    total, parts, logits, value = onet.ppo_loss(P, 2, bt, PPO_CFG, av, am, mode)
    grads = torch.autograd.grad(total, list(P.values()), allow_unused=True)
    assert float(total.detach()) == float(old_total.detach())
    assert [float(t.detach()) for t in parts] == [float(t.detach()) for t in old_parts]
    for name, g, og in zip(P, grads, old_grads):
        assert (g is None) == (og is None), name
        if g is not None:
            np.testing.assert_allclose(g.numpy(), og.numpy(), rtol=1e-14, atol=1e-14 * float(og.abs().max()), err_msg=name)
    # ppo_terms on the same logits and value returns the same numbers and the terms they average
    t2, p2, surr, ent_rows, vterms = onet.ppo_terms(logits, value, bt, PPO_CFG, am, mode)
    assert float(t2.detach()) == float(total.detach())
    assert float(surr.mean().detach()) == float(parts[1].detach())
    assert float(ent_rows.mean().detach()) == float(parts[2].detach())
    np.testing.assert_allclose(float(vterms.mean().detach()), float(parts[0].detach()), rtol=1e-15)
