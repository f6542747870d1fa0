"""GPU: instances with more variables than the cold kernels' 256-lane workgroups and than the env step's natural
workgroup (tests/irregular_pools.py: wide257, wide300, wide513k2, wide600; tests/test_wide_instances_cpu.py checks the
pools and the host builder against the oracle).  Everything is exact: the device graph templates against the host
builder, the assembled batch against the host reconstruction from the oracle, static variable features, reset, masks
and rollouts against OracleSATEnv, the behavioural-cloning labels against the reference greedy.

What runs here for the first time: a second and third trip of every `v += 256` loop of graph_templates_kernel,
static_var_features_kernel and bc_labels_kernel; gt_scan with more than one element per thread; the rank loop over
more than 64 occurrences; bitmap rows past word 8; the env step with more variables than lanes at the widths the
library picks itself (256 for wide300, 512 and, with the delta write, 256 for wide600)."""
import numpy as np
import pytest
import torch

import irregular_pools as ip
from oracle.sat_env import OracleSATEnv
from oracle.single_env import compute_joint_labels_parallel_greedy as oracle_labels
from test_env_gpu import _check_state, _mk, _np
from test_graph_templates_gpu import _assert_equal, _both
from test_irregular_assemble_gpu import check_assembled_batch
from test_wide_instances_cpu import WIDE, num_agents, template_c_star

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ templates ----
@pytest.mark.parametrize("name", WIDE)
def test_device_templates_equal_host_builder_on_wide_pools(name):
    from marlsat.learners.graphs import device_templates_fit

    p = ip.get(name)
    assert device_templates_fit(p.V, p.C, p.K)  # the kernels run: no host fallback
    _, host, dev = _both(p.pool, p.V, num_agents(p))
    _assert_equal(dev, host)
    gc = host.gc.cpu().numpy()
    assert (np.diff(gc[1]) == 0).any()  # low-vars: an agent's graph with no clause row


def test_device_templates_equal_host_builder_at_the_lds_bound():
    """One generated instance of (600, C*, 3), C* the largest clause count the kernels' LDS plan takes at V = 600
    (tests/test_wide_instances_cpu.py)."""
    from marlsat import ProblemPool
    from marlsat.learners import graphs

    V, K, A = 600, 3, 15
    C = template_c_star(V, K)
    assert graphs.device_templates_fit(V, C, K) and not graphs.device_templates_fit(V, C + 1, K)
    gen = ProblemPool.generate((V, C, K), 1, 11)
    _, host, dev = _both(gen.clauses.cpu().numpy(), V, A)
    _assert_equal(dev, host)
    assert dev.gv.shape == (1, A + 2)


# ------------------------------------------------------------- assembly ----
@pytest.mark.parametrize("critic_only", [False, True], ids=["full", "critic_only"])
@pytest.mark.parametrize("name", ["wide257", "wide600"])
def test_assembled_batch_equals_host_reconstruction_on_wide_pools(name, critic_only, monkeypatch):
    check_assembled_batch(name, critic_only, monkeypatch)


# ------------------------------------- static features, tables, masks ----
@pytest.mark.parametrize("name", WIDE)
def test_static_features_and_reset_match_oracle(name):
    p = ip.get(name)
    env, ora = _mk(p.V, p.C, p.vpa)
    assert env.num_agents == num_agents(p)
    dpool = env.make_pool(p.pool)
    svf = _np(dpool.static_var_features())
    want = np.ascontiguousarray(ora.static_var_features(p.pool), dtype=np.float32)
    assert svf.dtype == np.float32 and svf.shape == want.shape
    assert np.array_equal(svf.view(np.int32), want.view(np.int32))
    obs, st = env.reset_from_pool(dpool, len(p.inst), problem_idx=p.inst, assignments=p.x)
    oobs, ost = ora.reset(p.pool[p.inst], p.x.astype(np.int32))
    np.testing.assert_array_equal(_np(obs), oobs)
    _check_state(env, st, ost, name)  # the state and the three mask tensors msat_env_masks writes
    np.testing.assert_array_equal(_np(env.clause_features(st)), ora.clause_features(ost))
    np.testing.assert_array_equal(_np(env.get_obs(st).tensor), oobs)


# ------------------------------------------- env step at natural width ----
WIDTHS = {"wide300": (256, 256), "wide600": (512, 256)}  # full-write launch, delta launch


def _wide_actions(rng, ora, B, t):
    """Actions of step t with flips of variables past 255 (and past 511 where there are any) planted; returns the
    actions and the set of variables they flip."""
    A, M, V = ora.num_agents, ora.max_vars_per_agent, ora.num_vars
    av = ora.agent_vars
    high = [v for v in (V - 1, 260, 515) if v < V]
    if ora.action_mode == 0:
        a = rng.integers(0, M + 1, size=(B, A)).astype(np.int32)
        for k, v in enumerate(high):
            i, j = np.argwhere(av == v)[0]
            a[(t + k) % B, i] = j
        ok = a < M
        flipped = av[np.nonzero(ok)[1], a[ok]]
    else:
        dense = t % 2 == 1  # sparse steps stay under the delta write's quarter-of-the-bits limit, dense ones pass it
        a = (rng.random((B, A, M)) < (0.5 if dense else 0.03)).astype(np.int32)
        for k, v in enumerate(high):
            i, j = np.argwhere(av == v)[0]
            a[(t + k) % B, i, j] = 1
        flipped = np.broadcast_to(av, a.shape)[a == 1]
    return a, set(int(v) for v in flipped if v >= 0)


@pytest.mark.parametrize("delta", [False, True], ids=["full_write", "delta_write"])
@pytest.mark.parametrize("action_mode", [0, 1])
@pytest.mark.parametrize("name", ["wide300", "wide600"])
def test_rollout_at_the_natural_width_matches_oracle(name, action_mode, delta, monkeypatch):
    from marlsat import _lib
    from marlsat.envs import multi_agent_sat_env as mod

    monkeypatch.setenv("MARLSAT_OBS_DELTA", "2" if delta else "0")
    monkeypatch.setattr(mod, "OBS_DELTA", 2 if delta else 0)  # (the module reads the variable once, at import)
    p = ip.get(name)
    B, V = 4, p.V
    env, ora = _mk(V, p.C, p.vpa, max_steps=3, action_mode=action_mode)
    assert env.obs_delta_default() == delta
    dpool = env.make_pool(p.pool)
    desc = env._desc(B, dpool)
    got = (_lib.lib.msat_env_launch_threads(desc), _lib.lib.msat_env_delta_launch_threads(desc))
    print(f"{name}: msat_env_launch_threads = {got[0]}, msat_env_delta_launch_threads = {got[1]}")
    assert got == WIDTHS[name] and max(got) < V
    rng = np.random.default_rng(300 + action_mode)
    N = p.pool.shape[0]
    pidx = np.array([0, 1, 0, 1], np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs = env.alloc_obs(B)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs)
    oobs, ost = ora.reset(p.pool[pidx], x.astype(np.int32))
    np.testing.assert_array_equal(_np(obs), oobs)
    flipped, n_done, whole_batch = set(), 0, 0
    for t in range(6):
        a, f = _wide_actions(rng, ora, B, t)
        flipped |= f
        npidx = rng.integers(0, N, B).astype(np.int32)
        nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
        _, out = env.step_raw(st, torch.from_numpy(a).cuda(), autoreset=True, problem_idx=npidx, assignments=nx,
                              obs=obs)
        oobs, ost, r, d, info = ora.step_autoreset(ost, a, p.pool[npidx], nx.astype(np.int32))
        ctx = f"{name} mode {action_mode} t={t}"
        np.testing.assert_array_equal(_np(st.variable_assignments), ost.variable_assignments, err_msg=ctx)
        np.testing.assert_array_equal(_np(out["reward"]), r, err_msg=ctx)
        np.testing.assert_array_equal(_np(out["done"]).astype(bool), d, err_msg=ctx)
        np.testing.assert_array_equal(_np(obs), oobs, err_msg=ctx)
        np.testing.assert_array_equal(_np(out["num_unsatisfied"]), info["num_unsatisfied"], err_msg=ctx)
        _check_state(env, st, ost, ctx)
        n_done += int(d.sum())
        whole_batch += bool(d.all())
    assert n_done >= 2 * B and whole_batch >= 1  # max_steps = 3: the batch times out and resets, twice
    assert any(v >= 256 for v in flipped) and (V <= 512 or any(v >= 512 for v in flipped))


# ------------------------------------------------------------ BC labels ----
@pytest.mark.parametrize("name", ["wide257", "wide600"])
def test_bc_labels_match_reference_greedy_on_wide_pools(name):
    from marlsat import SATEnv
    from marlsat.runners.behavioral_cloning import compute_joint_labels

    p = ip.get(name)
    V, C, B = p.V, p.C, 6
    env = SATEnv(V, C, max_steps=5, vars_per_agent=p.vpa)
    pool = env.make_pool(p.pool)
    rng = np.random.default_rng(V)
    pidx = np.array([0, 1, 0, 1, 1, 0], np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    labels, deltas = compute_joint_labels(env, pool, pidx, x, 0.0, return_deltas=True)
    labels, deltas = labels.cpu().numpy(), deltas.cpu().numpy()
    ora = OracleSATEnv(V, C, 5, vars_per_agent=p.vpa)
    for b in range(B):
        cl = p.pool[pidx[b]]
        np.testing.assert_array_equal(labels[b], oracle_labels(ora, cl, x[b].astype(np.int32), 0.0),
                                      err_msg=f"env {b}")
        _, base = ora.satisfaction(x[b][None].astype(np.int32), cl[None])
        flips = np.repeat(x[b][None].astype(np.int32), V, 0)
        flips[np.arange(V), np.arange(V)] ^= 1
        _, nu = ora.satisfaction(flips, np.repeat(cl[None], V, 0))
        np.testing.assert_array_equal(deltas[b], nu - base[0], err_msg=f"env {b}")
    # the agents past variable 255 do get labels that are flips, not only the no-op
    M = env.max_vars_per_agent
    lo_agent = min(i for i, g in enumerate(env.agent_groups.values()) if g[-1] >= 256)
    assert (labels[pidx == 0][:, lo_agent:] < M).any()


# ------------------------------------------------------------ pool pack ----
def test_pool_pack_refuses_int32_min():
    """INT32_MIN has no int negation: it used to pass the |l| > V test as a negative number and leave a 32-bit code
    across its clause's other slots with the error flag clear."""
    from marlsat import ProblemPool

    with pytest.raises(ValueError, match="num_vars=3"):
        ProblemPool([[[1, -2147483648, 2]]], 3)
    with pytest.raises(ValueError, match="num_vars=3"):
        ProblemPool([[[1, 4, 2]]], 3)
    assert tuple(ProblemPool([[[1, -3, 2]]], 3).packed.shape) == (1, 1, 4)
