"""The env step's delta observation write (msat_env_step_delta) vs the full write and the NumPy oracle.

A step into an obs tensor the library has written before stores only the groups of elements that changed since
(per obs tensor, the library keeps a shadow of what it wrote: problem index, assignment bits, clause bits).  Every
comparison here is bitwise: a delta rollout, a full-write rollout (``obs_delta=False``) and the oracle must agree on
the observation, the state and the step record after every step.

The delta rollouts pass ``obs_delta=True``: left to itself the library takes the delta write only for large int32
blocks (SATEnv.obs_delta_default), and the shapes here are the small ones that reach the kernel's edges.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dataclasses import replace

from conftest import ROOT
from marlsat.random import Key
from oracle.sat_env import OracleSATEnv

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("variable_assignments", "clauses_satisfied_status", "clause_ntrue", "num_unsatisfied", "step",
                "env_done", "problem_idx")
OUT_FIELDS = ("reward", "done", "solved", "num_unsatisfied", "episode_step")


def _pool(V, C, N, seed0=0):
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses

    if V == 1:  # (N, 1, 1): the unit clauses x and not-x
        return np.array([[[1]], [[-1]]] * ((N + 1) // 2), dtype=np.int32)[:N]
    return np.stack([generate_sat_clauses(V, C, 3, seed=seed0 + i) for i in range(N)])


def _mk(V, C, vpa, max_steps, **kw):
    from marlsat import SATEnv

    env = SATEnv(V, C, max_steps=max_steps, vars_per_agent=vpa, **kw)
    ora = OracleSATEnv(V, C, max_steps=max_steps, vars_per_agent=vpa, reward_mode=kw.get("reward_mode", 0),
                       action_mode=kw.get("action_mode", 0))
    return env, ora


def _np(t):
    return t.detach().cpu().numpy()


def _actions(rng, env, B):
    A, M = env.num_agents, env.max_vars_per_agent
    if env.action_mode == 0:
        return rng.integers(0, M + 1, size=(B, A)).astype(np.int32)
    return rng.integers(0, 2, size=(B, A, M)).astype(np.int32)


def _obs_buffer(env, B, offset):
    """A (B, A, D) obs tensor whose first element lies `offset` elements past its allocation's start."""
    n = B * env.num_agents * env.obs_dim
    buf = torch.empty(n + offset, dtype=env.obs_dtype, device="cuda")
    return buf[offset:].view(B, env.num_agents, env.obs_dim)


def _same_state(a, b, ctx):
    for f in STATE_FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f"{ctx}: state.{f}"


def _same_out(a, b, ctx):
    for f in OUT_FIELDS:
        assert torch.equal(a[f], b[f]), f"{ctx}: out.{f}"


# name, V, C, vars_per_agent, B, N, max_steps
SHAPES = {
    "uf20": (20, 91, 10, 8, 5, 5),      # A*D = 262: not a multiple of 4 (head / tail stores, rows straddle words)
    "v1c1": (1, 1, 1, 4, 2, 4),         # A*D = 3
    "uf50": (50, 218, 10, 64, 6, 6),    # 8 envs in reset workgroups, 56 reset in their step workgroup
    "uf200": (200, 860, 8, 16, 4, 4),   # the 512-lane form
}
# shape, obs dtype, action mode, reward mode, obs base offset (elements), group bytes (None: the default)
CASES = [(s, dt, 0, 0, 0, None) for s in SHAPES for dt in ("int32", "int8")]
CASES += [("uf20", "int32", am, rm, 0, None) for am, rm in ((0, 1), (1, 0), (1, 1))]
CASES += [("uf50", "int32", am, rm, 0, None) for am, rm in ((0, 1), (1, 0), (1, 1))]
CASES += [("uf20", "int32", 0, 0, 1, None), ("uf20", "int8", 0, 0, 1, None), ("uf50", "int32", 1, 1, 1, None)]  # unaligned
# the other group sizes (their own store loop), aligned and not, both dtypes
CASES += [("uf20", dt, 0, 0, off, g) for dt in ("int32", "int8") for off in (0, 1) for g in (16, 64, 128)]
CASES += [("uf50", "int32", 0, 0, 3, g) for g in (16, 64, 128)]


@pytest.mark.parametrize("shape,dtype,action_mode,reward_mode,offset,group", CASES)
def test_delta_rollout_matches_full_write_and_oracle(shape, dtype, action_mode, reward_mode, offset, group,
                                                     monkeypatch):
    """3 x max_steps auto-reset steps with explicit reset inputs: solved envs, timeouts (the batch starts
    together, so whole-batch timeouts with reset-queue side workgroups) and plain steps in between."""
    from marlsat.envs import multi_agent_sat_env as mod

    if group is not None:
        monkeypatch.setattr(mod, "OBS_DELTA_GROUP", group)
    V, C, vpa, B, N, max_steps = SHAPES[shape]
    env, ora = _mk(V, C, vpa, max_steps, action_mode=action_mode, reward_mode=reward_mode,
                   obs_dtype=getattr(torch, dtype))
    pool = _pool(V, C, N)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(11)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs_d, obs_f = _obs_buffer(env, B, offset), _obs_buffer(env, B, offset)
    _, st_d = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_d)
    _, st_f = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_f)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    whole_batch = 0
    for t in range(3 * max_steps):
        a = _actions(rng, env, B)
        npidx = rng.integers(0, N, B).astype(np.int32)
        nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
        at = torch.from_numpy(a).cuda()
        _, out_d = env.step_raw(st_d, at, autoreset=True, problem_idx=npidx, assignments=nx, obs=obs_d,
                                obs_delta=True)
        _, out_f = env.step_raw(st_f, at, autoreset=True, problem_idx=npidx, assignments=nx, obs=obs_f,
                                obs_delta=False)
        oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[npidx], nx.astype(np.int32))
        ctx = f"{shape} {dtype} t={t}"
        assert torch.equal(obs_d, obs_f), ctx
        np.testing.assert_array_equal(_np(obs_d).astype(np.int32), oobs, err_msg=ctx)
        _same_state(st_d, st_f, ctx)
        _same_out(out_d, out_f, ctx)
        np.testing.assert_array_equal(_np(st_d.variable_assignments), ost.variable_assignments, err_msg=ctx)
        np.testing.assert_array_equal(_np(st_d.step), ost.step, err_msg=ctx)
        np.testing.assert_array_equal(_np(out_d["reward"]), r, err_msg=ctx)
        np.testing.assert_array_equal(_np(out_d["done"]).astype(bool), d, err_msg=ctx)
        whole_batch += bool(d.all())
    if shape != "v1c1":  # (a one-variable env is solved every other step: its batch rarely ends together)
        assert whole_batch >= 1


def test_stale_state_restored_as_the_bench_does():
    """The state arrays go back to a saved start and the episode counters are written directly (bench.py's
    pre-roll); the obs buffer is left as it was.  The next step's obs is that of the restored state."""
    V, C, vpa, B, N, max_steps = 50, 218, 10, 16, 6, 512
    env, ora = _mk(V, C, vpa, max_steps)
    pool = _pool(V, C, N)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(5)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs = env.alloc_obs(B)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs)
    _, ost0 = ora.reset(pool[pidx], x.astype(np.int32))
    start = [getattr(st, f).clone() for f in STATE_FIELDS]
    for t in range(3):  # the obs buffer (and its shadow) now describe a state three steps on
        npidx = rng.integers(0, N, B).astype(np.int32)
        nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
        env.step_raw(st, torch.from_numpy(_actions(rng, env, B)).cuda(), autoreset=True, problem_idx=npidx,
                     assignments=nx, obs=obs, obs_delta=True)
    for f, t in zip(STATE_FIELDS, start):
        getattr(st, f).copy_(t)
    steps = rng.integers(0, max_steps, B).astype(np.int32)
    steps[:3] = max_steps - 1  # these time out in the next step
    st.step.copy_(torch.from_numpy(steps))
    st.invalidate_reset_queue()
    a = _actions(rng, env, B)
    npidx = rng.integers(0, N, B).astype(np.int32)
    nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
    env.step_raw(st, torch.from_numpy(a).cuda(), autoreset=True, problem_idx=npidx, assignments=nx, obs=obs,
                 obs_delta=True)
    oobs, ost, _, d, _ = ora.step_autoreset(replace(ost0, step=steps), a, pool[npidx], nx.astype(np.int32))
    assert d[:3].all()
    np.testing.assert_array_equal(_np(obs), oobs)
    np.testing.assert_array_equal(_np(st.variable_assignments), ost.variable_assignments)


def test_delta_step_leaves_unchanged_elements_alone_and_invalidate_obs_rewrites_them(dtype="int32"):
    V, C, vpa, B, N, max_steps = 50, 218, 10, 16, 6, 512
    SENTINEL = 7
    env, ora = _mk(V, C, vpa, max_steps, obs_dtype=getattr(torch, dtype))
    pool = _pool(V, C, N)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(9)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs = env.alloc_obs(B)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    acts = [_actions(rng, env, B) for _ in range(3)]
    # the first step into `obs` writes it whole (nothing is known about it) and records what it wrote
    env.step_raw(st, torch.from_numpy(acts[0]).cuda(), obs=obs, obs_delta=True)
    oobs1, ost, _, d1, _ = ora.step(ost, acts[0])
    np.testing.assert_array_equal(_np(obs).astype(np.int32), oobs1)
    oobs2, ost, _, d2, _ = ora.step(ost, acts[1])
    oobs3, ost, _, d3, _ = ora.step(ost, acts[2])
    assert not d1.any() and not d2.any() and not d3.any()  # no env is done: none may be skipped below
    changed = oobs1 != oobs2
    assert changed.any()
    obs[torch.from_numpy(~changed).cuda()] = SENTINEL
    env.step_raw(st, torch.from_numpy(acts[1]).cuda(), obs=obs, obs_delta=True)
    got = _np(obs).astype(np.int32)
    np.testing.assert_array_equal(got[changed], oobs2[changed])
    assert ((got == SENTINEL) | (got == oobs2)).all()
    assert (got == SENTINEL).sum() > got.size // 2  # a full write leaves none
    env.invalidate_obs(obs)
    env.step_raw(st, torch.from_numpy(acts[2]).cuda(), obs=obs, obs_delta=True)
    np.testing.assert_array_equal(_np(obs).astype(np.int32), oobs3)


def _rng_pair(V=50, C=218, vpa=10, B=16, N=6, max_steps=4, seed0=0):
    env, _ = _mk(V, C, vpa, max_steps)
    dpool = env.make_pool(_pool(V, C, N, seed0))
    states = [env.reset_from_pool(dpool, B, Key(3, 0), with_obs=False)[1] for _ in range(2)]
    return env, dpool, states


def test_two_steppers_share_one_obs_tensor():
    env, dpool, (st_d, st_f) = _rng_pair()
    B = st_d.num_envs
    obs_d, obs_f = env.alloc_obs(B), env.alloc_obs(B)
    out_d, out_f = env._step_out(B), env._step_out(B)
    s1 = env.stepper(st_d, obs_d, out_d, seed=7, obs_delta=True)
    s2 = env.stepper(st_d, obs_d, out_d, seed=7, obs_delta=True)
    sf = env.stepper(st_f, obs_f, out_f, seed=7, obs_delta=False)
    rng = np.random.default_rng(1)
    for t in range(12):
        a = torch.from_numpy(_actions(rng, env, B)).cuda()
        (s1 if t % 2 == 0 else s2)(a, 100 + t)
        sf(a, 100 + t)
        assert torch.equal(obs_d, obs_f), t
        _same_state(st_d, st_f, t)
        _same_out(out_d, out_f, t)


def test_full_write_stepper_on_the_tensor_turns_delta_steps_into_full_writes():
    """A pre-bound full-write stepper does no per-call bookkeeping, so once one exists for a tensor no record of
    that tensor is trusted: delta steppers bound to it write whole blocks (a sentinel does not survive)."""
    env, dpool, (st_d, st_f) = _rng_pair(max_steps=512)
    B = st_d.num_envs
    obs_d, obs_f = env.alloc_obs(B), env.alloc_obs(B)
    out_d, out_f = env._step_out(B), env._step_out(B)
    sd = env.stepper(st_d, obs_d, out_d, seed=7, obs_delta=True)
    sf = env.stepper(st_f, obs_f, out_f, seed=7, obs_delta=False)
    rng = np.random.default_rng(6)
    steps = [sd, sd, None, sd, None, sd]  # None: the full-write stepper on obs_d, made at t = 2
    full_on_d = None
    for t, s_ in enumerate(steps):
        a = torch.from_numpy(_actions(rng, env, B)).cuda()
        if s_ is None and full_on_d is None:
            full_on_d = env.stepper(st_d, obs_d, out_d, seed=7, obs_delta=False)
        if t == 3:
            obs_d.fill_(7)  # what a delta step would leave mostly in place
        (s_ or full_on_d)(a, 100 + t)
        sf(a, 100 + t)
        assert torch.equal(obs_d, obs_f), t
        _same_state(st_d, st_f, t)


def test_one_state_stepped_into_two_obs_tensors():
    env, dpool, (st_d, st_f) = _rng_pair()
    B = st_d.num_envs
    obs_d, obs_f = [env.alloc_obs(B), env.alloc_obs(B)], env.alloc_obs(B)
    rng = np.random.default_rng(2)
    for t in range(12):
        a = torch.from_numpy(_actions(rng, env, B)).cuda()
        env.step_raw(st_d, a, autoreset=True, key=Key(7, 100 + t), obs=obs_d[t % 2], obs_delta=True)
        env.step_raw(st_f, a, autoreset=True, key=Key(7, 100 + t), obs=obs_f, obs_delta=False)
        assert torch.equal(obs_d[t % 2], obs_f), t
        _same_state(st_d, st_f, t)


def test_one_obs_tensor_under_two_pools():
    """Row i of the second pool is another instance: equal problem_idx, other masks."""
    env, pool1, (st1_d, st1_f) = _rng_pair(max_steps=512)
    B = st1_d.num_envs
    pool2 = env.make_pool(_pool(50, 218, 6, seed0=100))
    st2_d, st2_f = (env.reset_from_pool(pool2, B, Key(3, 0), with_obs=False)[1] for _ in range(2))
    assert torch.equal(st1_d.problem_idx, st2_d.problem_idx)
    obs_d, obs_f = env.alloc_obs(B), env.alloc_obs(B)
    rng = np.random.default_rng(3)
    for t in range(8):
        a = torch.from_numpy(_actions(rng, env, B)).cuda()
        sd, sf = (st1_d, st1_f) if t % 2 == 0 else (st2_d, st2_f)
        env.step_raw(sd, a, autoreset=True, key=Key(7, 100 + t), obs=obs_d, obs_delta=True)
        env.step_raw(sf, a, autoreset=True, key=Key(7, 100 + t), obs=obs_f, obs_delta=False)
        assert torch.equal(obs_d, obs_f), t
        _same_state(sd, sf, t)


def test_masked_reset_into_the_obs_tensor_between_steps():
    env, dpool, (st_d, st_f) = _rng_pair(max_steps=512)
    B = st_d.num_envs
    obs_d, obs_f = env.alloc_obs(B), env.alloc_obs(B)
    rng = np.random.default_rng(4)
    for t in range(9):
        a = torch.from_numpy(_actions(rng, env, B)).cuda()
        env.step_raw(st_d, a, autoreset=True, key=Key(7, 100 + t), obs=obs_d, obs_delta=True)
        env.step_raw(st_f, a, autoreset=True, key=Key(7, 100 + t), obs=obs_f, obs_delta=False)
        assert torch.equal(obs_d, obs_f), t
        if t % 3 == 1:
            m = torch.from_numpy((rng.integers(0, 3, B) == 0).astype(np.uint8)).cuda()
            for st, o in ((st_d, obs_d), (st_f, obs_f)):
                env.reset_from_pool(dpool, B, Key(9, t), state=st, reset_mask=m, obs=o)
            assert torch.equal(obs_d, obs_f), t
        _same_state(st_d, st_f, t)


DEBUG_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {root!r} + '/marl-sat_amd']
from marlsat import _lib
assert _lib.LIB_PATH.endswith('libmarlsat_debug.so'), _lib.LIB_PATH
from marlsat import SATEnv
from marlsat.random import Key
from marlsat.utils.generate_cnf_dataset import generate_sat_clauses
env = SATEnv(20, 91, max_steps=4, vars_per_agent=10)
pool = env.make_pool(np.stack([generate_sat_clauses(20, 91, 3, seed=i) for i in range(5)]))
B = 8
obs = env.alloc_obs(B)
ref = env.alloc_obs(B)
_, st = env.reset_from_pool(pool, B, Key(1, 0), with_obs=False)
rng = np.random.default_rng(0)
for t in range(10):
    a = torch.from_numpy(rng.integers(0, 11, (B, 2)).astype(np.int32)).cuda()
    env.step_raw(st, a, autoreset=True, key=Key(2, t), obs=obs, obs_delta=True)  # kept chunks are read back
    assert torch.equal(obs, env.get_obs(st).tensor), t
print("debug delta rollout ok", _lib.LIB_PATH)
"""


def test_debug_library_reads_back_the_chunks_a_delta_step_keeps():
    lib = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    assert os.path.exists(lib), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT.format(root=ROOT)], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, MARLSAT_LIB=lib))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "debug delta rollout ok" in r.stdout and "libmarlsat_debug.so" in r.stdout
