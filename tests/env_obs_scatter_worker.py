"""The checks of tests/test_env_obs_scatter_gpu.py, importable (the test runs them in its own process) and runnable as
a child process of that test:

    python env_obs_scatter_worker.py --threads T    (MARLSAT_ENV_THREADS=T: uf200 x 8 envs at a forced width)
    python env_obs_scatter_worker.py --debug        (MARLSAT_LIB=libmarlsat_debug.so: bounds checks and the read-back
                                                     of every element a sparse step leaves alone)

MARLSAT_ENV_THREADS and MARLSAT_LIB are read once per process, hence the child.  Everything is integer work compared
bitwise: the delta tensor with a full-write twin stepped in lockstep and both with the NumPy oracle.  Not collected by
pytest (no test_ prefix)."""
import argparse

import numpy as np
import torch

import conftest  # noqa: F401  (puts the repository root and the package on sys.path)
import test_env_gpu as E

B, N, MAX_STEPS, SENTINEL = 8, 4, 5, 7
STATE_FIELDS = ("variable_assignments", "clauses_satisfied_status", "clause_ntrue", "num_unsatisfied", "step",
                "env_done", "problem_idx")
OUT_FIELDS = ("reward", "done", "solved", "num_unsatisfied", "episode_step")

# name: V, C, vars_per_agent
SHAPES = {
    "v33c70": (33, 70, 3),      # 11 agents, rem == 0; source words end in mid-row
    "v64c64": (64, 64, 8),      # V and C whole words
    "v31c33": (31, 33, 31),     # one agent: no neighbour bits, every clause element in row 0
    "v96c832": (96, 832, 6),    # 16 agents, A * D = 16384: 256 lanes, more clauses than lanes (four scan slices)
    "v34c70null": (34, 70, 4),  # 9 agents of 4 x 7 + 3 x 2 variables (rem = 7); literal 0 in 3-wide rows
    "uf200": (200, 860, 8),     # the forced widths' shape (25 agents)
}
NULL_SHAPE = "v34c70null"
_POOLS = {}


def pool_of(shape):
    if shape not in _POOLS:
        V, C, _ = SHAPES[shape]
        pool = E._pool(V, C, N, seed0=800)
        if shape == NULL_SHAPE:  # the reference quirk: a clause with a literal 0 is related to every agent i >= rem
            pool = pool.copy()
            pool[1, ::5, 2] = 0
            pool[3, 1::4, 0] = 0
            pool[3, 2, :] = 0  # no real literal at all: always false, never changes
        _POOLS[shape] = pool
    return _POOLS[shape]


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def obs_buffer(env, offset):
    """A (B, A, D) obs tensor whose first element lies `offset` elements past its allocation's start."""
    n = B * env.num_agents * env.obs_dim
    return torch.empty(n + offset, dtype=env.obs_dtype, device="cuda")[offset:].view(B, env.num_agents, env.obs_dim)


def actions(rng, env, t):
    A, M = env.num_agents, env.max_vars_per_agent
    if env.action_mode == 0:  # index M: no flip.  Most agents idle on odd steps, so the small shapes stay sparse too
        a = rng.integers(0, M + 1, size=(B, A))
        return np.where(rng.random((B, A)) < (0.2 if t % 2 == 0 else 0.85), M, a).astype(np.int32)
    # mode 1: every variable has its own flip bit.  Dense on even steps (about half of V flips: more than a quarter
    # of V + C source bits change, the full write), a few on odd steps (the sparse path)
    return (rng.random((B, A, M)) < (0.5 if t % 2 == 0 else 0.04)).astype(np.int32)


def rollout(shape, action_mode, offset):
    """2 x max_steps + 2 auto-reset steps with explicit reset inputs, max_steps = 5: the batch times out together
    (full writes of fresh instances), sparse steps and (mode 1) steps past the quarter rule run in between, all on
    one tensor.  Returns the numbers of (env, step) pairs that took the sparse write, the full write without a reset,
    a reset, and the sparse write with a changed clause that holds a literal 0."""
    V, C, vpa = SHAPES[shape]
    env, ora = E._mk(V, C, vpa, max_steps=MAX_STEPS, action_mode=action_mode)
    pool = pool_of(shape)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(29 + offset)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs_d, obs_f = obs_buffer(env, offset), obs_buffer(env, offset)
    _, st_d = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_d)
    _, st_f = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_f)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    few = many = resets = null_changed = 0
    for t in range(2 * MAX_STEPS + 2):
        a = actions(rng, env, t)
        npidx = rng.integers(0, N, B).astype(np.int32)
        nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
        _, out_d = env.step_raw(st_d, _cuda(a), autoreset=True, problem_idx=npidx, assignments=nx, obs=obs_d,
                                obs_delta=True)
        _, out_f = env.step_raw(st_f, _cuda(a), autoreset=True, problem_idx=npidx, assignments=nx, obs=obs_f,
                                obs_delta=False)
        prev = ost
        oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[npidx], nx.astype(np.int32))
        ctx = f"{shape} mode {action_mode} offset {offset} t={t}"
        assert torch.equal(obs_d, obs_f), ctx + ": delta obs != full-write obs"
        np.testing.assert_array_equal(_np(obs_d), oobs, err_msg=ctx)
        for f in STATE_FIELDS:
            assert torch.equal(getattr(st_d, f), getattr(st_f, f)), f"{ctx}: state.{f}"
        for f in OUT_FIELDS:
            assert torch.equal(out_d[f], out_f[f]), f"{ctx}: out.{f}"
        np.testing.assert_array_equal(_np(st_d.variable_assignments), ost.variable_assignments, err_msg=ctx)
        np.testing.assert_array_equal(_np(out_d["reward"]), r, err_msg=ctx)
        np.testing.assert_array_equal(_np(out_d["done"]).astype(bool), d, err_msg=ctx)
        # which write each env took (t = 0 is the tensor's first step: whole blocks)
        dcl = prev.clauses_satisfied_status != ost.clauses_satisfied_status
        flips = (prev.variable_assignments != ost.variable_assignments).sum(1) + dcl.sum(1)
        if t > 0:
            live = ~d
            sparse = live & (4 * flips <= V + C)
            few += int(sparse.sum())
            many += int((live & (4 * flips > V + C)).sum())
            null_changed += int((sparse & (dcl & (prev.clauses == 0).any(-1)).any(1)).sum())
        resets += int(d.sum())
    return few, many, resets, null_changed


def noop_stores_nothing(shape, offset):
    V, C, vpa = SHAPES[shape]
    env, ora = E._mk(V, C, vpa, max_steps=512)
    pool = pool_of(shape)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(23)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs = obs_buffer(env, offset)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    noop = np.full((B, env.num_agents), env.max_vars_per_agent, dtype=np.int32)  # index M: no flip
    # the first step into `obs` writes it whole (nothing is known about it) and records what it wrote
    env.step_raw(st, _cuda(noop), obs=obs, obs_delta=True)
    oobs, ost, _, d, _ = ora.step(ost, noop)
    assert not d.any()  # no env is done: none is skipped below
    np.testing.assert_array_equal(_np(obs), oobs)
    obs.fill_(SENTINEL)  # nothing changes from here on: every element is a kept one
    for _ in range(2):
        _, out = env.step_raw(st, _cuda(noop), obs=obs, obs_delta=True)
        assert not _np(out["done"]).any()
        assert (_np(obs) == SENTINEL).all(), f"{shape} offset {offset}: a no-op step stored something"
    np.testing.assert_array_equal(_np(st.variable_assignments), x)
    env.invalidate_obs(obs)
    env.step_raw(st, _cuda(noop), obs=obs, obs_delta=True)
    np.testing.assert_array_equal(_np(obs), oobs)


def lone_variable_flip(offset):
    """V = 33, clauses over variables 1 .. 32 only: variable 33 is in no clause, so it is nobody's neighbour and its
    flip changes no clause.  The step that flips it stores exactly one element per env: (its owner's row, own-variable
    element 32)."""
    V, C, vpa = 33, 70, 3
    env, ora = E._mk(V, C, vpa, max_steps=512)
    pool = E._pool(V - 1, C, N, seed0=820)
    assert np.abs(pool).max() == V - 1
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(41)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs = obs_buffer(env, offset)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    A, M = env.num_agents, env.max_vars_per_agent
    noop = np.full((B, A), M, dtype=np.int32)
    env.step_raw(st, _cuda(noop), obs=obs, obs_delta=True)
    oobs0, ost, _, d, _ = ora.step(ost, noop)
    assert not d.any()
    np.testing.assert_array_equal(_np(obs), oobs0)
    owner, local = (V - 1) // vpa, (V - 1) % vpa
    assert int(_np(env.agent_vars)[owner, local]) == V - 1
    a = noop.copy()
    a[:, owner] = local
    obs.fill_(SENTINEL)
    _, out = env.step_raw(st, _cuda(a), obs=obs, obs_delta=True)
    oobs1, ost, _, d, _ = ora.step(ost, a)
    assert not d.any()
    want = oobs1 != oobs0
    assert want.sum() == B and want[:, owner, V - 1].all()  # the oracle agrees: one element per env
    got = _np(obs)
    np.testing.assert_array_equal(got != SENTINEL, want, err_msg=f"offset {offset}: elements stored")
    np.testing.assert_array_equal(got[want], oobs1[want])
    np.testing.assert_array_equal(got[:, owner, V - 1], 1 - x[:, V - 1].astype(np.int32))


def forced_width_group(T):
    """uf200 x 8 envs at a forced width.  At 64 lanes C = 860 > 4 x 64 clauses and A * WV = 25 x 8 = 200 > 2 x 64
    neighbour tasks lie past the prefetch: both tail loops of the scatter run."""
    from marlsat import _lib

    V, C, vpa = SHAPES["uf200"]
    env, _ = E._mk(V, C, vpa)
    got = _lib.lib.msat_env_delta_launch_threads(env._desc(B, env.make_pool(pool_of("uf200"))))
    assert got == T, f"msat_env_delta_launch_threads = {got}, forced {T}"
    for action_mode in (0, 1):
        for offset in (0, 3):
            few, many, resets, _ = rollout("uf200", action_mode, offset)
            assert few >= 1 and resets >= B, (few, resets)
            assert action_mode == 0 or many >= 1
    noop_stores_nothing("uf200", 1)


def debug_group():
    """(No sentinel cases here: the debug library reads back every element a sparse step leaves alone.)"""
    for shape in ("v33c70", NULL_SHAPE):
        for action_mode in (0, 1):
            few, _, resets, _ = rollout(shape, action_mode, 1)
            assert few >= 1 and resets >= B, (few, resets)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int)
    ap.add_argument("--debug", action="store_true")
    args = ap.parse_args()
    from marlsat import _lib

    if args.debug:
        assert _lib.LIB_PATH.endswith("libmarlsat_debug.so"), _lib.LIB_PATH
        debug_group()
        torch.cuda.synchronize()
        print("obs scatter debug ok", _lib.LIB_PATH)
    else:
        forced_width_group(args.threads)
        torch.cuda.synchronize()
        print(f"obs scatter threads {args.threads} ok")
