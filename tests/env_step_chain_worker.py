"""The checks of tests/test_env_step_chain_gpu.py, importable (the test runs them in its own process) and runnable as
a child process of that test:

    python env_step_chain_worker.py --threads T     (MARLSAT_ENV_THREADS=T: decode + paths at a forced width)
    python env_step_chain_worker.py --debug         (MARLSAT_LIB=libmarlsat_debug.so: the paths group)

MARLSAT_ENV_THREADS and MARLSAT_LIB are read once per process, hence the child.  Everything is integer work compared
bitwise with the NumPy oracle; the delta cases also with a full-write twin stepped in lockstep.  Not collected by
pytest (no test_ prefix)."""
import argparse
from dataclasses import fields

import numpy as np
import torch

import conftest  # noqa: F401  (puts the repository root and the package on sys.path)
import test_env_gpu as E

# V70 C33 vpa 9: 8 agents of 9, 9, 9, 9, 9, 9, 8, 8 variables -- own ranges that cross a 32-bit word, two ballot
# passes at 64 lanes.  V33 C70 vpa 3: 11 agents, rem == 0, source-word ends in mid-chunk.
SMALL = {"v70c33": (70, 33, 9), "v33c70": (33, 70, 3)}
OUT = (("reward", None), ("done", bool), ("solved", bool), ("num_unsatisfied", None), ("episode_step", None))
STATE_FIELDS = ("variable_assignments", "clauses_satisfied_status", "clause_ntrue", "num_unsatisfied", "step",
                "env_done", "problem_idx")


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_out(out, r, d, info, ctx):
    np.testing.assert_array_equal(_np(out["reward"]), r, err_msg=ctx)
    np.testing.assert_array_equal(_np(out["done"]).astype(bool), d, err_msg=ctx)
    np.testing.assert_array_equal(_np(out["solved"]).astype(bool), info["solved"], err_msg=ctx)
    np.testing.assert_array_equal(_np(out["num_unsatisfied"]), info["num_unsatisfied"], err_msg=ctx)
    np.testing.assert_array_equal(_np(out["episode_step"]), info["episode_step"], err_msg=ctx)


def _check_twins(obs_d, obs_f, st_d, st_f, out_d, out_f, ctx):
    assert torch.equal(obs_d, obs_f), ctx + ": delta obs != full-write obs"
    for f in STATE_FIELDS:
        assert torch.equal(getattr(st_d, f), getattr(st_f, f)), f"{ctx}: state.{f}"
    if out_d is not None:
        for f, _ in OUT:
            assert torch.equal(out_d[f], out_f[f]), f"{ctx}: out.{f}"


def _obs_buffer(env, B, offset):
    """A (B, A, D) obs tensor whose first element lies `offset` elements past its allocation's start."""
    n = B * env.num_agents * env.obs_dim
    return torch.empty(n + offset, dtype=env.obs_dtype, device="cuda")[offset:].view(B, env.num_agents, env.obs_dim)


def _merge(ora, mask, old, new):
    """OracleState: rows of `new` where mask, else `old`."""
    sel = lambda a, b: np.where(mask.reshape(mask.shape + (1,) * (a.ndim - 1)), b, a)
    return type(old)(**{f.name: sel(getattr(old, f.name), getattr(new, f.name)) for f in fields(old)})


# ----------------------------------------------------------------------------------------------- action decode --
def edge_actions(M, n):
    return [-M - 2, -M - 1, -M, -1, 0, n - 1, n, M, M + 3]


def decode_mode0(shape, reward_mode):
    """Every agent in turn takes each edge action while the others idle: env (i, k) gives agent i value k.  Two steps
    into one tensor (the second is a delta step) against the oracle and a full-write twin."""
    V, C, vpa = SMALL[shape]
    env, ora = E._mk(V, C, vpa, max_steps=64, reward_mode=reward_mode)
    A, M = env.num_agents, env.max_vars_per_agent
    sizes = _np(env.action_mask).sum(1)
    rows = [(i, a) for i in range(A) for a in edge_actions(M, int(sizes[i]))]
    B = len(rows)
    acts = np.full((B, A), M, np.int32)
    for b, (i, a) in enumerate(rows):
        acts[b, i] = a
    N = 3
    pool = E._pool(V, C, N, seed0=500)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(5)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs_d, obs_f = env.alloc_obs(B), env.alloc_obs(B)
    _, st_d = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_d)
    _, st_f = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_f)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    for t in range(2):
        ctx = f"decode {shape} reward {reward_mode} t={t}"
        _, out_d = env.step_raw(st_d, _cuda(acts), obs=obs_d, obs_delta=True)
        _, out_f = env.step_raw(st_f, _cuda(acts), obs=obs_f, obs_delta=False)
        oobs, ost, r, d, info = ora.step(ost, acts)
        np.testing.assert_array_equal(_np(obs_d), oobs, err_msg=ctx)
        _check_out(out_d, r, d, info, ctx)
        E._check_state(env, st_d, ost, ctx)
        _check_twins(obs_d, obs_f, st_d, st_f, out_d, out_f, ctx)


def decode_single_agent(V=33, C=70):
    """The same list through the single-agent SatEnv (the scatter drops what lies below -V)."""
    from marlsat.envs.sat_env import SatEnv
    from oracle.single_env import OracleSatEnv

    acts = np.array(edge_actions(V, V), np.int32)
    B = len(acts)
    pool = E._pool(V, C, B, seed0=520)
    x0 = np.random.default_rng(6).integers(0, 2, (B, V)).astype(np.int32)
    env = SatEnv(V, C, max_clause_len=3, c_bonus=2.5, max_steps=8)
    _, st = env.reset(None, pool, assignments=x0)
    ora = OracleSatEnv(V, C, 3, c_bonus=2.5, max_steps=8)
    ost = ora.reset(pool, x0)
    for t in range(2):
        _, st, rew, dones, _ = env.step_env(None, st, {"agent_0": torch.from_numpy(acts)})
        ost, r, d = ora.step(ost, acts)
        np.testing.assert_array_equal(_np(st.variable_assignments), ost["x"], err_msg=f"single t={t}")
        np.testing.assert_array_equal(_np(rew["agent_0"]), r, err_msg=f"single t={t}")
        np.testing.assert_array_equal(_np(dones["__all__"]), d, err_msg=f"single t={t}")


def decode_mode1(shape):
    """Mode 1: every variable's own flip word -- none, all, and random ones."""
    V, C, vpa = SMALL[shape]
    env, ora = E._mk(V, C, vpa, max_steps=64, action_mode=1)
    A, M = env.num_agents, env.max_vars_per_agent
    B, N = 8, 3
    pool = E._pool(V, C, N, seed0=540)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(7)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs_d, obs_f = env.alloc_obs(B), env.alloc_obs(B)
    _, st_d = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_d)
    _, st_f = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_f)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    for t in range(3):
        a = (rng.random((B, A, M)) < (0.5, 0.05, 0.3)[t]).astype(np.int32)
        a[0] = 0
        a[1] = 1
        ctx = f"decode mode 1 {shape} t={t}"
        _, out_d = env.step_raw(st_d, _cuda(a), obs=obs_d, obs_delta=True)
        _, out_f = env.step_raw(st_f, _cuda(a), obs=obs_f, obs_delta=False)
        oobs, ost, r, d, info = ora.step(ost, a)
        np.testing.assert_array_equal(_np(obs_d), oobs, err_msg=ctx)
        _check_out(out_d, r, d, info, ctx)
        E._check_state(env, st_d, ost, ctx)
        _check_twins(obs_d, obs_f, st_d, st_f, out_d, out_f, ctx)


def decode_group():
    for shape in SMALL:
        for reward_mode in (0, 1):  # sparse, PBRS
            decode_mode0(shape, reward_mode)
        decode_mode1(shape)
    decode_single_agent()


# ---------------------------------------------------------------------------------------- paths in one launch --
def paths_in_one_launch(explicit, shape="v33c70"):
    """B = 16 (rq_cap 8), max_steps 3.  Launch 2 holds at once: ten envs that time out (ranks 0-7 through the reset
    workgroups, ranks 8-9 in their own workgroup), an env solved by its step (in-workgroup reset), running envs.
    Ten autoreset delta steps with a plain step and a masked reset in between, explicit reset inputs or Philox
    draws (then the oracle is fed what the device drew)."""
    from marlsat import _lib
    from marlsat.random import Key
    from marlsat.utils.generate_cnf_dataset import generate_sat_solution

    V, C, vpa = SMALL[shape]
    B, N, SEED0 = 16, 4, 560
    assert _lib.lib.msat_reset_queue_words(B) == 2 * B
    env, ora = E._mk(V, C, vpa, max_steps=3)
    A, M = env.num_agents, env.max_vars_per_agent
    pool = E._pool(V, C, N, seed0=SEED0)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(11 + int(explicit))
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    # env 12: one flip away from its instance's planted solution, by a variable whose flip breaks a clause
    SOLVER = 12
    sol = generate_sat_solution(V, SEED0 + int(pidx[SOLVER])).astype(np.int32)
    assert ora.satisfaction(sol[None], pool[pidx[SOLVER]][None])[1][0] == 0
    for v in range(V):
        y = sol.copy()
        y[v] ^= 1
        if ora.satisfaction(y[None], pool[pidx[SOLVER]][None])[1][0] > 0:
            break
    x[SOLVER] = y
    solver_agent = int(_np(env.variable_to_agent_idx)[v])
    solver_action = int(np.nonzero(_np(env.agent_vars)[solver_agent] == v)[0][0])
    obs_d, obs_f = _obs_buffer(env, B, 1), _obs_buffer(env, B, 1)
    _, st_d = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_d)
    _, st_f = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_f)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    # envs 0-9 one step ahead: they time out together at launch 2 (direct counter writes: the queue is rebuilt)
    for st in (st_d, st_f):
        st.step[:10] = 1
        st.invalidate_reset_queue()
    ost.step[:10] = 1
    seen_all = False
    for t in range(10):
        ctx = f"paths {shape} explicit={explicit} t={t}"
        a = rng.integers(0, M + 1, (B, A)).astype(np.int32)
        if t < 2:
            a[SOLVER] = M
        if t == 1:
            a[SOLVER, solver_agent] = solver_action
        if t == 4:  # a plain step in between
            _, out_d = env.step_raw(st_d, _cuda(a), obs=obs_d, obs_delta=True)
            _, out_f = env.step_raw(st_f, _cuda(a), obs=obs_f, obs_delta=False)
            oobs, ost, r, d, info = ora.step(ost, a)
        else:
            kw = {}
            if explicit:
                npidx = rng.integers(0, N, B).astype(np.int32)
                nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
                kw = dict(problem_idx=npidx, assignments=nx)
            else:
                kw = dict(key=Key(77, t))
            _, out_d = env.step_raw(st_d, _cuda(a), autoreset=True, obs=obs_d, obs_delta=True, **kw)
            _, out_f = env.step_raw(st_f, _cuda(a), autoreset=True, obs=obs_f, obs_delta=False, **kw)
            if not explicit:  # what the device drew (only the rows of done envs are used)
                npidx = _np(st_d.problem_idx)
                nx = _np(st_d.variable_assignments)
            was = ost
            oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[npidx], nx.astype(np.int32))
            timed = was.step + 1 >= env.max_steps
            if int(timed.sum()) >= 10 and bool((info["solved"] & ~timed).any()) and bool((~d).any()):
                seen_all = True
        np.testing.assert_array_equal(_np(obs_d), oobs, err_msg=ctx)
        _check_out(out_d, r, d, info, ctx)
        E._check_state(env, st_d, ost, ctx)
        np.testing.assert_array_equal(_np(st_d.clause_ntrue),
                                      ora.num_true_literals(ost.variable_assignments, ost.clauses), err_msg=ctx)
        _check_twins(obs_d, obs_f, st_d, st_f, out_d, out_f, ctx)
        if t == 6:  # a masked reset in between
            m = rng.random(B) < 0.4
            rp = rng.integers(0, N, B).astype(np.int32)
            rx = rng.integers(0, 2, (B, V)).astype(np.uint8)
            for st, ob in ((st_d, obs_d), (st_f, obs_f)):
                env.reset_from_pool(dpool, B, problem_idx=rp, assignments=rx, state=st, reset_mask=m.astype(np.uint8),
                                    obs=ob)
            _, st_r = ora.reset(pool[rp], rx.astype(np.int32))
            ost = _merge(ora, m, ost, st_r)
            np.testing.assert_array_equal(_np(obs_d), ora.get_obs(ost), err_msg=ctx + " masked reset")
            _check_twins(obs_d, obs_f, st_d, st_f, None, None, ctx + " masked reset")
    assert seen_all, "no launch held reset-workgroup, in-workgroup, solved and running envs at once"


def paths_group():
    paths_in_one_launch(True)
    paths_in_one_launch(False)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int)
    ap.add_argument("--debug", action="store_true")
    args = ap.parse_args()
    from marlsat import _lib

    if args.debug:
        assert _lib.LIB_PATH.endswith("libmarlsat_debug.so"), _lib.LIB_PATH
        paths_group()
        torch.cuda.synchronize()
        print("step chain debug ok", _lib.LIB_PATH)
    else:
        env, _ = E._mk(33, 70, 3)
        got = _lib.lib.msat_env_launch_threads(env._desc(16, env.make_pool(E._pool(33, 70, 1))))
        assert got == args.threads, f"msat_env_launch_threads = {got}, forced {args.threads}"
        decode_group()
        paths_group()
        torch.cuda.synchronize()
        print(f"step chain threads {args.threads} ok")
