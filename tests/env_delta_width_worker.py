"""The checks of tests/test_env_delta_width_gpu.py and the forced-width check of tests/test_env_delta_width_cpu.py,
runnable as a child process (MARLSAT_ENV_THREADS and MARLSAT_LIB are read once per process):

    python env_delta_width_worker.py --host T       (MARLSAT_ENV_THREADS=T: both width exports report T; no GPU)
    python env_delta_width_worker.py --natural      (no override: the delta rule's own widths)
    python env_delta_width_worker.py --forced T     (MARLSAT_ENV_THREADS=T: forced delta on task-index shapes)
    python env_delta_width_worker.py --debug        (MARLSAT_LIB=libmarlsat_debug.so: one natural-width case)

A launch with an obs shadow (msat_env_step_delta) takes its workgroup size from env_delta_threads, not from
env_threads (env_kernels.hip): msat_env_delta_launch_threads reports it.  Everything is integer work compared bitwise
with the NumPy oracle.  Not collected by pytest (no test_ prefix)."""
import argparse
import ctypes

import numpy as np

import conftest  # noqa: F401  (puts the repository root and the package on sys.path)

DELTA_MIN_ELEMS = 16384  # A * D from which the delta write is the default, and the delta rule its own

# V, C, A (A <= V; D = 2V + C): the grid of tests/test_capi.py
GRID = [
    (20, 91, 2), (50, 218, 5), (100, 430, 10), (100, 430, 5), (60, 600, 2), (200, 860, 10), (200, 860, 25),
    (130, 60, 65), (126, 60, 63), (23, 97, 3), (12, 40, 1), (1, 1, 1),
    (100, 824, 4),   # A * D = 4096
    (50, 141, 17),   # 4097
    (100, 181, 43),  # 16383
    (100, 5261, 3),  # 16383
    (100, 824, 16),  # 16384
]
GRID_B = (1, 8, 1023, 1024, 1025, 1032, 2047, 2048, 2049, 4095, 4096, 4097, 8192)


def plain_lanes(A, D, B):
    """env_threads (env_kernels.hip), the full-write launches' rule, restated."""
    n = A * D
    if n >= 16384:
        return 512
    if n > 4096:
        return 256 if B <= 1024 else 128
    return 128 if B <= 1024 else 64


def delta_lanes(A, D, B, int8=False):
    """env_delta_threads (env_kernels.hip), the rule of the launches with an obs shadow, restated: 256 lanes for
    int32 observations of A * D >= 16384 at every B (no B threshold: 256 lanes won at 1024, 2048 and 4096 envs of
    uf200, profiles/r10/ab_widths.txt); the plain rule's width for int8 and for smaller shapes."""
    if A * D >= DELTA_MIN_ELEMS and not int8:
        return 256
    return plain_lanes(A, D, B)


def desc(V, C, A, B, int8=False):
    from marlsat import _lib

    return _lib.EnvDesc(num_envs=B, num_vars=V, num_clauses=C, clause_width=3, num_agents=A,
                        max_vars_per_agent=-(-V // A), max_steps=512, action_mode=0, reward_mode=0,
                        obs_dtype=1 if int8 else 0, num_problems=1, r_clause=0.0, r_sat=1.0, gamma=0.99)


def host_widths(forced):
    """Both exports over the grid: the restated rules, or `forced` for every desc."""
    from marlsat import _lib

    seen = set()
    for V, C, A in GRID:
        for B in GRID_B:
            for int8 in (False, True):
                d = desc(V, C, A, B, int8)
                got = _lib.lib.msat_env_delta_launch_threads(ctypes.byref(d))
                plain = _lib.lib.msat_env_launch_threads(ctypes.byref(d))
                D = 2 * V + C
                assert got == (forced or delta_lanes(A, D, B, int8)), (V, C, A, B, int8, got)
                assert plain == (forced or plain_lanes(A, D, B)), (V, C, A, B, int8, plain)
                seen.add((got, plain))
    return seen


# ------------------------------------------------------------------------------------------------ GPU rollouts --
def _imports():
    import torch

    import env_step_chain_worker as W

    return torch, W, W.E


def _desc_of(env, B, pool):
    return env._desc(B, pool)


def delta_rollout(V, C, vpa, B, autoreset, want_T, *, steps=12, obs_delta=None, offset=0, action_mode=0, max_steps=4,
                  sample=None, noop_at=(), dense_at=(), seed=0, N=4):
    """reset -> `steps` delta steps into ONE obs tensor (the shadow belongs to the tensor), each against the oracle:
    obs (all envs, or the rows of `sample`), outputs and state.  noop_at: steps whose actions flip nothing (after a
    sentinel fill nothing may be stored, unless the env resets); dense_at: mode-1 steps flipping half the variables
    (past the quarter rule: whole blocks)."""
    torch, W, E = _imports()
    from marlsat import _lib

    env, ora = E._mk(V, C, vpa, max_steps=max_steps, action_mode=action_mode)
    A, M = env.num_agents, env.max_vars_per_agent
    pool = E._pool(V, C, N, seed0=700 + seed)
    dpool = env.make_pool(pool)
    got = _lib.lib.msat_env_delta_launch_threads(_desc_of(env, B, dpool))
    assert got == want_T, f"V{V} C{C} A{A} B{B}: msat_env_delta_launch_threads = {got}, want {want_T}"
    if obs_delta is None:
        assert env.obs_delta_default() == (A * env.obs_dim >= DELTA_MIN_ELEMS)
    rng = np.random.default_rng(900 + seed + B)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs = W._obs_buffer(env, B, offset)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs)
    s = np.arange(B) if sample is None else np.asarray(sample)
    full = sample is None
    _, ost = ora.reset(pool[pidx[s]], x[s].astype(np.int32))
    if not full:  # staggered counters: the sampled envs time out at different launches
        c0 = (np.arange(B) % max_steps).astype(np.int32)
        st.step.copy_(W._cuda(c0))
        st.invalidate_reset_queue()
        ost.step = c0[s].copy()
    sdev = torch.from_numpy(s).cuda()
    sparse = whole = 0
    for t in range(steps):
        ctx = f"V{V} C{C} A{A} B{B} T{want_T} autoreset={autoreset} mode={action_mode} off={offset} t={t}"
        if action_mode == 0:
            a = rng.integers(0, M + 1, (B, A))
            a = np.where(rng.random((B, A)) < 0.6, M, a).astype(np.int32)
            if t in noop_at:
                a[:] = M
        else:
            p = 0.5 if t in dense_at else (0.0 if t in noop_at else 0.03)
            a = (rng.random((B, A, M)) < p).astype(np.int32)
        kw = {}
        if autoreset:
            npidx = rng.integers(0, N, B).astype(np.int32)
            nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
            kw = dict(autoreset=True, problem_idx=npidx, assignments=nx)
        prev = ost
        _, out = env.step_raw(st, W._cuda(a), obs=obs, obs_delta=obs_delta, **kw)
        if autoreset:
            oobs, ost, r, d, info = ora.step_autoreset(ost, a[s], pool[npidx[s]], nx[s].astype(np.int32))
        else:
            oobs, ost, r, d, info = ora.step(ost, a[s])
        flips = ((prev.variable_assignments != ost.variable_assignments).sum(1) +
                 (prev.clauses_satisfied_status != ost.clauses_satisfied_status).sum(1))
        sparse += int((4 * flips <= V + C).sum())
        whole += int((4 * flips > V + C).sum())
        np.testing.assert_array_equal(E._np(obs[sdev]), oobs, err_msg=ctx)
        for f, cast in W.OUT:
            g = E._np(out[f])[s]
            np.testing.assert_array_equal(g.astype(cast) if cast else g, {"reward": r, "done": d}.get(f, info.get(f)),
                                          err_msg=f"{ctx} out.{f}")
        if full:
            E._check_state(env, st, ost, ctx)
        else:
            np.testing.assert_array_equal(E._np(st.variable_assignments)[s], ost.variable_assignments, err_msg=ctx)
            np.testing.assert_array_equal(E._np(st.clauses_satisfied_status)[s].astype(bool),
                                          ost.clauses_satisfied_status, err_msg=ctx)
            np.testing.assert_array_equal(E._np(st.step)[s], ost.step, err_msg=ctx)
        if t in noop_at and not autoreset and full:
            # nothing changed (a finished env keeps its state as well): a second no-op step must store nothing
            SENT = 7
            obs.fill_(SENT)
            _, out = env.step_raw(st, W._cuda(a), obs=obs, obs_delta=obs_delta)
            before = ost
            oobs, ost, r, d, info = ora.step(ost, a)
            np.testing.assert_array_equal(ost.variable_assignments, before.variable_assignments)
            assert (E._np(obs) == SENT).all(), ctx + ": an all-no-op step stored something"
            env.invalidate_obs(obs)
            env.step_raw(st, W._cuda(a), obs=obs, obs_delta=obs_delta)
            oobs, ost, r, d, info = ora.step(ost, a)
            np.testing.assert_array_equal(E._np(obs), oobs, err_msg=ctx + " restored")
    return sparse, whole


def natural_group(small_only=False):
    """The delta rule's own widths, no override: 12-step rollouts with autoreset on and off.  SATEnv derives the agent
    count from vars_per_agent (A = ceil(V / vpa)), so A * D = 16384 with 16 agents is (96, 832, 6) and 16383 with 43
    agents is (86, 209, 2)."""
    cases = [
        # V, C, vpa, A, B, forced delta
        (200, 860, 8, 25, 16, None),   # uf200, 25 agents: the bench's shape
        (96, 832, 6, 16, 8, None),     # A * D = 16384: the first shape of the delta rule
        (86, 209, 2, 43, 8, True),     # A * D = 16383: the last shape of the plain rule (forced delta)
    ]
    for V, C, vpa, A, B, od in cases[:1] if small_only else cases:
        D = 2 * V + C
        assert -(-V // vpa) == A
        for autoreset in (True, False):
            delta_rollout(V, C, vpa, B, autoreset, delta_lanes(A, D, B), obs_delta=od, seed=A)


# forced widths, forced delta: shapes that break a wrong task index (U = chunk tasks per agent row, obs_sparse.h)
def forced_group(T):
    torch, W, E = _imports()
    shapes = [
        (20, 91, 10),     # 2 agents: A * U < T at every width
        (64, 2080, 32),   # 2 agents, D = 2208: more tasks per agent row than 64 lanes
        (96, 832, 6),     # 16 agents, U = 3 + 26 + 3 = 32: A * U = 512, a multiple of every width
        (33, 70, 3),      # 11 agents, rem == 0, source-word ends in mid-chunk
    ]
    for i, (V, C, vpa) in enumerate(shapes):
        for offset in (0, 1, 2, 3):  # a sliced obs tensor: block bases misaligned by 1-3 elements
            if offset > 1 and i in (1, 2):  # (the large shapes: aligned and off by one only)
                continue
            # mode 0: sparse steps and an all-no-op step that stores nothing
            delta_rollout(V, C, vpa, 8, False, T, steps=4, obs_delta=True, offset=offset, max_steps=64, noop_at=(2,),
                          seed=10 * i + offset)
        # mode 1 across the quarter rule in both directions
        sp, wh = delta_rollout(V, C, vpa, 8, False, T, steps=5, obs_delta=True, offset=1, action_mode=1, max_steps=64,
                               dense_at=(1, 3), seed=50 + i)
        assert sp >= 1 and wh >= 1, (sp, wh)
    # reset workgroups, in-workgroup resets, a solved env and running envs in one launch
    W.paths_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", type=int)
    ap.add_argument("--natural", action="store_true")
    ap.add_argument("--forced", type=int)
    ap.add_argument("--debug", action="store_true")
    args = ap.parse_args()
    from marlsat import _lib

    if args.host is not None:
        assert host_widths(args.host) == {(args.host, args.host)}
        print(f"delta width host forced {args.host} ok")
        return
    import torch

    if args.natural:
        natural_group()
        torch.cuda.synchronize()
        print("delta width natural ok")
    elif args.debug:
        assert _lib.LIB_PATH.endswith("libmarlsat_debug.so"), _lib.LIB_PATH
        natural_group(small_only=True)
        torch.cuda.synchronize()
        print("delta width debug ok", _lib.LIB_PATH)
    else:
        forced_group(args.forced)
        torch.cuda.synchronize()
        print(f"delta width forced {args.forced} ok")


if __name__ == "__main__":
    main()
