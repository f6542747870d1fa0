"""The checks of tests/test_env_static_shape_gpu.py, runnable as a child process (MARLSAT_ENV_STATIC and MARLSAT_LIB are
read once per process):

    python env_static_shape_worker.py --host              (no GPU: msat_env_static_shape over the dispatch descs)
    python env_static_shape_worker.py --dump F [--debug]  (every case, or the debug library's two; arrays -> F.npz)

A delta step of uf200-860 with 25 agents and int32 observations takes shadow::env_kernel<.., StaticShape<200, 860, 25>>
(env_kernels.hip, takes_static_shape) unless MARLSAT_ENV_STATIC=0.  Every case steps that geometry at a small batch
against the NumPy oracle -- observations, outputs, state -- and records, after every launch, the whole obs tensor, the
shadow rows, every step output and every state array; the test compares the records of a default process and of a
MARLSAT_ENV_STATIC=0 process bitwise.  A case that fails is recorded under its name, and the others still run.
Not collected by pytest (no test_ prefix)."""
import argparse
import ctypes
import json
import os
import traceback

import numpy as np

import conftest  # noqa: F401  (puts the repository root and the package on sys.path)

UF200 = (200, 860, 8)  # 25 agents
# V, C, vars per agent, int8: the descs a static kernel must NOT take (20 agents; C + 1; V - 1; int8 observations)
NEIGHBOURS = {"a20": (200, 860, 10, False), "c861": (200, 861, 8, False), "v199": (199, 860, 8, False),
              "int8": (200, 860, 8, True)}


def static_on():
    return os.environ.get("MARLSAT_ENV_STATIC") != "0"


def host_dispatch():
    """msat_env_static_shape: 1 for (200, 860, 25) int32 exactly when the switch is on, 0 for every neighbour."""
    from marlsat import _lib

    import env_delta_width_worker as DW

    f = _lib.lib.msat_env_static_shape
    for B in (1, 2, 12, 4096):
        assert f(ctypes.byref(DW.desc(200, 860, 25, B))) == int(static_on()), B
        for V, C, A in ((200, 860, 20), (200, 861, 25), (199, 860, 25), (200, 860, 10), (100, 430, 10), (20, 91, 2)):
            assert f(ctypes.byref(DW.desc(V, C, A, B))) == 0, (V, C, A, B)
        assert f(ctypes.byref(DW.desc(200, 860, 25, B, int8=True))) == 0, B
    narrow = DW.desc(200, 860, 25, 8)
    narrow.clause_width = 2
    assert f(ctypes.byref(narrow)) == 0
    bad = DW.desc(200, 860, 25, 8)
    bad.num_vars = 0
    assert f(ctypes.byref(bad)) == 0
    assert f(None) == 0


# ------------------------------------------------------------------------------------------------------ rollouts --
def _imports():
    import torch

    import env_step_chain_worker as W

    return torch, W, W.E


class Record:
    """name -> array of everything a launch left behind."""

    def __init__(self):
        self.arrays = {}

    def take(self, tag, st, obs, out):
        _, W, E = _imports()
        a = self.arrays
        a[f"{tag}.obs"] = E._np(obs).copy()
        sh = getattr(obs, "_marlsat_shadow", None)
        if sh is not None and sh.words is not None:
            a[f"{tag}.shadow"] = E._np(sh.words).copy()
        for f, _ in W.OUT:
            a[f"{tag}.out.{f}"] = E._np(out[f]).copy()
        for f in W.STATE_FIELDS:
            a[f"{tag}.state.{f}"] = E._np(getattr(st, f)).copy()
        if st.reset_queue is not None:
            a[f"{tag}.state.reset_queue"] = E._np(st.reset_queue).copy()


def _expect_static(env, B, dpool, want):
    from marlsat import _lib

    got = _lib.lib.msat_env_static_shape(env._desc(B, dpool))
    assert got == int(want), f"msat_env_static_shape = {got}, want {int(want)}"


def rollout(rec, name, B, *, steps=4, autoreset=True, max_steps=64, action_mode=0, reward_mode=0, offset=0,
            fresh=False, dense_at=(), counters=None, planted=None, shape=UF200, obs_dtype=None, seed=0, N=4):
    """reset -> `steps` delta steps into one obs tensor, each against the oracle and recorded.  fresh: the tensor the
    steps write was never reset into (sentinel-filled: the first step writes every element); counters: step counters
    planted before the first launch; planted: an env put one flip away from its instance's planted solution, solved
    by its step 1."""
    torch, W, E = _imports()
    from marlsat.utils.generate_cnf_dataset import generate_sat_solution

    V, C, vpa = shape
    kw = {} if obs_dtype is None else {"obs_dtype": obs_dtype}
    env, ora = E._mk(V, C, vpa, max_steps=max_steps, action_mode=action_mode, reward_mode=reward_mode, **kw)
    A, M = env.num_agents, env.max_vars_per_agent
    seed0 = 1600 + 10 * seed
    pool = E._pool(V, C, N, seed0=seed0)
    dpool = env.make_pool(pool)
    _expect_static(env, B, dpool, shape == UF200 and obs_dtype is None and static_on())
    rng = np.random.default_rng(1700 + seed)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    solver = None
    if planted is not None:
        sol = generate_sat_solution(V, seed0 + int(pidx[planted])).astype(np.int32)
        assert ora.satisfaction(sol[None], pool[pidx[planted]][None])[1][0] == 0
        for v in range(V):  # a variable whose flip breaks a clause
            y = sol.copy()
            y[v] ^= 1
            if ora.satisfaction(y[None], pool[pidx[planted]][None])[1][0] > 0:
                break
        x[planted] = y
        agent = int(E._np(env.variable_to_agent_idx)[v])
        solver = (agent, int(np.nonzero(E._np(env.agent_vars)[agent] == v)[0][0]))
    obs = W._obs_buffer(env, B, offset)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=env.alloc_obs(B) if fresh else obs)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    if fresh:
        obs.fill_(7)
    if counters is not None:
        st.step.copy_(W._cuda(np.asarray(counters, np.int32)))
        st.invalidate_reset_queue()
        ost.step[:] = np.asarray(counters, np.int32)
    sparse = whole = resets = solved = 0
    for t in range(steps):
        ctx = f"{name} B{B} t={t}"
        if action_mode == 0:
            a = np.where(rng.random((B, A)) < 0.6, M, rng.integers(0, M + 1, (B, A))).astype(np.int32)
            if solver is not None and t < 2:
                a[planted] = M
                if t == 1:
                    a[planted, solver[0]] = solver[1]
        else:
            a = (rng.random((B, A, M)) < (0.5 if t in dense_at else 0.03)).astype(np.int32)
        prev = ost
        if autoreset:
            npidx = rng.integers(0, N, B).astype(np.int32)
            nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
            _, out = env.step_raw(st, W._cuda(a), autoreset=True, problem_idx=npidx, assignments=nx, obs=obs,
                                  obs_delta=True)
            oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[npidx], nx.astype(np.int32))
        else:
            _, out = env.step_raw(st, W._cuda(a), obs=obs, obs_delta=True)
            oobs, ost, r, d, info = ora.step(ost, a)
        flips = ((prev.variable_assignments != ost.variable_assignments).sum(1) +
                 (prev.clauses_satisfied_status != ost.clauses_satisfied_status).sum(1))
        sparse += int((4 * flips <= V + C).sum())
        whole += int((4 * flips > V + C).sum())
        resets += int(np.asarray(d).sum())
        solved += int(np.asarray(info["solved"]).sum())
        rec.take(f"{name}.{t}", st, obs, out)
        np.testing.assert_array_equal(E._np(obs), oobs, err_msg=ctx)
        W._check_out(out, r, d, info, ctx)
        E._check_state(env, st, ost, ctx)
        np.testing.assert_array_equal(E._np(st.clause_ntrue),
                                      ora.num_true_literals(ost.variable_assignments, ost.clauses), err_msg=ctx)
    return dict(sparse=sparse, whole=whole, resets=resets, solved=solved)


def two_states(rec, name, invalidate_at=None, B=8):
    """Two states of different instances stepped in turn into one fresh tensor: every launch finds shadow rows that
    name another instance's state and writes whole blocks; then one state alone (sparse steps).  invalidate_at: the
    tensor overwritten and invalidate_obs before that launch."""
    torch, W, E = _imports()
    V, C, vpa = UF200
    N = 4
    env, ora = E._mk(V, C, vpa, max_steps=64)
    A, M = env.num_agents, env.max_vars_per_agent
    pool = E._pool(V, C, N, seed0=1810)
    dpool = env.make_pool(pool)
    _expect_static(env, B, dpool, static_on())
    rng = np.random.default_rng(31)
    states = []
    for k in range(2):
        pidx = ((np.arange(B) + k) % N).astype(np.int32)  # never the instance of the other state's env
        x = rng.integers(0, 2, (B, V)).astype(np.uint8)
        _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=env.alloc_obs(B))
        _, ost = ora.reset(pool[pidx], x.astype(np.int32))
        states.append([st, ost])
    obs = W._obs_buffer(env, B, 2)
    obs.fill_(7)
    for t, k in enumerate((0, 1, 0, 1, 1, 1)):
        st, ost = states[k]
        a = np.where(rng.random((B, A)) < 0.6, M, rng.integers(0, M + 1, (B, A))).astype(np.int32)
        if t == invalidate_at:
            obs.fill_(7)
            env.invalidate_obs(obs)
        _, out = env.step_raw(st, W._cuda(a), obs=obs, obs_delta=True)
        oobs, ost, r, d, info = ora.step(ost, a)
        states[k][1] = ost
        ctx = f"{name} t={t} state {k}"
        rec.take(f"{name}.{t}", st, obs, out)
        np.testing.assert_array_equal(E._np(obs), oobs, err_msg=ctx)
        W._check_out(out, r, d, info, ctx)
        E._check_state(env, st, ost, ctx)


# ------------------------------------------------------------------------------------------------------- cases --
def case_running_warm(rec):
    for B in (1, 3, 8, 12):
        got = rollout(rec, f"running_warm{B}", B, steps=3, seed=B)
        assert got["sparse"] >= B, got


def case_first_step_fresh(rec):
    rollout(rec, "first_step_fresh", 3, steps=2, fresh=True, seed=21)


def case_two_states_one_tensor(rec):
    two_states(rec, "two_states")


def case_invalidate_obs(rec):
    two_states(rec, "invalidate", invalidate_at=4, B=3)


def case_timeouts(rec):
    """B = 8 = rq_cap, max_steps 4, counters planted: envs 0-2 time out in launch 1 (their marks made by launch 0:
    reset workgroups and covered envs), envs 3-4 in launch 2, the others later; six launches."""
    got = rollout(rec, "timeouts", 8, steps=6, max_steps=4, counters=[2, 2, 2, 1, 1, 0, 0, 0], seed=22)
    assert got["resets"] >= 8, got


def case_whole_batch_timeout(rec):
    """B = 12 > rq_cap = 8, max_steps 3: the whole batch times out in launches 2 and 5, ranks 8-11 reset in their
    own workgroup."""
    from marlsat import _lib

    assert _lib.lib.msat_reset_queue_words(12) == 24
    got = rollout(rec, "whole_batch", 12, steps=6, max_steps=3, seed=23)
    assert got["resets"] >= 24, got


def case_solved(rec):
    got = rollout(rec, "solved", 8, steps=3, planted=5, seed=24)
    assert got["solved"] >= 1 and got["resets"] >= 1, got


def case_action_mode1(rec):
    got = rollout(rec, "action_mode1", 3, steps=5, action_mode=1, dense_at=(1, 3), seed=25)
    assert got["sparse"] >= 1 and got["whole"] >= 1, got


def case_pbrs(rec):
    rollout(rec, "pbrs", 8, steps=4, max_steps=3, reward_mode=1, seed=26)


def case_no_autoreset(rec):
    rollout(rec, "no_autoreset", 3, steps=4, autoreset=False, max_steps=3, seed=27)
    rollout(rec, "no_autoreset_mode1", 3, steps=3, autoreset=False, action_mode=1, dense_at=(1,), seed=28)


def case_misaligned(rec):
    rollout(rec, "misaligned", 3, steps=4, max_steps=3, offset=1, seed=29)


def case_neighbours(rec):
    """The descs next to the compiled shape: msat_env_static_shape is 0 (rollout asserts it) and one step of B = 2
    on the kernel of any shape equals the oracle."""
    import torch

    for i, (key, (V, C, vpa, int8)) in enumerate(sorted(NEIGHBOURS.items())):
        rollout(rec, f"neighbour_{key}", 2, steps=1, shape=(V, C, vpa), obs_dtype=torch.int8 if int8 else None,
                seed=30 + i)


CASES = {k[5:]: v for k, v in sorted(globals().items()) if k.startswith("case_")}
DEBUG_CASES = ("running_warm", "timeouts")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--dump")
    ap.add_argument("--debug", action="store_true")
    args = ap.parse_args()
    from marlsat import _lib

    if args.host:
        host_dispatch()
        print(f"static shape host ok static={int(static_on())}")
        return
    import torch

    if args.debug:
        assert _lib.LIB_PATH.endswith("libmarlsat_debug.so"), _lib.LIB_PATH
    rec, status = Record(), {}
    for name in DEBUG_CASES if args.debug else CASES:
        try:
            CASES[name](rec)
            torch.cuda.synchronize()
            status[name] = "ok"
        except AssertionError:  # a mismatch is recorded: the test of this case fails, the others still run
            status[name] = traceback.format_exc()[-3000:]
        except Exception:  # anything else (a device error among them) ends the run: nothing more is launched
            print(f"case {name}:\n{traceback.format_exc()[-3000:]}")
            raise SystemExit(3)
    np.savez(args.dump, **rec.arrays)
    print("STATUS " + json.dumps(status))
    print(f"static shape cases done static={int(static_on())}", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
