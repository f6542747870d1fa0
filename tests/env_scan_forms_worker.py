"""The checks of tests/test_env_scan_forms_gpu.py, run as a child process of that test:

    python env_scan_forms_worker.py --group edges --threads T   (MARLSAT_ENV_THREADS=T, MARLSAT_OBS_DELTA=2)
    python env_scan_forms_worker.py --group forms | paths | scatter      (MARLSAT_OBS_DELTA=2)
    python env_scan_forms_worker.py --group debug   (MARLSAT_LIB=libmarlsat_debug.so: bounds checks and read-back)

MARLSAT_ENV_THREADS, MARLSAT_OBS_DELTA and MARLSAT_LIB are read once per process, hence the child.  The cases are the
ones at which a literal read of the clause scan or of the scatter can go wrong (marl-sat_amd/csrc/env_kernels.hip:
clause_slice, eval_clauses, scatter_clause, scatter_obs): NULL and ABSENT codes, lanes past C, slices on both sides
of the prefetch's end, repeated variables, every path that shares the scan.  Every comparison
here is bitwise against the NumPy oracle over short auto-reset rollouts -- assignment, clause status, clause_ntrue,
unsatisfied count, reward / done / solved and the whole obs block.  Each group prints one line per case (tag + what
ran) and "scan forms <group> ok" at the end.  Not collected by pytest (no test_ prefix)."""
import argparse
import itertools

import numpy as np
import torch

import conftest  # noqa: F401  (puts the repository root and the package on sys.path)
import irregular_pools as IP
import test_env_gpu as E

SENTINEL = 7
MAX_STEPS = 3


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ntrue_of(clauses, x):
    """(B, C, K) literals, (B, V) assignment -> (B, C) true literals per clause: literal l is true iff l > 0 and x = 1
    or l < 0 and x = 0; literal 0 never; a variable that stands twice counts twice."""
    cl = np.asarray(clauses)
    xv = np.asarray(x)[np.arange(cl.shape[0])[:, None, None], np.maximum(np.abs(cl) - 1, 0)]
    return (((cl > 0) & (xv == 1)) | ((cl < 0) & (xv == 0))).sum(-1).astype(np.uint8)


def check(st, ost, obs, oobs, ctx, out=None, r=None, d=None, info=None):
    np.testing.assert_array_equal(_np(st.variable_assignments), ost.variable_assignments, err_msg=ctx + " x")
    np.testing.assert_array_equal(_np(st.clauses_satisfied_status).astype(bool), ost.clauses_satisfied_status,
                                  err_msg=ctx + " clause status")
    np.testing.assert_array_equal(_np(st.clause_ntrue), ntrue_of(ost.clauses, ost.variable_assignments),
                                  err_msg=ctx + " clause_ntrue")
    np.testing.assert_array_equal(_np(st.num_unsatisfied), ost.num_unsatisfied, err_msg=ctx + " unsat count")
    if obs is not None:
        np.testing.assert_array_equal(_np(obs).astype(np.int32), oobs, err_msg=ctx + " obs")
    if out is not None:
        np.testing.assert_array_equal(_np(out["reward"]), r, err_msg=ctx + " reward")  # fp32, the reference's op order
        np.testing.assert_array_equal(_np(out["done"]).astype(bool), d, err_msg=ctx + " done")
        np.testing.assert_array_equal(_np(out["solved"]).astype(bool), info["solved"], err_msg=ctx + " solved")
        np.testing.assert_array_equal(_np(out["num_unsatisfied"]), info["num_unsatisfied"], err_msg=ctx + " out unsat")


def make_actions(rng, env, B, t, idle):
    A, M = env.num_agents, env.max_vars_per_agent
    if env.action_mode == 0:
        if t == 1:  # a no-op step: index M flips nothing (an env that did not just reset changes no element)
            return np.full((B, A), M, np.int32)
        a = rng.integers(0, M + 1, size=(B, A))
        return np.where(rng.random((B, A)) < idle, M, a).astype(np.int32)
    # mode 1: dense on even steps (past the quarter rule: the full write), a few flips on odd ones
    return (rng.random((B, A, M)) < (0.5 if t % 2 == 0 else 0.05)).astype(np.int32)


def rollout(tag, V, C, vpa, pool, B, delta, steps=6, idle=0.6, offset=0, seed=0, **kw):
    """reset + `steps` auto-reset steps with explicit reset inputs, max_steps = 3: envs time out (B % 4 == 0: the reset
    queue is on, so they reset in workgroups of their own, their step workgroups scan with NULL clause-state pointers)
    and solved envs reset in their own workgroup.  delta None: the process default (MARLSAT_OBS_DELTA=2 forces the
    delta write); False: whole blocks.  Returns (resets, solved, sparse steps, full-write steps of live envs)."""
    env, ora = E._mk(V, C, vpa, max_steps=MAX_STEPS, **kw)
    N = pool.shape[0]
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(100 + seed)
    pidx = (np.arange(B) % N).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    n = B * env.num_agents * env.obs_dim
    obs = torch.empty(n + offset, dtype=env.obs_dtype, device="cuda")[offset:].view(B, env.num_agents, env.obs_dim)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs)
    oobs, ost = ora.reset(pool[pidx], x.astype(np.int32))
    check(st, ost, obs, oobs, f"{tag} reset")
    resets = solved = few = many = 0
    for t in range(steps):
        a = make_actions(rng, env, B, t, idle)
        npidx = rng.integers(0, N, B).astype(np.int32)
        nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
        _, out = env.step_raw(st, _cuda(a), autoreset=True, problem_idx=npidx, assignments=nx, obs=obs, obs_delta=delta)
        prev = ost
        oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[npidx], nx.astype(np.int32))
        check(st, ost, obs, oobs, f"{tag} t={t}", out, r, d, info)
        flips = (prev.variable_assignments != ost.variable_assignments).sum(1) + \
            (prev.clauses_satisfied_status != ost.clauses_satisfied_status).sum(1)
        if t > 0:
            few += int((~d & (4 * flips <= V + C)).sum())
            many += int((~d & (4 * flips > V + C)).sum())
        resets += int(d.sum())
        solved += int(np.asarray(info["solved"]).sum())
    # obs only: the same observation from the state alone, the state untouched
    np.testing.assert_array_equal(_np(env.get_obs(st).tensor).astype(np.int32), oobs, err_msg=tag + " get_obs")
    check(st, ost, None, None, tag + " after get_obs")
    print(f"{tag}: resets {resets} solved {solved} sparse {few} full {many}", flush=True)
    return resets, solved, few, many


# ------------------------------------------------------------------ edges ----
# the prefetch covers 4 x T clauses, a slice 64: C on both sides of a slice and of the prefetch's end; V = 21 (not a
# multiple of 32), agents of 5, 4, 4, 4, 4 variables
EDGE_C = {64: (1, 63, 64, 65, 255, 256, 257, 321), 256: (1100,), 512: (600,)}
EDGE_V = {64: (21, 5), 256: (70, 7), 512: (70, 7)}


def edges_group(T):
    from marlsat import _lib

    V, vpa = EDGE_V[T]
    for C in EDGE_C[T]:
        pool = E._pool(V, C, 3, seed0=4000 + C)
        for dt, delta in ((torch.int32, None), (torch.int8, None), (torch.int32, False)):
            env, _ = E._mk(V, C, vpa, obs_dtype=dt)
            desc = env._desc(8, env.make_pool(pool))
            got = (_lib.lib.msat_env_launch_threads if delta is False else _lib.lib.msat_env_delta_launch_threads)(desc)
            assert got == T, f"launch width {got}, forced {T}"
            tag = f"edges T={T} C={C} {str(dt)[6:]} {'full' if delta is False else 'delta'}"
            resets, _, few, _ = rollout(tag, V, C, vpa, pool, 8, delta, obs_dtype=dt, offset=C % 4, seed=C)
            assert resets >= 8, tag
            assert delta is False or few >= 1, tag


# ------------------------------------------------------------------ forms ----
def forms_group(names=("quirks23", "k2", "k1", "solo"), dtypes=(torch.int32, torch.int8)):
    """tests/irregular_pools.py: literal 0, a variable twice in a clause (same sign and both), an all-zero clause, 2-
    and 1-wide clauses (ABSENT slots), variables in no clause; quirks23 has agents of 8, 8 and 7 variables (rem = 2 > 0)
    and literal 0 rows: every agent i >= rem is related to those clauses."""
    for name in names:
        ip = IP.get(name)
        for dt, delta in itertools.chain(((d, None) for d in dtypes), ((torch.int32, False),)):
            tag = f"forms {name} {str(dt)[6:]} {'full' if delta is False else 'delta'}"
            resets, _, few, _ = rollout(tag, ip.V, ip.C, ip.vpa, ip.pool, 8, delta, obs_dtype=dt, idle=0.5, offset=1)
            assert resets >= 8, tag
            assert delta is False or few >= 1, tag


# ------------------------------------------------------------------ paths ----
def solved_env_case(delta):
    """An env one flip away from a satisfying assignment (brute force over V = 12): the step solves it, and it resets
    in its own workgroup (solved, not timed out)."""
    V, C, vpa, B = 12, 40, 4, 4
    pool = E._pool(V, C, 2, seed0=4100)
    allx = ((np.arange(1 << V)[:, None] >> np.arange(V)) & 1).astype(np.int32)
    sol = []
    for n in range(2):
        nt = ntrue_of(np.broadcast_to(pool[n], (1 << V,) + pool[n].shape), allx)
        good = np.flatnonzero((nt > 0).all(1))
        assert len(good), "the generator plants a solution"
        sol.append(allx[good[0]])
    env, ora = E._mk(V, C, vpa, max_steps=50)
    pidx = np.array([0, 1, 0, 1], np.int32)
    x = np.stack([sol[i] for i in pidx]).astype(np.uint8)
    x[:, 5] ^= 1  # variable 5 = agent 1's local 1
    obs, st = env.reset_from_pool(env.make_pool(pool), B, problem_idx=pidx, assignments=x)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    a = np.full((B, env.num_agents), env.max_vars_per_agent, np.int32)
    a[:2, 1] = 1  # envs 0 and 1 flip it back; 2 and 3 idle
    rng = np.random.default_rng(9)
    for t in range(2):
        nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
        _, out = env.step_raw(st, _cuda(a), autoreset=True, problem_idx=pidx[::-1].copy(), assignments=nx, obs=obs,
                              obs_delta=delta)
        oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[pidx[::-1]], nx.astype(np.int32))
        check(st, ost, obs, oobs, f"solved t={t}", out, r, d, info)
        if t == 0:
            assert np.asarray(info["solved"]).tolist() == [True, True, False, False]
        a[:] = env.max_vars_per_agent
    print("paths solved env: ok", flush=True)


def single_agent_case():
    """The single-agent env: the delta reward and the state-only step (NULL obs) on a pool with quirk rows."""
    from marlsat.envs.sat_env import SatEnv
    from oracle.single_env import OracleSatEnv

    ip = IP.get("quirks23")
    B = 8
    pool = ip.pool[np.arange(B) % len(ip.pool)]
    rng = np.random.default_rng(3)
    x0 = rng.integers(0, 2, (B, ip.V)).astype(np.int32)
    env = SatEnv(ip.V, ip.C, max_clause_len=3, c_bonus=2.5, max_steps=MAX_STEPS)
    _, st = env.reset(None, pool, assignments=x0)
    ora = OracleSatEnv(ip.V, ip.C, 3, c_bonus=2.5, max_steps=MAX_STEPS)
    ost = ora.reset(pool, x0)
    for t in range(6):
        a = rng.integers(-ip.V - 2, ip.V + 2, B).astype(np.int32)
        _, st, rew, dones, _ = env.step_env(None, st, {"agent_0": torch.from_numpy(a)})
        ost, r, d = ora.step(ost, a)
        ctx = f"single t={t}"
        np.testing.assert_array_equal(_np(st.variable_assignments), ost["x"], err_msg=ctx)
        nt = ntrue_of(pool, ost["x"])
        np.testing.assert_array_equal(_np(st.clause_ntrue), nt, err_msg=ctx)
        np.testing.assert_array_equal(_np(st.clauses_satisfied_status), (nt > 0).astype(np.uint8), err_msg=ctx)
        np.testing.assert_array_equal(_np(st.num_unsatisfied), (nt == 0).sum(1), err_msg=ctx)
        np.testing.assert_array_equal(_np(rew["agent_0"]), r, err_msg=ctx)
        np.testing.assert_array_equal(_np(dones["__all__"]), d, err_msg=ctx)
    print("paths single agent: ok", flush=True)


def grouped_case():
    """Two small classes in one grouped launch against the oracle, RNG resets replayed with the class seeds."""
    from marlsat.envs.mixed import MixedSATEnv, group_seed
    from marlsat.random import Key
    from oracle.rng import reset_draws

    ips = [IP.get("quirks23"), IP.get("k2")]
    sizes = [8, 12]
    classes, oras = zip(*(E._mk(ip.V, ip.C, ip.vpa, max_steps=MAX_STEPS) for ip in ips))
    mixed = MixedSATEnv(list(classes))
    key = Key(0x77, 1)
    obs, states = mixed.reset([c.make_pool(ip.pool) for c, ip in zip(classes, ips)], sizes, key)
    osts = []
    for g, (ora, ip, B) in enumerate(zip(oras, ips, sizes)):
        p0, x0 = reset_draws(key.seed ^ group_seed(g), key.counter, B, ip.V, len(ip.pool))
        oobs, ost = ora.reset(ip.pool[p0], x0.astype(np.int32))
        check(states[g], ost, obs[g], oobs, f"grouped class {g} reset")
        osts.append(ost)
    outs = mixed.alloc_outs(states)
    seed = 0xBEE
    step = mixed.stepper(states, obs, outs, autoreset=True, seed=seed)
    rng = np.random.default_rng(6)
    done = 0
    for t in range(5):
        acts = [make_actions(rng, c, B, t, 0.5) for c, B in zip(classes, sizes)]
        step([_cuda(a) for a in acts], 30 + t)
        for g, (ora, ip, B) in enumerate(zip(oras, ips, sizes)):
            p2, x2 = reset_draws(seed ^ group_seed(g), 30 + t, B, ip.V, len(ip.pool))
            oobs, osts[g], r, d, info = ora.step_autoreset(osts[g], acts[g], ip.pool[p2], x2.astype(np.int32))
            check(states[g], osts[g], obs[g], oobs, f"grouped class {g} t={t}", outs[g], r, d, info)
            done += int(d.sum())
    assert done >= sum(sizes)
    print("paths grouped: ok", flush=True)


def paths_group(debug=False):
    ip = IP.get("quirks23")
    pool30 = E._pool(30, 126, 4, seed0=50)
    for delta in (None, False):
        w = "full" if delta is False else "delta"
        kw = dict(reward_mode=1, r_clause=0.03, r_sat=5.0, gamma=0.97)  # PBRS: the scan reads the old status byte
        resets, _, _, _ = rollout(f"paths pbrs quirks23 {w}", ip.V, ip.C, ip.vpa, ip.pool, 8, delta, idle=0.5, **kw)
        assert resets >= 8
        if not debug:
            rollout(f"paths pbrs v30c126 mode1 {w}", 30, 126, 7, pool30, 8, delta, action_mode=1, **kw)
        solved_env_case(delta)
    single_agent_case()
    grouped_case()


# ---------------------------------------------------------------- scatter ----
def noop_stores_nothing(name):
    """Steps that change nothing store nothing: the obs tensor keeps a sentinel in every element."""
    ip = IP.get(name)
    env, ora = E._mk(ip.V, ip.C, ip.vpa, max_steps=512)
    B = 8
    pidx = (np.arange(B) % len(ip.pool)).astype(np.int32)
    x = np.random.default_rng(23).integers(0, 2, (B, ip.V)).astype(np.uint8)
    obs = env.alloc_obs(B)
    _, st = env.reset_from_pool(env.make_pool(ip.pool), B, problem_idx=pidx, assignments=x)
    _, ost = ora.reset(ip.pool[pidx], x.astype(np.int32))
    noop = np.full((B, env.num_agents), env.max_vars_per_agent, np.int32)
    env.step_raw(st, _cuda(noop), obs=obs)  # the first step into obs writes it whole
    oobs, ost, _, d, _ = ora.step(ost, noop)
    live = ~d  # (an instance of all-satisfied clauses is done at once)
    np.testing.assert_array_equal(_np(obs), oobs)
    obs.fill_(SENTINEL)
    for _ in range(2):
        env.step_raw(st, _cuda(noop), obs=obs)
        assert (_np(obs)[live] == SENTINEL).all(), f"{name}: a no-op step stored something"
    print(f"scatter noop {name}: ok ({int(live.sum())} live envs)", flush=True)


def scatter_group():
    """The forced delta on the small shapes, action mode 1: steps past the quarter rule (whole blocks) between sparse
    ones, int32 (scatter_obs) and int8 (the chunk write); then the steps that store nothing."""
    for name in ("quirks23", "k2"):
        ip = IP.get(name)
        for dt in (torch.int32, torch.int8):
            tag = f"scatter {name} mode1 {str(dt)[6:]}"
            _, _, few, many = rollout(tag, ip.V, ip.C, ip.vpa, ip.pool, 8, None, obs_dtype=dt, action_mode=1, offset=3)
            assert few >= 1 and many >= 1, (tag, few, many)
    V, C = EDGE_V[64][0], 257
    pool = E._pool(V, C, 3, seed0=4000 + C)
    _, _, few, _ = rollout("scatter C=257 mode1 int32", V, C, EDGE_V[64][1], pool, 8, None, action_mode=1, offset=2)
    assert few >= 1, few
    noop_stores_nothing("quirks23")
    noop_stores_nothing("k2")


def debug_group():
    """One case per group on the debug library: its MSAT_DCHECKs bound every index, and a sparse step's untouched
    elements are read back.  (No sentinel cases: the read-back would see the sentinel.)"""
    V, vpa = EDGE_V[64]
    pool = E._pool(V, 257, 3, seed0=4257)
    rollout("debug edges C=257 int32 delta", V, 257, vpa, pool, 8, None, offset=1)
    forms_group(names=("quirks23", "k1"), dtypes=(torch.int32,))
    paths_group(debug=True)
    ip = IP.get("k2")
    rollout("debug scatter k2 mode1 int32", ip.V, ip.C, ip.vpa, ip.pool, 8, None, action_mode=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", required=True, choices=["edges", "forms", "paths", "scatter", "debug"])
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    from marlsat import _lib
    from marlsat.envs import multi_agent_sat_env as M

    if args.group == "debug":
        assert _lib.LIB_PATH.endswith("libmarlsat_debug.so"), _lib.LIB_PATH
    assert M.OBS_DELTA == 2, "MARLSAT_OBS_DELTA=2 (the delta write for every shape) is this worker's setting"
    {"edges": lambda: edges_group(args.threads), "forms": forms_group, "paths": paths_group, "scatter": scatter_group,
     "debug": debug_group}[args.group]()
    torch.cuda.synchronize()
    print(f"scan forms {args.group} ok {_lib.LIB_PATH}")
