"""Child process of tests/test_env_paths_gpu.py: the env kernels at a forced workgroup size against the oracle.

MARLSAT_ENV_THREADS / MARLSAT_ENV_GROUP_THREADS are read once per process (env_kernels.hip), so every forced size
needs a process of its own: the parent sets the variable and runs

    python env_threads_worker.py --threads T          (MARLSAT_ENV_THREADS=T)
    python env_threads_worker.py --group-threads T    (MARLSAT_ENV_GROUP_THREADS=T)

The worker first asserts that the library reports the forced size (msat_env_launch_threads /
msat_env_group_launch_threads: what the launches use), then compares bitwise with the oracle and exits non-zero at
the first mismatch (an uncaught AssertionError).  Not collected by pytest (no test_ prefix)."""
import argparse

import numpy as np
import torch

import conftest  # noqa: F401  (puts the repository root and the package on sys.path)
import test_env_gpu as E

SHAPES = [  # name, V, C, vars_per_agent
    ("uf20", 20, 91, 10),
    ("uf50", 50, 218, 10),
    ("uf100", 100, 430, 10),
    # T = 64: A*WC = 700 > 4T, A*WV = 200 > 2T, C = 860 > 4T -- every loop behind the prefetch
    ("uf200_a25", 200, 860, 8),
    ("rem23", 23, 97, 10),
    ("one_agent", 12, 40, 12),
    ("a65", 130, 60, 2),  # 65 agents: the action loop's second pass at T = 64, no reset-queue fast path
]


def rollout(T, name, V, C, vpa, B, autoreset, N=6, steps=10):
    """reset -> `steps` steps (max_steps 4: timeouts, and with autoreset their resets), every output and state field
    against the oracle."""
    from marlsat import _lib

    env, ora = E._mk(V, C, vpa, max_steps=4)
    pool = E._pool(V, C, N, seed0=300)
    dpool = env.make_pool(pool)
    got = _lib.lib.msat_env_launch_threads(env._desc(B, dpool))
    assert got == T, f"{name} B={B}: msat_env_launch_threads = {got}, forced {T}"
    rng = np.random.default_rng(1000 * B + T)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x)
    oobs, ost = ora.reset(pool[pidx], x.astype(np.int32))
    ctx = f"{name} T={T} B={B} autoreset={autoreset}"
    np.testing.assert_array_equal(E._np(obs), oobs, err_msg=ctx + " reset")
    E._check_state(env, st, ost, ctx + " reset")
    for t in range(steps):
        a = E._random_actions(rng, env, B)
        if autoreset:
            npidx = rng.integers(0, N, B).astype(np.int32)
            nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
            obs, out = env.step_raw(st, torch.from_numpy(a).cuda(), autoreset=True, problem_idx=npidx, assignments=nx)
            oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[npidx], nx.astype(np.int32))
        else:
            obs, out = env.step_raw(st, torch.from_numpy(a).cuda())
            oobs, ost, r, d, info = ora.step(ost, a)
        c = f"{ctx} t={t}"
        np.testing.assert_array_equal(E._np(obs), oobs, err_msg=c)
        np.testing.assert_array_equal(E._np(out["reward"]), r, err_msg=c)
        np.testing.assert_array_equal(E._np(out["done"]).astype(bool), d, err_msg=c)
        np.testing.assert_array_equal(E._np(out["solved"]).astype(bool), info["solved"], err_msg=c)
        np.testing.assert_array_equal(E._np(out["num_unsatisfied"]), info["num_unsatisfied"], err_msg=c)
        np.testing.assert_array_equal(E._np(out["episode_step"]), info["episode_step"], err_msg=c)
        E._check_state(env, st, ost, c)
        np.testing.assert_array_equal(E._np(st.clause_ntrue), ora.num_true_literals(ost.variable_assignments,
                                                                                     ost.clauses), err_msg=c)


def run_threads(T):
    for name, V, C, vpa in SHAPES:
        for B in (8, 7):  # 8: the reset queue's fast path (B % 4 == 0, fewer than 64 agents); 7: queue only cleared
            for autoreset in (False, True):
                rollout(T, name, V, C, vpa, B, autoreset)
    for reward_mode in (0, 1):
        for action_mode in (0, 1):
            E._modes_rollout(50, 218, 10, 9, 4, reward_mode, action_mode)
    torch.cuda.synchronize()
    print(f"env threads {T} ok")


def run_group_threads(T):
    from marlsat import _lib

    for total in (1, 52, 2048, 2049, 8192):
        got = _lib.lib.msat_env_group_launch_threads(total)
        assert got == T, f"msat_env_group_launch_threads({total}) = {got}, forced {T}"
    E.test_config5_grouped_matches_oracle_per_class()
    E.test_grouped_eight_classes_with_empty_ones()
    torch.cuda.synchronize()
    print(f"env group threads {T} ok")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int)
    ap.add_argument("--group-threads", type=int)
    args = ap.parse_args()
    assert (args.threads is None) != (args.group_threads is None), "give --threads or --group-threads"
    if args.threads is not None:
        run_threads(args.threads)
    else:
        run_group_threads(args.group_threads)
