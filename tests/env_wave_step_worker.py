"""The checks of tests/test_env_wave_step_gpu.py, runnable as a child process (MARLSAT_ENV_THREADS and MARLSAT_LIB are
read once per process):

    python env_wave_step_worker.py --group G [--threads T] [--debug]

The full writes of a launch with an obs shadow, int32 observations and 16-byte groups -- a reset in the step's
workgroup, a reset workgroup, a first write into a fresh tensor, a shadow row that names another instance, a step past
the quarter rule -- stage the instance's tables without a prefetched rel word (env_kernels.hip, PfDepth), and the
sparse steps between them scatter from the prefetched pool and nbr words.  Every group below drives such launches at
the width the process runs at (the delta rule's own, or a forced one) and compares observations, outputs and state
bitwise with the NumPy oracle.  Not collected by pytest (no test_ prefix)."""
import argparse

import numpy as np

import conftest  # noqa: F401  (puts the repository root and the package on sys.path)
import env_delta_width_worker as DW

UF200 = (200, 860, 8)  # 25 agents: the bench's shape, A * D = 31500 (delta by default, the delta rule's width)


def _width(V, C, vpa, B, forced):
    A, D = -(-V // vpa), 2 * V + C
    return forced or DW.delta_lanes(A, D, B)


def small_batches(forced):
    """B = 1, 3, 5, 8 on uf200: fewer envs than a workgroup holds waves, B % 4 != 0 (no reset queue: every reset in
    its step's workgroup), autoreset on and off."""
    V, C, vpa = UF200
    for B in (1, 3, 5, 8):
        DW.delta_rollout(V, C, vpa, B, True, _width(V, C, vpa, B, forced), steps=6, seed=B)
    DW.delta_rollout(V, C, vpa, 5, False, _width(V, C, vpa, 5, forced), steps=4, max_steps=64, noop_at=(2,), seed=9)


def paths(forced):
    """Reset workgroups, in-workgroup resets, a solved env and running envs in one launch (explicit and Philox reset
    inputs); a whole-batch timeout with B = 16 > rq_cap = 8 (ranks 8-15 reset in their step's workgroup), three times
    in twelve launches."""
    _, W, _ = DW._imports()
    W.paths_group()
    V, C, vpa = 70, 33, 9
    DW.delta_rollout(V, C, vpa, 16, True, _width(V, C, vpa, 16, forced), steps=12, obs_delta=True, offset=3,
                     max_steps=4, seed=21)


def _two_states_one_tensor(forced):
    """A first step into a fresh (sentinel-filled) tensor, then two states of different instances stepped in turn into
    that one tensor: every launch finds shadow rows that name another instance's state and writes whole blocks; then
    one state alone again (sparse steps), an invalidate_obs in between."""
    torch, W, E = DW._imports()
    V, C, vpa, B, N = 70, 33, 9, 8, 4
    env, ora = E._mk(V, C, vpa, max_steps=64)
    A, M = env.num_agents, env.max_vars_per_agent
    pool = E._pool(V, C, N, seed0=810)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(31)
    states = []
    for k in range(2):
        pidx = ((np.arange(B) + k) % N).astype(np.int32)  # never the instance of the other state's env
        x = rng.integers(0, 2, (B, V)).astype(np.uint8)
        _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=env.alloc_obs(B))
        _, ost = ora.reset(pool[pidx], x.astype(np.int32))
        states.append([st, ost])
    obs = W._obs_buffer(env, B, 2)
    obs.fill_(7)  # a fresh tensor: no shadow yet, the first step writes every element
    for t, k in enumerate((0, 1, 0, 1, 1, 1, 1)):
        st, ost = states[k]
        a = np.where(rng.random((B, A)) < 0.6, M, rng.integers(0, M + 1, (B, A))).astype(np.int32)
        if t == 5:
            obs.fill_(7)
            env.invalidate_obs(obs)
        _, out = env.step_raw(st, W._cuda(a), obs=obs, obs_delta=True)
        oobs, ost, r, d, info = ora.step(ost, a)
        states[k][1] = ost
        ctx = f"two states t={t} state {k}"
        np.testing.assert_array_equal(E._np(obs), oobs, err_msg=ctx)
        W._check_out(out, r, d, info, ctx)
        E._check_state(env, st, ost, ctx)


def shapes(forced):
    """The full write's and the scatter's index arithmetic on the device: V20 C91; D % 4 != 0 with the block 1-3
    elements off a 16-byte boundary and rem > 0 with literal-0 clauses (V23 C97, 8 agents, D = 143: the reference's
    quirk rows i >= rem); A = 1; and a shape past the prefetch at 64 and 256 lanes (V200 C1100, 67 agents:
    C > 1024 = 256 lanes x 4 pool words, A * WV = 536 > 512 = 256 x 2 nbr words), so the tail loops of the scan and
    the scatter run.  Mode-1 steps cross the quarter rule in both directions."""
    _, W, E = DW._imports()
    _two_states_one_tensor(forced)
    DW.delta_rollout(20, 91, 10, 8, True, _width(20, 91, 10, 8, forced), steps=6, obs_delta=True, seed=41)
    DW.delta_rollout(12, 40, 12, 8, True, _width(12, 40, 12, 8, forced), steps=6, obs_delta=True, offset=1, seed=42)
    plain_pool = E._pool

    def quirk_pool(V, C, N, k=3, seed0=0):
        p = plain_pool(V, C, N, k, seed0).copy()
        p[:, ::5, 2] = 0  # literal 0: such a clause is related to every agent i >= rem
        p[:, 3, :] = 0
        return p

    E._pool = quirk_pool
    try:
        assert 23 % 8 == 7  # rem > 0
        for offset in (1, 2, 3):
            DW.delta_rollout(23, 97, 3, 8, True, _width(23, 97, 3, 8, forced), steps=5, obs_delta=True, offset=offset,
                             seed=43 + offset)
        sp, wh = DW.delta_rollout(23, 97, 3, 8, False, _width(23, 97, 3, 8, forced), steps=5, obs_delta=True, offset=1,
                                  action_mode=1, max_steps=64, dense_at=(1, 3), seed=47)
        assert sp >= 1 and wh >= 1, (sp, wh)
    finally:
        E._pool = plain_pool
    DW.delta_rollout(200, 1100, 3, 4, True, _width(200, 1100, 3, 4, forced), steps=5, N=2, seed=48)


def modes(forced):
    """PBRS and sparse rewards, mode-0 edge actions, mode-1 flip words and the single-agent env (single-delta reward),
    each against the oracle and a full-write twin (tests/env_step_chain_worker.py)."""
    _, W, _ = DW._imports()
    W.decode_group()
    sp, wh = DW.delta_rollout(*UF200, 4, False, _width(*UF200, 4, forced), steps=4, action_mode=1, max_steps=64,
                              dense_at=(1,), seed=51)
    assert sp >= 1 and wh >= 1, (sp, wh)


GROUPS = {"small_batches": small_batches, "paths": paths, "shapes": shapes, "modes": modes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", required=True, choices=sorted(GROUPS))
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--debug", action="store_true")
    args = ap.parse_args()
    import torch

    from marlsat import _lib

    if args.debug:
        assert _lib.LIB_PATH.endswith("libmarlsat_debug.so"), _lib.LIB_PATH
    GROUPS[args.group](args.threads)
    torch.cuda.synchronize()
    print(f"wave step {args.group} threads {args.threads} ok", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
