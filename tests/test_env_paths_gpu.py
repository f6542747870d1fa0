"""GPU parity of the env step on the paths that tests/test_env_gpu.py's small batches never take: every workgroup
size env_threads() picks at natural batch sizes (64 lanes for small instances at B > 1024, 128 for uf100 at
B > 1024), instances larger than the per-lane prefetch (the clause-scan and table-staging loops behind the
prefetched registers), the pending scan of the reset queue at B > 4096, 63 and 65 agents, and the forced sizes of
MARLSAT_ENV_THREADS / MARLSAT_ENV_GROUP_THREADS (each in a child process: tests/env_threads_worker.py).

All of it is integer work against the NumPy oracle: bitwise, no tolerances.  Every case first asserts the workgroup
size the library reports for it (msat_env_launch_threads), so a retuned env_threads() fails the case instead of
silently moving it to another kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle.rng import reset_draws
from marlsat.random import Key
from test_env_gpu import _mk, _np, _pool

MAX_STEPS = 5  # an env whose counter starts at c times out at the launches t with (c + t) % 5 == 4


def rq_capacity(B):
    """Reset workgroups of a queue-consuming launch (env_kernels.hip rq_capacity)."""
    return (B // 256 + 8 + 7) & ~7


def rq_scan_words(B):
    """Pending words per lane of the queue scan (env_kernels.hip rq_scan: W)."""
    return ((B + 63) // 64 + 3) & ~3


def queue_fast_path(A, B):
    """The autoreset launch of the sparse reward mode with mode-0 actions consumes the reset queue (set_reset_queue)."""
    return A < 64 and B % 4 == 0


# name, V, C, vars_per_agent, A, B, T, RNG resets (else caller-given problem_idx / assignments), mass timeout,
# sample size, launches.  T is what env_threads() picks; what each case reaches is in its comment.
CASES = [
    ("uf50_x1032", 50, 218, 10, 5, 1032, 64, True, False, 64, 8),  # T = 64, queue fast path, XCD-major remap
    ("uf50_x1030", 50, 218, 10, 5, 1030, 64, False, False, 64, 8),  # B % 4: queue only cleared; B % 8: no remap
    ("uf100_x1032", 100, 430, 10, 10, 1032, 128, False, False, 64, 8),  # the bench's config-3 kernel
    ("uf100_a5_x1032", 100, 430, 20, 5, 1032, 64, False, False, 64, 8),  # C > 4 * 64: clause loop after the prefetch
    ("c600_x12", 60, 600, 30, 2, 12, 128, False, False, 64, 8),  # C = 600 > 4 * 128
    ("c600_x1032", 60, 600, 30, 2, 1032, 64, False, False, 64, 8),  # C = 600 > 4 * 64, two tail passes
    ("uf200_a10_x1032", 200, 860, 20, 10, 1032, 128, False, False, 40, 6),  # C > 512; A*WC = 280 (costly oracle)
    ("a65_x8", 130, 60, 2, 65, 8, 512, False, False, 64, 8),  # 65 agents: the queue's fast path is off
    ("a63_x8", 126, 60, 2, 63, 8, 512, False, False, 64, 8),  # 63 agents: the queue word in lane 63 of the action load
    ("a63_x16", 126, 60, 2, 63, 16, 512, False, False, 64, 8),  # the same with more pending envs than reset workgroups
    ("uf20_x4100", 20, 91, 10, 2, 4100, 64, True, False, 64, 8),  # queue scan: 68 words per lane (no bit mask)
    ("uf20_x8192", 20, 91, 10, 2, 8192, 64, True, True, 64, 8),  # 128 words per lane; the mass timeout
]
IDS = [c[0] for c in CASES]


def _plan(B, A, nsample, seed):
    """Staggered episode counters and the sampled envs of a case (host only; depends on nothing the device computes).

    Counters: three small groups at 4, 2, 1 (they time out at launches 0 and 5, 2 and 7, 3: fewer pending envs than
    reset workgroups; launch 0 finds the queue empty, so its timeouts reset in place), every other env at 3 (launches
    1 and 6: more pending envs than reset workgroups whenever B allows).
    At B > 4096 the small groups hold the envs on both sides of queue-scan lane boundaries (k W - 1 and k W): the env
    at k W - 1 is the last word of a lane's range, past the 64 the lane could keep as a bit mask.
    Sample: envs 0..15, the last 16, the boundary envs, two of each small group, random others."""
    rng = np.random.default_rng(seed)
    cap, W = rq_capacity(B), rq_scan_words(B)
    edges = [i for k in (1, 2, 31, 60) for i in (k * W - 1, k * W)] if B > 4096 else []
    assert all(0 < i < B for i in edges)
    few = max(1, min(cap // 2, B // 8))
    taken = set(edges)
    order = edges + [int(i) for i in rng.permutation(B) if int(i) not in taken]
    groups = [order[g:3 * few:3] for g in range(3)]
    counters = np.full(B, MAX_STEPS - 2, np.int32)
    for g, idx in enumerate(groups):
        counters[idx] = (4, 2, 1)[g]
    must = list(range(min(16, B))) + list(range(max(0, B - 16), B)) + edges + [i for g in groups for i in g[:2]]
    sample = list(dict.fromkeys(must))
    assert len(sample) <= max(nsample, 1)
    rest = [i for i in order[3 * few:] if i not in set(sample)]
    sample = np.array(sorted(sample + rest[:max(0, min(nsample, B) - len(sample))]), np.int64)
    return counters, sample


class _Coverage:
    """Which reset paths the sampled envs took, from the counters alone: an env is pending iff its counter is
    max_steps - 1 before the launch; from the second launch after the queue was zeroed, a queue-consuming launch
    resets the pending envs of rank < cap (index order) in reset workgroups and the others in their step workgroup."""

    def __init__(self, A, B):
        self.queue, self.cap, self.B = queue_fast_path(A, B), rq_capacity(B), B
        self.side = self.over = self.inplace = self.none = 0
        self.more = self.fewer = 0  # queue-consuming launches with more / fewer pending envs than reset workgroups

    def classify(self, step0, launch):
        pend = step0 == MAX_STEPS - 1
        active = self.queue and launch >= 1
        side = pend & (np.cumsum(pend) - 1 < self.cap) if active else np.zeros_like(pend)
        return pend, side, active

    def add(self, step0, launch, sample, reset):
        pend, side, active = self.classify(step0, launch)
        self.side += int(side[sample].sum())
        self.inplace += int((pend & ~side)[sample].sum())
        self.over += int((pend & ~side)[sample].sum()) if active else 0
        self.none += int((~reset).sum())
        if active and pend.any():
            self.more += int(pend.sum() > self.cap)
            self.fewer += int(pend.sum() < self.cap)

    def check(self):
        assert self.inplace > 0 and self.none > 0, vars(self)  # a timeout reset in place, an env that does not reset
        if self.queue:
            assert self.side > 0 and self.fewer > 0, vars(self)  # a reset workgroup's env
            if self.B > self.cap:  # more envs than reset workgroups: a pending env of rank >= cap, reset in place
                assert self.over > 0 and self.more > 0, vars(self)


@pytest.mark.parametrize("name,V,C,vpa,A,B,T,rng_resets,mass,nsample,steps", CASES, ids=IDS)
def test_plans_reach_every_reset_path(name, V, C, vpa, A, B, T, rng_resets, mass, nsample, steps):
    """CPU: the counters and the sample of every case reach what the GPU test then asserts on the device's own
    counters -- replayed here on the counters alone (no env is solved: an env resets iff it times out)."""
    counters, sample = _plan(B, A, nsample, CASES.index((name, V, C, vpa, A, B, T, rng_resets, mass, nsample, steps)))
    assert len(sample) <= 64 and len(set(sample.tolist())) == len(sample)
    cov = _Coverage(A, B)
    step = counters.copy()
    for t in range(steps):
        pend = step == MAX_STEPS - 1
        cov.add(step, t, sample, pend[sample])
        step = np.where(pend, 0, step + 1)
    cov.check()
    # the one case where B <= cap leaves no env to overflow the reset workgroups has a larger twin that does
    assert B > rq_capacity(B) or not queue_fast_path(A, B) or name == "a63_x8"


@pytest.mark.gpu
@pytest.mark.parametrize("name,V,C,vpa,A,B,T,rng_resets,mass,nsample,steps", CASES, ids=IDS)
def test_large_batch_rollout_sampled_parity(name, V, C, vpa, A, B, T, rng_resets, mass, nsample, steps):
    """Autoreset steps at full B (sparse reward, mode-0 actions, int32 obs): invariants on every env, and a sample of
    envs replayed on the oracle each step from the device's pre-step problem_idx / assignment / step -- obs, the step
    outputs and the post-step state bitwise.  The sample must contain a timed-out env reset by a reset workgroup, one
    reset in place behind the reset workgroups' capacity, and one that does not reset (_Coverage.check; where the
    queue cannot act -- B % 4 != 0, 65 agents -- a timeout reset in place and an env that does not reset; a63_x8 has
    no more envs than reset workgroups, its twin a63_x16 has)."""
    from marlsat import _lib
    from oracle.sat_env import OracleSATEnv

    case = CASES.index((name, V, C, vpa, A, B, T, rng_resets, mass, nsample, steps))
    N = 8
    env, ora = _mk(V, C, vpa, max_steps=MAX_STEPS)
    assert env.num_agents == A
    pool = _pool(V, C, N, seed0=4000 + 10 * case)
    dpool = env.make_pool(pool)
    got = _lib.lib.msat_env_launch_threads(env._desc(B, dpool))
    print(f"{name}: msat_env_launch_threads = {got}")
    assert got == T
    counters, sample = _plan(B, A, nsample, case)
    sdev = torch.from_numpy(sample).cuda()
    rng = np.random.default_rng(500 + case)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x)
    assert st.reset_queue is not None
    st.step.copy_(torch.from_numpy(counters).cuda())
    st.invalidate_reset_queue()
    cov = _Coverage(A, B)
    launch = 0  # launches since the queue was zeroed
    M = env.max_vars_per_agent
    for t in range(steps + (2 if mass else 0)):
        if t == steps:  # every counter one step short of the last: this launch lists every env, the next resets them
            st.step.fill_(MAX_STEPS - 2)
            st.invalidate_reset_queue()
            launch = 0
        ctx = f"{name} t={t}"
        pidx0, x0, step0 = _np(st.problem_idx).copy(), _np(st.variable_assignments).copy(), _np(st.step).copy()
        pend, side, active = cov.classify(step0, launch)
        # the device's queue lists exactly the pending envs the host predicts (none on the first launch after zeroing)
        q = _np(st.reset_queue).view(np.uint32)
        par, tok = st.reset_serial & 1, 0x80000000 | (st.reset_serial & 0x7FFFFFFF)
        np.testing.assert_array_equal(q[par * B:(par + 1) * B] == tok, pend & active, err_msg=ctx + " queue")
        a = rng.integers(0, M + 1, (B, A)).astype(np.int32)
        if rng_resets:
            key = Key(77 + case, t + 1)
            obs, out = env.step_raw(st, torch.from_numpy(a).cuda(), autoreset=True, key=key)
            p2, x2 = reset_draws(key.seed, key.counter, B, V, N)
        else:
            p2 = rng.integers(0, N, B).astype(np.int32)
            x2 = rng.integers(0, 2, (B, V)).astype(np.uint8)
            obs, out = env.step_raw(st, torch.from_numpy(a).cuda(), autoreset=True, problem_idx=p2, assignments=x2)
        launch += 1
        # ---- every env: the clause state is consistent, and what a reset writes follows from the step's done
        sat = st.clauses_satisfied_status.int()
        assert torch.equal(C - sat.sum(1), st.num_unsatisfied), ctx
        assert torch.equal(st.clause_ntrue.gt(0).int(), sat), ctx
        done = _np(out["done"]).astype(bool)
        assert done[pend].all(), ctx
        np.testing.assert_array_equal(_np(out["episode_step"]), step0 + 1, err_msg=ctx)
        np.testing.assert_array_equal(_np(st.step), np.where(done, 0, step0 + 1), err_msg=ctx)
        np.testing.assert_array_equal(_np(st.problem_idx), np.where(done, p2, pidx0), err_msg=ctx)
        np.testing.assert_array_equal(_np(st.variable_assignments)[done], x2[done], err_msg=ctx)
        # ---- the sample: replayed on the oracle
        s = sample
        _, ost = ora.reset(pool[pidx0[s]], x0[s].astype(np.int32))
        ost.step = step0[s].copy()
        oobs, ost, r, d, info = ora.step_autoreset(ost, a[s], pool[p2[s]], x2[s].astype(np.int32))
        np.testing.assert_array_equal(_np(obs[sdev]), oobs, err_msg=ctx)
        np.testing.assert_array_equal(_np(out["reward"])[s], r, err_msg=ctx)
        np.testing.assert_array_equal(done[s], d, err_msg=ctx)
        np.testing.assert_array_equal(_np(out["solved"])[s].astype(bool), info["solved"], err_msg=ctx)
        np.testing.assert_array_equal(_np(out["num_unsatisfied"])[s], info["num_unsatisfied"], err_msg=ctx)
        np.testing.assert_array_equal(_np(out["episode_step"])[s], info["episode_step"], err_msg=ctx)
        np.testing.assert_array_equal(_np(st.variable_assignments)[s], ost.variable_assignments, err_msg=ctx)
        np.testing.assert_array_equal(_np(st.clauses_satisfied_status)[s].astype(bool), ost.clauses_satisfied_status,
                                      err_msg=ctx)
        np.testing.assert_array_equal(_np(st.clause_ntrue)[s],
                                      OracleSATEnv.num_true_literals(ost.variable_assignments, ost.clauses),
                                      err_msg=ctx)
        np.testing.assert_array_equal(_np(st.num_unsatisfied)[s], ost.num_unsatisfied, err_msg=ctx)
        np.testing.assert_array_equal(_np(st.step)[s], ost.step, err_msg=ctx)
        np.testing.assert_array_equal(_np(st.env_done)[s].astype(bool), ost.done[:, 0], err_msg=ctx)
        np.testing.assert_array_equal(_np(st.problem_idx)[s], np.where(d, p2[s], pidx0[s]), err_msg=ctx)
        np.testing.assert_array_equal(pool[_np(st.problem_idx)[s]], ost.clauses, err_msg=ctx)
        cov.add(step0, launch - 1, sample, d)
        if t == steps + 1:  # the mass timeout: every env the launch before did not solve (and reset) was pending
            np.testing.assert_array_equal(pend, ~prev_done, err_msg=ctx)
            assert pend.mean() > 0.9 and active and int(side.sum()) == cov.cap, ctx
        prev_done = done
    cov.check()


WORKER = os.path.join(ROOT, "tests", "env_threads_worker.py")


def _run_worker(flag, T, var):
    """One child process with the override in its environment (the library reads it once per process)."""
    env = dict(os.environ, **{var: str(T)})
    r = subprocess.run([sys.executable, WORKER, flag, str(T)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("T", [64, 128, 256, 512])
def test_forced_env_threads_match_oracle(T):
    """MARLSAT_ENV_THREADS=T: reset and 10-step rollouts (autoreset off and on) of uf20 .. uf200 with 25 agents,
    uneven and single-agent partitions and 65 agents, and the four reward / action mode pairs on uf50, bitwise
    against the oracle, after the library reported T for every one of them (env_threads_worker.py).  T = 64 on
    uf200 walks every loop behind the prefetch (A*WC = 700, A*WV = 200, C = 860), and with 65 agents the action
    loop's second pass; T = 256 / 512 run the small instances on sizes env_threads() never gives them."""
    assert f"env threads {T} ok" in _run_worker("--threads", T, "MARLSAT_ENV_THREADS")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [256, 1024])
def test_forced_env_group_threads_match_oracle(T):
    """MARLSAT_ENV_GROUP_THREADS=T: the grouped launch of config 5 against the oracle per class, and the eight-class
    launch with empty classes, after msat_env_group_launch_threads reported T (natural: 512 at these sizes)."""
    assert f"env group threads {T} ok" in _run_worker("--group-threads", T, "MARLSAT_ENV_GROUP_THREADS")
