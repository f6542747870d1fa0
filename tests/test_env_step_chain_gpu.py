"""The env step's shortened chain: no broadcast barrier after the clause scan -- every wave derives done, the reset
decision and the shadow diff count itself, lane 0's transition outputs are waited for by nobody, and the in-workgroup
reset has a barrier of its own.  Every path a launch can take is walked here, next to the action decode in front of
the scan and the sparse delta write behind the decision.

Bitwise against the NumPy oracle; the delta cases also against a full-write twin stepped in lockstep.
  * action decode: every agent in turn takes each of -M-2, -M-1, -M, -1, 0, n-1, n, M, M+3 (sparse and PBRS
    rewards; the single-agent SatEnv, whose scatter drops what the gather clamps), mode 1 with no / all / random
    flip words, on V70 C33 vpa 9 (own ranges cross a 32-bit word, two ballot passes at 64 lanes) and V33 C70 vpa 3;
  * paths in one launch: B = 16 (8 reset workgroups), max_steps 3 -- ten envs time out in one launch (ranks 0-7 in
    reset workgroups, 8-9 in their own), one env is solved by its step, the others run; explicit reset inputs and
    Philox draws, ten delta steps with a plain step and a masked reset in between;
  * the full-or-sparse decision from the per-wave diff count: sparse steps at obs offsets 0-3, int32 and int8,
    across the quarter rule, with a row naming another instance, after invalidate_obs, and an all-no-op step that
    must store nothing;
  * the first two groups again at forced 64 and 512 lanes, the paths group on the debug library (bounds checks and
    the read-back of kept chunks), each in a child process (tests/env_step_chain_worker.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import env_step_chain_worker as W

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "env_step_chain_worker.py")


@pytest.mark.parametrize("shape", sorted(W.SMALL))
@pytest.mark.parametrize("reward_mode", [0, 1])
def test_action_decode_mode0(shape, reward_mode):
    W.decode_mode0(shape, reward_mode)


def test_action_decode_single_agent():
    W.decode_single_agent()


@pytest.mark.parametrize("shape", sorted(W.SMALL))
def test_action_decode_mode1(shape):
    W.decode_mode1(shape)


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit", "philox"])
def test_paths_in_one_launch(explicit):
    W.paths_in_one_launch(explicit)


SHAPES = dict(W.SMALL, uf200=(200, 860, 8))
MASK_CASES = [(s, dt, am, off) for s in sorted(W.SMALL) for dt in ("int32", "int8") for am in (0, 1)
              for off in (0, 1, 2, 3)] + [("uf200", "int32", 0, 1)]


@pytest.mark.parametrize("shape,dtype,action_mode,offset", MASK_CASES)
def test_sparse_steps_follow_the_per_wave_decision(shape, dtype, action_mode, offset):
    V, C, vpa = SHAPES[shape]
    B, N, SENTINEL = 8, 4, 7
    env, ora = W.E._mk(V, C, vpa, max_steps=512, action_mode=action_mode, obs_dtype=getattr(torch, dtype))
    A, M = env.num_agents, env.max_vars_per_agent
    pool = W.E._pool(V, C, N, seed0=600)
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(31 + offset)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs_d, obs_f = W._obs_buffer(env, B, offset), W._obs_buffer(env, B, offset)
    _, st_d = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_d)
    _, st_f = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_f)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))

    def actions(dense):
        if action_mode == 0:  # index M: no flip
            a = rng.integers(0, M + 1, (B, A))
            return np.where(rng.random((B, A)) < (0.0 if dense else 0.8), M, a).astype(np.int32)
        return (rng.random((B, A, M)) < (0.5 if dense else 0.04)).astype(np.int32)

    few = many = 0

    def step(a, ctx):
        nonlocal ost, few, many
        _, out_d = env.step_raw(st_d, W._cuda(a), obs=obs_d, obs_delta=True)
        _, out_f = env.step_raw(st_f, W._cuda(a), obs=obs_f, obs_delta=False)
        prev = ost
        oobs, ost, r, d, info = ora.step(ost, a)
        flips = ((prev.variable_assignments != ost.variable_assignments).sum(1) +
                 (prev.clauses_satisfied_status != ost.clauses_satisfied_status).sum(1))
        few += int((4 * flips <= V + C).sum())
        many += int((4 * flips > V + C).sum())
        np.testing.assert_array_equal(W._np(obs_d).astype(np.int32), oobs, err_msg=ctx)
        W._check_out(out_d, r, d, info, ctx)
        W.E._check_state(env, st_d, ost, ctx)
        W._check_twins(obs_d, obs_f, st_d, st_f, out_d, out_f, ctx)

    ctx = f"{shape} {dtype} mode {action_mode} offset {offset}"
    step(actions(False), ctx + " first (whole blocks)")
    step(actions(False), ctx + " sparse")
    few = many = 0
    step(actions(True), ctx + " dense")
    step(actions(False), ctx + " sparse after dense")
    assert few >= 1
    if action_mode == 1:
        assert many >= 1  # the quarter rule was crossed in both directions
    # rows naming another instance: half the envs move to other instances behind the obs tensor's back
    m = np.arange(B) % 2 == 0
    rp = ((pidx + 1) % N).astype(np.int32)
    rx = rng.integers(0, 2, (B, V)).astype(np.uint8)
    for st in (st_d, st_f):
        env.reset_from_pool(dpool, B, problem_idx=rp, assignments=rx, state=st, reset_mask=m.astype(np.uint8),
                            with_obs=False)
    _, st_r = ora.reset(pool[rp], rx.astype(np.int32))
    ost = W._merge(ora, m, ost, st_r)
    step(actions(False), ctx + " other instance")
    step(actions(False), ctx + " sparse again")
    # a caller who wrote into the buffer says so
    obs_d.fill_(SENTINEL)
    env.invalidate_obs(obs_d)
    step(actions(False), ctx + " after invalidate_obs")
    # nothing changes: nothing is stored
    noop = np.full((B, A), M, np.int32) if action_mode == 0 else np.zeros((B, A, M), np.int32)
    before = ost
    obs_d.fill_(SENTINEL)
    _, out = env.step_raw(st_d, W._cuda(noop), obs=obs_d, obs_delta=True)
    _, ost, _, _, _ = ora.step(ost, noop)
    np.testing.assert_array_equal(ost.variable_assignments, before.variable_assignments)
    assert (W._np(obs_d) == SENTINEL).all(), ctx + ": an all-no-op step stored something"
    env.invalidate_obs(obs_d)
    env.step_raw(st_d, W._cuda(noop), obs=obs_d, obs_delta=True)
    np.testing.assert_array_equal(W._np(obs_d).astype(np.int32), ora.get_obs(ost), err_msg=ctx + " restored")


def _child(args, env):
    r = subprocess.run([sys.executable, WORKER] + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("T", [64, 512])
def test_decode_and_paths_at_forced_width(T):
    assert f"step chain threads {T} ok" in _child(["--threads", str(T)], {"MARLSAT_ENV_THREADS": str(T)})


def test_paths_on_the_debug_library():
    lib = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    assert os.path.exists(lib), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    out = _child(["--debug"], {"MARLSAT_LIB": lib})
    assert "step chain debug ok" in out and "libmarlsat_debug.so" in out
