"""The sparse path of the env step's delta observation write: bitwise against the full write and the NumPy oracle.

A delta step with 16-byte groups builds no bit images: it derives the dirty chunks from the source diff
(marl-sat_amd/csrc/obs_sparse.h) and evaluates each from the task's registers (chunks inside one source word) or
element by element (chunks that straddle a source word, a region, an agent row or an end of the block).  The shapes
here reach those edges; a reset, a row naming another instance and a step that flips more than a quarter of the
V + C source bits keep the full-image write, and the rollouts alternate between the two on one tensor.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle.sat_env import OracleSATEnv

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("variable_assignments", "clauses_satisfied_status", "clause_ntrue", "num_unsatisfied", "step",
                "env_done", "problem_idx")
OUT_FIELDS = ("reward", "done", "solved", "num_unsatisfied", "episode_step")
B, N, MAX_STEPS = 8, 4, 5

# name: V, C, vars_per_agent
SHAPES = {
    "v33c70": (33, 70, 3),     # source-word ends in mid-chunk, rem != 0
    "v64c64": (64, 64, 8),     # len == 32 exactly; V + C and D multiples of 32
    "v31c33": (31, 33, 31),    # one agent: no neighbour bits
    "uf200": (200, 860, 8),    # the 512-lane form
}


def _pool(V, C):
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses

    return np.stack([generate_sat_clauses(V, C, 3, seed=40 + i) for i in range(N)])


_POOLS = {}


def _setup(shape, dtype, action_mode, max_steps=MAX_STEPS):
    from marlsat import SATEnv

    V, C, vpa = SHAPES[shape]
    env = SATEnv(V, C, max_steps=max_steps, vars_per_agent=vpa, action_mode=action_mode,
                 obs_dtype=getattr(torch, dtype))
    ora = OracleSATEnv(V, C, max_steps=max_steps, vars_per_agent=vpa, action_mode=action_mode)
    if shape not in _POOLS:
        _POOLS[shape] = _pool(V, C)
    return env, ora, _POOLS[shape]


def _np(t):
    return t.detach().cpu().numpy()


def _obs_buffer(env, offset):
    """A (B, A, D) obs tensor whose first element lies `offset` elements past its allocation's start."""
    n = B * env.num_agents * env.obs_dim
    buf = torch.empty(n + offset, dtype=env.obs_dtype, device="cuda")
    return buf[offset:].view(B, env.num_agents, env.obs_dim)


def _actions(rng, env, t):
    A, M = env.num_agents, env.max_vars_per_agent
    if env.action_mode == 0:  # index M: no flip.  Most agents idle on odd steps, so the small shapes stay sparse too
        a = rng.integers(0, M + 1, size=(B, A))
        return np.where(rng.random((B, A)) < (0.2 if t % 2 == 0 else 0.85), M, a).astype(np.int32)
    # mode 1: every variable has its own flip bit.  Dense on even steps (about half of V flips: more than a quarter
    # of V + C source bits change, the full write), a few on odd steps (the sparse path)
    p = 0.5 if t % 2 == 0 else 0.04
    return (rng.random((B, A, M)) < p).astype(np.int32)


CASES = [(s, dt, am, off) for s in SHAPES for dt in ("int32", "int8") for am in (0, 1) for off in (0, 1, 2, 3)]


@pytest.mark.parametrize("shape,dtype,action_mode,offset", CASES)
def test_sparse_rollout_matches_full_write_and_oracle(shape, dtype, action_mode, offset):
    """2 x max_steps + 2 auto-reset steps with explicit reset inputs: the batch starts together, so it times out
    together (full writes of fresh instances), and sparse steps run in between on the same tensor."""
    env, ora, pool = _setup(shape, dtype, action_mode)
    V, C, _ = SHAPES[shape]
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(17 + offset)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs_d, obs_f = _obs_buffer(env, offset), _obs_buffer(env, offset)
    _, st_d = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_d)
    _, st_f = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x, obs=obs_f)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    few = many = resets = 0
    for t in range(2 * MAX_STEPS + 2):
        a = _actions(rng, env, t)
        npidx = rng.integers(0, N, B).astype(np.int32)
        nx = rng.integers(0, 2, (B, V)).astype(np.uint8)
        at = torch.from_numpy(a).cuda()
        _, out_d = env.step_raw(st_d, at, autoreset=True, problem_idx=npidx, assignments=nx, obs=obs_d,
                                obs_delta=True)
        _, out_f = env.step_raw(st_f, at, autoreset=True, problem_idx=npidx, assignments=nx, obs=obs_f,
                                obs_delta=False)
        prev = ost
        oobs, ost, r, d, info = ora.step_autoreset(ost, a, pool[npidx], nx.astype(np.int32))
        ctx = f"{shape} {dtype} mode {action_mode} offset {offset} t={t}"
        assert torch.equal(obs_d, obs_f), ctx
        np.testing.assert_array_equal(_np(obs_d).astype(np.int32), oobs, err_msg=ctx)
        for f in STATE_FIELDS:
            assert torch.equal(getattr(st_d, f), getattr(st_f, f)), f"{ctx}: state.{f}"
        for f in OUT_FIELDS:
            assert torch.equal(out_d[f], out_f[f]), f"{ctx}: out.{f}"
        np.testing.assert_array_equal(_np(st_d.variable_assignments), ost.variable_assignments, err_msg=ctx)
        np.testing.assert_array_equal(_np(out_d["reward"]), r, err_msg=ctx)
        np.testing.assert_array_equal(_np(out_d["done"]).astype(bool), d, err_msg=ctx)
        # which write each env took (t = 0 is the tensor's first step: whole blocks)
        flips = ((prev.variable_assignments != ost.variable_assignments).sum(1) +
                 (prev.clauses_satisfied_status != ost.clauses_satisfied_status).sum(1))
        if t > 0:
            live = ~d
            few += int((live & (4 * flips <= V + C)).sum())
            many += int((live & (4 * flips > V + C)).sum())
        resets += int(d.sum())
    assert few >= 1 and resets >= B  # the sparse path ran, and every env was reset in between
    if action_mode == 1:
        assert many >= 1  # the quarter rule was crossed in both directions


@pytest.mark.parametrize("shape,dtype,offset", [("v33c70", "int32", 0), ("v33c70", "int32", 3),
                                                 ("v33c70", "int8", 5), ("uf200", "int32", 1)])
def test_noop_steps_store_nothing(shape, dtype, offset):
    SENTINEL = 7
    env, ora, pool = _setup(shape, dtype, 0, max_steps=512)
    V, C, _ = SHAPES[shape]
    dpool = env.make_pool(pool)
    rng = np.random.default_rng(23)
    pidx = rng.integers(0, N, B).astype(np.int32)
    x = rng.integers(0, 2, (B, V)).astype(np.uint8)
    obs = _obs_buffer(env, offset)
    _, st = env.reset_from_pool(dpool, B, problem_idx=pidx, assignments=x)
    _, ost = ora.reset(pool[pidx], x.astype(np.int32))
    noop = np.full((B, env.num_agents), env.max_vars_per_agent, dtype=np.int32)  # index M: no flip
    at = torch.from_numpy(noop).cuda()
    # the first step into `obs` writes it whole (nothing is known about it) and records what it wrote
    _, out = env.step_raw(st, at, obs=obs, obs_delta=True)
    oobs, ost, _, d, _ = ora.step(ost, noop)
    assert not d.any()  # no env is done: none is skipped below
    np.testing.assert_array_equal(_np(obs).astype(np.int32), oobs)
    obs.fill_(SENTINEL)  # nothing changes from here on: every element is a kept one
    for _ in range(2):
        _, out = env.step_raw(st, at, obs=obs, obs_delta=True)
        assert not _np(out["done"]).any()
        assert (_np(obs) == SENTINEL).all()
    np.testing.assert_array_equal(_np(st.variable_assignments), x)
    env.invalidate_obs(obs)
    env.step_raw(st, at, obs=obs, obs_delta=True)
    np.testing.assert_array_equal(_np(obs).astype(np.int32), oobs)


DEBUG_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {root!r} + '/marl-sat_amd']
from marlsat import _lib
assert _lib.LIB_PATH.endswith('libmarlsat_debug.so'), _lib.LIB_PATH
from marlsat import SATEnv
from marlsat.random import Key
from marlsat.utils.generate_cnf_dataset import generate_sat_clauses
B = 8
for dtype, offset in ((torch.int32, 1), (torch.int8, 5)):
    env = SATEnv(33, 70, max_steps=4, vars_per_agent=3, obs_dtype=dtype)
    pool = env.make_pool(np.stack([generate_sat_clauses(33, 70, 3, seed=i) for i in range(4)]))
    n = B * env.num_agents * env.obs_dim
    obs = torch.empty(n + offset, dtype=dtype, device='cuda')[offset:].view(B, env.num_agents, env.obs_dim)
    _, st = env.reset_from_pool(pool, B, Key(1, 0), with_obs=False)
    rng = np.random.default_rng(0)
    for t in range(10):
        a = torch.from_numpy(rng.integers(0, 4, (B, env.num_agents)).astype(np.int32)).cuda()
        env.step_raw(st, a, autoreset=True, key=Key(2, t), obs=obs, obs_delta=True)  # kept chunks are read back
        assert torch.equal(obs, env.get_obs(st).tensor), (dtype, t)
print("debug sparse rollout ok", _lib.LIB_PATH)
"""


def test_debug_library_reads_back_the_chunks_a_sparse_step_keeps():
    """In a fresh child process, so that the library it loads is the debug one: every chunk the sparse path leaves
    alone is read back and compared with the element evaluator."""
    lib = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "libmarlsat_debug.so")
    assert os.path.exists(lib), "libmarlsat_debug.so not built (__graft_entry__.build() does)"
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT.format(root=ROOT)], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, MARLSAT_LIB=lib))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "debug sparse rollout ok" in r.stdout and "libmarlsat_debug.so" in r.stdout
