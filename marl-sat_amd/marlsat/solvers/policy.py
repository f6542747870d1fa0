"""A trained policy as a SAT solver: tracked search, sampled restarts and a WalkSAT finish.

``policy_search`` is the inference loop: the reference's evaluation (src/runners/mappo_runner.py, runner:30-73 --
reset, then ``max_steps`` joint actions through ``step_env`` while remembering the first solve) with the memory
kept on the device by ``msat_solve_track`` (include/marlsat.h).  Beside ``runners.mappo_runner.evaluate_policy``,
which stays the reference's greedy evaluation, it

  * samples (Gumbel-max at a temperature, ``msat_sample_actions_t``) as well as taking the argmax;
  * writes no observation (``learner.policy`` reads ``(problem_idx, assignment)`` only) and runs no torch op
    in the step loop: per step one forward-and-sample, one env step, one track call;
  * keeps, for a row that never solves, the best assignment it saw and the step it saw it at, and for every
    row the number of variables it flipped.

``solve_pool_with_policy`` wraps it in restarts over a ``ProblemPool``, as ``solvers.walksat.solve_pool`` wraps
``walksat``: an optional greedy round, then rounds of ``tries`` sampled tries per unsolved instance, one winner
per instance chosen on the device (``msat_solve_pick``), and for what is left a WalkSAT run from the best
assignment the policy reached.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ..random import Key, as_key, split
from .walksat import noise_p32, walksat

_MASK = (1 << 64) - 1
BY_NONE, BY_POLICY, BY_WALKSAT = 0, 1, 2
FINISHES = ("walksat", "none")


@dataclass
class SearchRecord:
    """The device record of ``policy_search`` over B rows (``msat_solve_state``, include/marlsat.h)."""

    prev_x: torch.Tensor  # (B,V) uint8
    best_x: torch.Tensor  # (B,V) uint8: the solution where solved, else the best assignment seen
    best_unsat: torch.Tensor  # (B,) int32
    best_step: torch.Tensor  # (B,) int32
    first_solve: torch.Tensor  # (B,) int32, -1 = not solved, 0 = the reset assignment already satisfied
    flips: torch.Tensor  # (B,) int32
    unsolved: torch.Tensor  # (1,) int32
    steps_run: int = 0  # env steps the loop took (max_steps unless the early exit stopped it)

    @classmethod
    def alloc(cls, B: int, V: int, device) -> "SearchRecord":
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        return cls(e((B, V), torch.uint8), e((B, V), torch.uint8), e((B,), torch.int32), e((B,), torch.int32),
                   e((B,), torch.int32), e((B,), torch.int32), e((1,), torch.int32))

    def c(self) -> _lib.SolveStateC:
        return _lib.SolveStateC(self.prev_x.data_ptr(), self.best_x.data_ptr(), self.best_unsat.data_ptr(),
                                self.best_step.data_ptr(), self.first_solve.data_ptr(), self.flips.data_ptr(),
                                self.unsolved.data_ptr())

    def as_evaluation(self, max_steps: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``evaluate_policy``'s ``(solved, steps, solution)``: steps = the first solving step (``max_steps`` where
        unsolved), solution zeros where unsolved.  (A reset assignment that already satisfies its formula is
        ``first_solve == 0`` here; ``evaluate_policy`` only looks after a step.)"""
        first = self.first_solve.cpu().numpy()
        solved = first >= 0
        steps = np.where(solved, first, max_steps).astype(np.int32)
        sol = self.best_x.cpu().numpy() * solved[:, None].astype(np.uint8)
        return solved, steps, sol


def search_keys(key, max_steps: int) -> Tuple[Key, List[Key]]:
    """``evaluate_policy``'s key schedule: ``k_reset, k_run = split(key)``, then per step
    ``k_run, k_act = split(k_run)``.  Returns ``(k_reset, [k_act of step 1, 2, ...])``."""
    k = Key(*key) if isinstance(key, tuple) else as_key(key)
    k_reset, k_run = split(k, 2)
    acts = []
    for _ in range(int(max_steps)):
        k_run, k_act = split(k_run, 2)
        acts.append(k_act)
    return k_reset, acts


def check_temperature(temperature: float, who: str) -> float:
    t = float(temperature)
    if not (0.0 < t < math.inf):
        raise ValueError(f"{who}: temperature must be in (0, inf), got {temperature}")
    return t


@torch.no_grad()
def policy_search(learner, pool, problem_idx, max_steps: int, key, *, greedy: bool = False,
                  temperature: float = 1.0, early_exit: bool = True, trace: Optional[list] = None,
                  assignments=None, row_offset: Optional[int] = None, actor_only: bool = False) -> SearchRecord:
    """Row b searches instance ``problem_idx[b]`` of ``pool`` for ``max_steps`` steps of ``learner``'s policy
    (argmax when ``greedy``, else sampled at ``temperature``) from a random assignment, with ``evaluate_policy``'s
    key schedule (``search_keys``).  Returns the device ``SearchRecord``.

    Every 16 steps the host reads ``unsolved`` and stops at 0; a solved row is frozen, so this changes no
    output (``early_exit=False`` runs all steps).  ``trace``: a list that receives the reset assignment and
    every step's actions.  ``assignments`` ((B, V) 0/1): start there instead of the reset draw.  ``row_offset``
    (the slabs of ``solve_pool_with_policy``): row b samples the stream of row ``row_offset + b`` of an
    undivided batch (``learner.policy``).  ``actor_only``: every step encodes the agents' graphs alone, without
    the critic's graph that a search never reads (``learner.policy(actor_only=True)``); the record is the same."""
    env, dev = learner.env, learner.device
    max_steps = int(max_steps)
    if not 1 <= max_steps <= env.max_steps:
        raise ValueError(f"policy_search: max_steps={max_steps} outside [1, env.max_steps={env.max_steps}] (the "
                         f"env ends an episode there)")
    temperature = check_temperature(temperature, "policy_search")
    k_reset, k_acts = search_keys(key, max_steps)
    idx = torch.as_tensor(np.asarray(problem_idx), dtype=torch.int32, device=dev)
    B, V = idx.numel(), env.num_vars
    _, st = env.reset_from_pool(pool, B, k_reset, problem_idx=idx, assignments=assignments, with_obs=False)
    out = env._step_out(B)
    rec = SearchRecord.alloc(B, V, dev)
    rc, L, stream = rec.c(), _lib.lib, _lib.stream_ptr(dev)
    x_ptr, nun_ptr = st.variable_assignments.data_ptr(), st.num_unsatisfied.data_ptr()
    _lib.check(L.msat_solve_track_init(B, V, x_ptr, nun_ptr, ctypes.byref(rc), stream), "msat_solve_track_init")
    if trace is not None:
        trace.append(st.variable_assignments.clone())
    solved_ptr, step_nun_ptr = out["solved"].data_ptr(), out["num_unsatisfied"].data_ptr()
    for t in range(max_steps):
        act, _, _ = learner.policy(st, k_acts[t], greedy=greedy, critic=False, temperature=temperature,
                                   row_offset=row_offset, actor_only=actor_only)
        if trace is not None:
            trace.append(act.clone())
        env.step_raw(st, act, autoreset=False, out=out, with_obs=False)
        _lib.check(L.msat_solve_track(B, V, t + 1, x_ptr, solved_ptr, step_nun_ptr, ctypes.byref(rc), stream),
                   "msat_solve_track")
        rec.steps_run = t + 1
        if early_exit and (t + 1) % 16 == 0 and int(rec.unsolved.item()) == 0:
            break
    return rec


def check_solve_args(*, tries, rounds, max_steps, env_max_steps, temperature, finish, finish_tries, finish_flips,
                     noise, max_batch) -> None:
    """Argument checks of ``solve_pool_with_policy`` (host only)."""
    who = "solve_pool_with_policy"
    if int(tries) < 1 or int(rounds) < 0:
        raise ValueError(f"{who}: tries={tries}, rounds={rounds}")
    if max_steps is None or not 1 <= int(max_steps) <= int(env_max_steps):
        raise ValueError(f"{who}: max_steps={max_steps} outside [1, env.max_steps={env_max_steps}]")
    check_temperature(temperature, who)
    if finish not in FINISHES:
        raise ValueError(f"{who}: finish={finish!r}, expected one of {FINISHES}")
    if int(finish_tries) < 1 or int(finish_flips) < 0:
        raise ValueError(f"{who}: finish_tries={finish_tries}, finish_flips={finish_flips}")
    noise_p32(noise)
    if int(max_batch) < int(tries):
        raise ValueError(f"{who}: max_batch={max_batch} holds no instance's tries={tries} rows")


def round_plan(rounds: int, tries: int, greedy_round: bool) -> List[Tuple[bool, int]]:
    """(greedy, rows per instance) of every round: one greedy try first when ``greedy_round``, then ``tries``
    sampled tries."""
    return [(True, 1) if (greedy_round and r == 0) else (False, int(tries)) for r in range(int(rounds))]


def _round_outputs(n: int, V: int, device):
    """One buffer for a round's picks (so the round costs one device -> host read): five int32 arrays, the
    assignments, the solved flags."""
    buf = torch.empty(20 * n + n * V + n, dtype=torch.uint8, device=device)
    ints = buf[: 20 * n].view(torch.int32).view(5, n)
    return buf, ints, buf[20 * n: 20 * n + n * V].view(n, V), buf[20 * n + n * V:]


@torch.no_grad()
def solve_pool_with_policy(learner, pool, *, tries: int = 8, rounds: int = 2, max_steps: int = None,
                           temperature: float = 1.0, greedy_round: bool = True, finish: str = "walksat",
                           finish_tries: int = 8, finish_flips: int = 100_000, noise: float = 0.5,
                           max_batch: int = 4096, key=None, actor_only: bool = False) -> Dict[str, np.ndarray]:
    """One solution per instance of ``pool`` from ``learner``'s policy, WalkSAT finishing what it leaves.

    Round r (``round_plan``) runs, for every instance still unsolved, one greedy try (round 0 with
    ``greedy_round``) or ``tries`` tries sampled at ``temperature`` -- rows i * tries .. i * tries + tries - 1
    for the i-th of them, in instance order -- under ``Key(key.seed, key.counter + r)``, in slabs of at most
    ``max_batch`` rows.  Row s of a round starts where ``env.reset`` starts env s and samples the stream of row
    s, whatever the slab size, so ``max_batch`` changes no result.  ``msat_solve_pick`` reduces each slab to one
    record per instance; the host reads them once per round.  An instance's result is the winner of its first
    solving round.  An instance no round solves keeps its best record over all rounds (least ``best_unsat``,
    then least ``best_step``, then the earlier round, then the lower try), and with ``finish="walksat"``
    ``finish_tries`` WalkSAT samples of ``finish_flips`` flips start from that assignment under
    ``Key(key.seed, key.counter + rounds)``; the lowest solving sample wins.

    ``learner``: a ``MAPPOLearner`` over ``pool`` (its network, templates and chunk size are used at any batch).
    ``actor_only``: passed to every ``policy_search`` (actor-only graph batches; no result changes).
    Returns host arrays over the N instances: ``solved`` bool; ``by`` int8 (0 none, 1 policy, 2 walksat);
    ``solution`` (N, V) uint8 (zeros where unsolved); ``round``, ``try`` int32 of the winning or best try;
    ``steps`` int32 (the policy's first solving step, -1 where it did not solve); ``flips`` int32 (policy
    flips of that try); ``finish_flips`` int32 (WalkSAT flips of the winning sample, -1 otherwise);
    ``best_unsat`` int32 and ``best_solution`` (N, V) uint8 (the policy's best assignment; the solution where
    it solved)."""
    env = learner.env
    check_solve_args(tries=tries, rounds=rounds, max_steps=max_steps, env_max_steps=env.max_steps,
                     temperature=temperature, finish=finish, finish_tries=finish_tries, finish_flips=finish_flips,
                     noise=noise, max_batch=max_batch)
    if learner.pool is not pool:
        raise ValueError("solve_pool_with_policy: learner was built over another pool (its graph templates are "
                         "the pool's)")
    k = as_key(key)
    dev = learner.device
    N, V = int(pool.num_problems), int(pool.num_vars)
    i32 = lambda fill: np.full(N, fill, dtype=np.int32)
    out = {"solved": np.zeros(N, dtype=bool), "by": np.zeros(N, dtype=np.int8),
           "solution": np.zeros((N, V), dtype=np.uint8), "round": i32(-1), "try": i32(-1), "steps": i32(-1),
           "flips": i32(-1), "finish_flips": i32(-1), "best_unsat": i32(np.iinfo(np.int32).max),
           "best_solution": np.zeros((N, V), dtype=np.uint8)}
    best_step = i32(np.iinfo(np.int32).max)
    L = _lib.lib
    for r, (greedy, T) in enumerate(round_plan(rounds, tries, greedy_round)):
        todo = np.flatnonzero(~out["solved"])
        if todo.size == 0:
            break
        rk = Key(k.seed, (k.counter + r) & _MASK)
        pidx = np.repeat(todo, T).astype(np.int32)
        per = max(1, int(max_batch) // T)  # instances per slab
        x0 = None
        if todo.size > per:  # several slabs: the whole round's reset draw, cut up below
            _, st0 = env.reset_from_pool(pool, pidx.size, search_keys(rk, 0)[0], problem_idx=pidx, with_obs=False)
            x0 = st0.variable_assignments
        n = int(todo.size)
        buf, ints, xs, flags = _round_outputs(n, V, dev)
        for s0 in range(0, n, per):
            s1 = min(n, s0 + per)
            rec = policy_search(learner, pool, pidx[s0 * T: s1 * T], max_steps, rk, greedy=greedy,
                                temperature=temperature, assignments=None if x0 is None else x0[s0 * T: s1 * T],
                                row_offset=s0 * T, actor_only=actor_only)
            rc = rec.c()
            _lib.check(L.msat_solve_pick(s1 - s0, T, V, ctypes.byref(rc), flags[s0:s1].data_ptr(),
                                         ints[0, s0:s1].data_ptr(), ints[1, s0:s1].data_ptr(),
                                         ints[2, s0:s1].data_ptr(), ints[3, s0:s1].data_ptr(),
                                         ints[4, s0:s1].data_ptr(), xs[s0:s1].data_ptr(), _lib.stream_ptr(dev)),
                       "msat_solve_pick")
        host = buf.cpu().numpy()  # the round's one read
        h_int = host[: 20 * n].view(np.int32).reshape(5, n)
        h_x = host[20 * n: 20 * n + n * V].reshape(n, V)
        won = host[20 * n + n * V:] != 0
        h_try, h_steps, h_flips, h_bu, h_bs = h_int
        # a solving round ends the instance; otherwise the record replaces the kept one only if strictly better
        better = won | (h_bu < out["best_unsat"][todo]) | \
            ((h_bu == out["best_unsat"][todo]) & (h_bs < best_step[todo]))
        idx = todo[better]
        out["round"][idx] = r
        out["try"][idx] = h_try[better]
        out["flips"][idx] = h_flips[better]
        out["best_unsat"][idx] = h_bu[better]
        out["best_solution"][idx] = h_x[better]
        best_step[idx] = h_bs[better]
        idx = todo[won]
        out["solved"][idx] = True
        out["by"][idx] = BY_POLICY
        out["steps"][idx] = h_steps[won]
        out["solution"][idx] = h_x[won]
    out["best_unsat"][out["round"] < 0] = -1  # no round ran for the instance: no record
    left = np.flatnonzero(~out["solved"])
    if finish == "walksat" and left.size:
        if (out["round"][left] < 0).any():  # rounds == 0: no policy record, WalkSAT starts from its own draw
            init = None
        else:
            init = np.repeat(out["best_solution"][left], finish_tries, axis=0)
        x, ok, fl, _ = walksat(pool, np.repeat(left, finish_tries), key=Key(k.seed, (k.counter + int(rounds)) & _MASK),
                               max_flips=int(finish_flips), noise=noise, assignments=init)
        okm = ok.reshape(left.size, finish_tries) != 0
        first = torch.argmax(okm.to(torch.int32) * torch.arange(finish_tries, 0, -1, dtype=torch.int32, device=dev),
                             dim=1)
        rows = torch.arange(left.size, device=dev) * finish_tries + first
        packed = torch.cat([x[rows].to(torch.int32), fl[rows, None], okm.any(dim=1)[:, None].to(torch.int32)],
                           dim=1).cpu().numpy()
        won = packed[:, V + 1] != 0
        idx = left[won]
        out["solved"][idx] = True
        out["by"][idx] = BY_WALKSAT
        out["solution"][idx] = packed[won, :V].astype(np.uint8)
        out["finish_flips"][idx] = packed[won, V]
    return out
