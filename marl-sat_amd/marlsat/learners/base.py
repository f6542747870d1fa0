"""What the learners share (MAPPOLearner, BCLearner, SinglePPOLearner, AssignLearner): the activation planner, the
graph templates of a pool and the batch kind they are planned for, the one ``assemble`` call, the micro-batch and chunk
cuts with their single device -> host read, the row gather, the keyed permutation, the Adam guard and the PPO
learners' rollout buffers.  A learner keeps what is its own: the loss launch and its arguments, schedules, rollout,
metrics and the validation of its config.
"""
from __future__ import annotations

import ctypes
from typing import Iterator, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from .graphs import assemble, assemble_critic, batch_totals, make_templates

L_ = _lib.lib
NO_BAD_STEP = 2 ** 31 - 1  # msat_adam_checked's "no non-finite update" value

# The graphs of a sample that a batch holds: all A + 1, the agents' A alone, or graph 0 alone (the critic's: every
# variable and clause; all there is for the single-agent network and the assignment predictor).
FULL, ACTOR, GRAPH0 = "full", "actor", "graph0"


def activation_bytes_per_sample(rows: float, H: int, L: int) -> float:
    """Saved activations of one training sample of ``rows`` graph rows (encode tape, fp32, per message step): var
    rows Hp, Hn, NV, two G4 tapes = 12H, clause rows Hc, GIN, G4 = 7H (bounded by 12H), plus ~24H of transients.
    L = 0: the transients alone, what inference holds."""
    return 4.0 * L * rows * 12 * H + 4.0 * rows * 24 * H


def activation_plan(config: dict, rows: float, H: int, L: int, minibatch: int, num_envs: int,
                    micro_bytes: Optional[float] = None):
    """(micro, chunk): the training micro-batch and the inference chunk (samples) that keep the saved activations
    inside the budget (``micro_bytes``, else MICROBATCH_BYTES); ``rows`` = a sample's mean graph rows
    (sample_rows)."""
    budget = micro_bytes if micro_bytes is not None else float(config.get("MICROBATCH_BYTES", 240e9))
    cap = max(1, min(minibatch, int(budget // activation_bytes_per_sample(rows, H, L))))
    micro = -(-minibatch // -(-minibatch // cap))  # equal micro-batches, none above the budget
    chunk = max(1, min(num_envs, int(budget // activation_bytes_per_sample(rows, H, 0))))
    return micro, chunk


def sample_rows(tpl, kind: str) -> float:
    """A sample's mean graph rows in a batch of ``kind``."""
    return {FULL: tpl.mean_full_rows, ACTOR: tpl.mean_actor_rows,
            GRAPH0: tpl.mean_full_rows - tpl.mean_actor_rows}[kind]


def bounds(start: int, stop: int, step: int) -> List[int]:
    """The cuts of [start, stop) into pieces of ``step`` (a short last one), both ends included."""
    return list(range(start, stop, step)) + [stop]


def spans(n: int, step: int) -> List[Tuple[int, int]]:
    """[(b0, b1), ...]: [0, n) in chunks of ``step``."""
    b = bounds(0, n, step)
    return list(zip(b[:-1], b[1:]))


def gather_rows(idx: torch.Tensor, srcs: Sequence[torch.Tensor], lead: int = 1) -> List[torch.Tensor]:
    """Rows ``idx`` (int32, device) of every tensor of ``srcs`` in one launch (msat_gather_rows).  The sources share
    their ``lead`` leading dimensions, which ``idx`` indexes flattened: 1 for a dataset (N, ...), 2 for rollout
    buffers (T, B, ...)."""
    S, n = idx.numel(), len(srcs)
    outs = [torch.empty((S,) + tuple(t.shape[lead:]), dtype=t.dtype, device=idx.device) for t in srcs]
    src = (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs])
    dst = (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs])
    rb = (ctypes.c_int32 * n)(*[t[(0,) * lead].numel() * t.element_size() for t in srcs])
    _lib.check(L_.msat_gather_rows(idx.data_ptr(), S, n, src, dst, rb, _lib.stream_ptr(idx.device)),
               "msat_gather_rows")
    return outs


class Learner:
    """State and helpers of every learner: device, net, pool, tpl, svf, kind, micro, chunk, first_bad, trace, and N,
    its row count (T*B transitions or the dataset's samples)."""

    name = "learner"  # in front of check_finite's message
    # after "a variable in no clause" in check_finite's message
    nonfinite_hint = " (tests/test_isolated_variable.py; utils.generate_cnf_dataset.has_isolated_variable)"

    def _init_shared(self, config: dict, network, device, templates: str, micro_bytes: Optional[float]) -> None:
        self.cfg = dict(config)
        self.net, self.device = network, device
        # "host": graphs.build_templates + upload; "device": graphs.build_templates_device (the same arrays)
        self.templates, self.micro_bytes = templates, micro_bytes
        # parity instrumentation: a list receives one record per Adam step (each learner says what it holds)
        self.trace: Optional[list] = None
        # fail-loud guard: the smallest Adam count whose update left a parameter non-finite (INT32_MAX: none)
        self.first_bad = torch.full((1,), NO_BAD_STEP, dtype=torch.int32, device=device)

    def _plan_pool(self, pool, kind: str, num_vars: int, num_agents: int, minibatch: int, num_envs: int) -> None:
        """The pool, its graph templates and static variable features, and the micro-batch / inference chunk planned
        for batches of ``kind`` (the learner's own from now on)."""
        self.tpl = make_templates(pool, num_vars, num_agents, self.templates, self.device)
        self.kind = kind
        self.micro, self.chunk = activation_plan(self.cfg, sample_rows(self.tpl, kind), self.net.H, self.net.L,
                                                 minibatch, num_envs, self.micro_bytes)
        self.svf = pool.static_var_features()
        self.pool = pool

    def _alloc_rollout(self, T: int, B: int, V: int, act_shape: Tuple[int, ...]) -> None:
        """The PPO learners' transition buffers ``tr``, advantages, targets, bootstrap values and moment workspace."""
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        self.N = T * B
        self.tr = {
            "pidx": z((T, B), torch.int32), "x": z((T, B, V), torch.uint8), "action": z(act_shape, torch.int32),
            "log_prob": z(act_shape, torch.float32), "value": z((T, B), torch.float32),
            "reward": z((T, B), torch.float32), "done": z((T, B), torch.uint8), "solved": z((T, B), torch.uint8),
            "num_unsatisfied": z((T, B), torch.int32), "episode_step": z((T, B), torch.int32),
        }
        self.adv = z((T, B), torch.float32)
        self.targets = z((T, B), torch.float32)
        self.last_val = z((B,), torch.float32)
        self.mom_ws = z((2 * 1024 + 2,), torch.float64)
        self.moments = z((2,), torch.float64)

    def _batch(self, pidx: torch.Tensor, x: torch.Tensor, kind: Optional[str] = None, totals=None):
        """The graph batch of samples (pidx, x) of ``kind`` (default: the learner's).  ``totals``: the batch's planned
        row totals (micro_batches), which spare the device -> host read."""
        kind = self.kind if kind is None else kind
        if kind == GRAPH0 and totals is not None:
            return assemble_critic(self.tpl, self.pool.packed, self.svf, pidx, x, totals)
        return assemble(self.tpl, self.pool.packed, self.svf, pidx.contiguous(), x.contiguous(), kind == GRAPH0,
                        totals, kind == ACTOR)

    def totals(self, inst: torch.Tensor, cuts: List[int]):
        """The row totals of the learner's batches inst[cuts[i]:cuts[i+1]]: ONE device -> host read for all."""
        return batch_totals(self.tpl, inst, cuts, self.kind == ACTOR, self.kind == GRAPH0)

    def micro_batches(self, inst: torch.Tensor, step: int) -> Iterator[Tuple[int, int, tuple]]:
        """(m0, m1, totals) of the rows' cuts into batches of ``step``; ``inst`` = their instance ids in order.  Every
        batch's row totals come from one device -> host read (assemble would otherwise read each batch's totals back,
        and the GPU idled while the host caught up)."""
        cuts = bounds(0, inst.numel(), step)
        return zip(cuts[:-1], cuts[1:], self.totals(inst, cuts))

    def permutation(self, generator: torch.Generator, n: Optional[int] = None) -> torch.Tensor:
        """A pseudo-random permutation of the learner's rows (T*B transitions or N samples; or of [0, n)), keyed from
        the host generator's stream and drawn on the device (msat_permutation)."""
        n = self.N if n is None else int(n)
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator))
        perm = torch.empty((n,), dtype=torch.int32, device=self.device)
        _lib.check(L_.msat_permutation(n, seed, 0, perm.data_ptr(), _lib.stream_ptr(self.device)), "msat_permutation")
        return perm

    def check_finite(self) -> None:
        """One read of the Adam guard (msat_adam_checked) per cycle or epoch: raise instead of carrying non-finite
        parameters on (the loop of mappo_runner.py:313-317 would train on NaN silently, as the reference does).  The
        guard is re-armed for a caller that recovers."""
        bad = int(self.first_bad.item())
        if bad != NO_BAD_STEP:
            self.first_bad.fill_(NO_BAD_STEP)
            raise FloatingPointError(f"{self.name}: Adam step {bad} left non-finite parameters.  A known cause: a pool "
                                     f"instance with a variable in no clause{self.nonfinite_hint}")
