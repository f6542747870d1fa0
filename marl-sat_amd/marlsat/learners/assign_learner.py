"""Supervised training of the assignment predictor on the device -- ``train_step`` / ``eval_step`` of
src/learners/bc_learner.py and the epoch loop of src/runners/bc_runner.py (:104-139).

The dataset is (instance id, input assignment x, expert solution) per sample; the GNN input is re-derived on the
device from (instance, x) as in every learner here (``assemble(critic_only=True)``: graph 0 alone).  One epoch is one
keyed device permutation of the N samples cut into minibatches ``perm[i:i+BATCH_SIZE]`` (the last one may be short
and is averaged over its own size, bc_runner.py:108-113); each minibatch is one gradient of the per-variable two-class
cross-entropy, ``jnp.mean`` over (sample, variable) (msat_assign_loss; micro-batched, exact: per-row terms add),
followed by one Adam step at the constant LEARNING_RATE (``optax.adam``, bc_learner.py:19: eps 1e-8, no schedule, no
clip).  The same launch that makes the loss also makes the arg-max assignment and checks it against the formula, so
Sol-Acc costs no second pass and no host loop: the prediction counted is the one from the parameters *before* the
minibatch's update, as ``train_step`` returns its logits.

Single process.  Deviations from the reference are listed in DESIGN.md §17.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from ..envs.multi_agent_sat_env import ProblemPool
from .assign_gnn import GNNAssignmentPredictor
from .base import GRAPH0, Learner, bounds, gather_rows

L_ = _lib.lib


class AssignLearner(Learner):
    """``trace``: a list receives, per Adam step, the minibatch rows, the parameters it started from, the gradient and
    the learning rate (and the step's predictions / solved flags)."""

    name = "assignment predictor"

    def __init__(self, config: dict, network: GNNAssignmentPredictor, pool: ProblemPool,
                 micro_bytes: Optional[float] = None, templates: str = "host"):
        self._init_shared(config, network, pool.device, templates, micro_bytes)
        self.V, self.C = int(pool.num_vars), int(pool.num_clauses)
        self.MB = int(config.get("BATCH_SIZE", 32))
        if self.MB < 1:
            raise ValueError(f"BATCH_SIZE={self.MB} must be >= 1")
        self.lr = float(config.get("LEARNING_RATE", 1e-4))
        # graph 0 of a template with one agent is all V variables and all C clauses
        self._plan_pool(pool, GRAPH0, self.V, 1, self.MB, self.MB)
        self.N = 0
        self.data: Optional[Dict[str, torch.Tensor]] = None
        self.minibatch_losses = None  # the last epoch's per-minibatch mean losses and accuracies (numpy)
        self.minibatch_accs = None

    def set_data(self, problem_idx, x, labels) -> None:
        """The dataset, kept on the device: problem_idx (N,) into the pool, x (N, V) u8 the input assignment that
        ``assemble`` derives the features from, labels (N, V) u8 the expert solution."""
        dev = self.device
        pidx = torch.as_tensor(problem_idx, device=dev).to(torch.int32).contiguous()
        xs = torch.as_tensor(x, device=dev).to(torch.uint8).contiguous()
        lab = torch.as_tensor(labels, device=dev).to(torch.uint8).contiguous()
        N = pidx.numel()
        if pidx.dim() != 1 or xs.shape != (N, self.V) or lab.shape != (N, self.V):
            raise ValueError(f"set_data: expected problem_idx (N,), x (N, {self.V}), labels (N, {self.V}); got "
                             f"{tuple(pidx.shape)}, {tuple(xs.shape)}, {tuple(lab.shape)}")
        if N and (int(pidx.min()) < 0 or int(pidx.max()) >= self.pool.num_problems):
            raise ValueError("set_data: problem_idx outside the pool")
        self.N = N
        self.data = {"pidx": pidx, "x": xs, "labels": lab}

    def gather_rows(self, idx: torch.Tensor):
        """The dataset rows ``idx`` (int32, device) in one launch (msat_gather_rows): (pidx, x, labels)."""
        return gather_rows(idx, [self.data["pidx"], self.data["x"], self.data["labels"]])

    def _loss(self, logits, S, labels, mb_size, pidx, dlogits, pred, unsat, solved, sums):
        """msat_assign_loss on one micro-batch or slab (labels / dlogits None: predict only)."""
        dev = self.device
        nll = torch.empty((S,), device=dev) if labels is not None else None
        correct = torch.empty((S,), dtype=torch.int32, device=dev) if labels is not None else None
        _lib.check(L_.msat_assign_loss(
            logits.data_ptr(), S, self.V, _lib.ptr(labels), mb_size, self.pool.packed.data_ptr(),
            self.pool.num_problems, self.C, pidx.data_ptr(), _lib.ptr(dlogits), pred.data_ptr(), _lib.ptr(nll),
            _lib.ptr(correct), unsat.data_ptr(), solved.data_ptr(), _lib.ptr(sums), _lib.stream_ptr(dev)),
            "msat_assign_loss")

    def plan(self, order: torch.Tensor, train: bool):
        """The micro-batches of a whole pass over the dataset rows ``order`` (minibatches of BATCH_SIZE, each cut into
        micro-batches) and their row totals, from ONE batch_totals(critic_only=True) read for the pass.
        -> [(start, stop, [(m0, m1, totals), ...]), ...] with positions into ``order``."""
        n, step = order.numel(), self.micro if train else self.chunk
        cuts = [bounds(i, min(i + self.MB, n), step) for i in range(0, n, self.MB)]
        every = sorted({b for c in cuts for b in c})
        sizes = dict(zip(every[:-1], self.totals(self.data["pidx"].index_select(0, order.long()), every)))
        return [(c[0], c[-1], [(m0, m1, sizes[m0]) for m0, m1 in zip(c[:-1], c[1:])]) for c in cuts]

    def minibatch_pass(self, idx: torch.Tensor, sums: torch.Tensor, mb_size: int, train: bool, micro=None):
        """The dataset rows ``idx`` through the network and the loss in micro-batches; ``sums`` (5,) fp64 accumulates
        (nll, correct, valid rows, invalid rows, solved samples).  ``train``: net.grads = d(mean loss)/d(params), the
        mean dividing by ``mb_size`` samples, so micro-batch gradients add up to the minibatch's.  ``micro``: the
        minibatch's entry of ``plan`` (positions relative to the pass); None plans this minibatch alone.
        -> (pred (n, V) u8, solved (n,) u8) in ``idx`` order."""
        net, dev, V = self.net, self.device, self.V
        idx = idx.to(torch.int32).contiguous()
        n = idx.numel()
        if train:
            net.grads.zero_()
        pred = torch.empty((n, V), dtype=torch.uint8, device=dev)
        unsat = torch.empty((n,), dtype=torch.int32, device=dev)
        solved = torch.empty((n,), dtype=torch.uint8, device=dev)
        if micro is None:
            micro = [m for _, _, ms in self.plan(idx, train) for m in ms]
        base = micro[0][0]
        for m0, m1, tot in ((a - base, b - base, t) for a, b, t in micro):
            S = m1 - m0
            pidx, x, lab = self.gather_rows(idx[m0:m1].contiguous())
            gb = self._batch(pidx, x, totals=tot)
            logits, _, state = net.forward(gb, critic=False, save=train)
            dlog = torch.empty_like(logits)
            self._loss(logits, S, lab, mb_size, pidx, dlog, pred[m0:m1], unsat[m0:m1], solved[m0:m1], sums)
            if train:
                net.backward(gb, state, dlog, None)
            del state
        return pred, solved

    def _metrics(self, sums: torch.Tensor, sizes: List[int], what: str) -> Dict[str, float]:
        """The epoch's one device -> host read and the reference's averages (bc_runner.py:136-142): loss and var_acc
        are the unweighted means of the minibatch means, sol_acc is solved samples / samples."""
        s = sums.cpu()
        bad = int(s[:, 3].sum())
        if bad:
            raise ValueError(f"{what}: {bad} (sample, variable) row(s) of this pass are invalid: a label outside "
                             f"{{0, 1}} or a non-finite logit; the reference's loss is NaN there")
        self.check_finite()
        rows = torch.tensor(sizes, dtype=torch.float64) * self.V
        self.minibatch_losses = (s[:, 0] / rows).numpy()  # each minibatch's mean, in step order
        self.minibatch_accs = (s[:, 1] / rows).numpy()
        return {"loss": float(self.minibatch_losses.mean()), "var_acc": float(self.minibatch_accs.mean()),
                "sol_acc": float(s[:, 4].sum()) / float(sum(sizes))}

    def train_epoch(self, generator: torch.Generator, rows=None) -> Dict[str, float]:
        """One pass over the dataset, or over its rows ``rows`` (the runner's training split), bc_runner.py:104-121:
        an Adam step per minibatch; -> loss, var_acc, sol_acc.  Two device -> host reads per epoch: the micro-batches'
        row totals before the first minibatch (``plan``) and the metrics after the last."""
        if not self.N:
            raise ValueError("AssignLearner.train_epoch: no data (set_data first)")
        if rows is not None:
            rows = torch.as_tensor(rows, device=self.device).to(torch.int32).contiguous()
        net, N, MB = self.net, self.N if rows is None else rows.numel(), self.MB
        if not N:
            raise ValueError("AssignLearner.train_epoch: no rows")
        starts = list(range(0, N, MB))
        sums = torch.zeros((len(starts), 5), dtype=torch.float64, device=self.device)
        perm = self.permutation(generator, N)
        if rows is not None:
            perm = rows.index_select(0, perm.long())
        for k, (i, j, micro) in enumerate(self.plan(perm, True)):  # the pass's one planning read
            idx = perm[i:j]
            pred, solved = self.minibatch_pass(idx, sums[k], idx.numel(), True, micro)
            if self.trace is not None:
                self.trace.append({"idx": idx.cpu(), "params": net.params.clone(), "grads": net.grads.clone(),
                                   "lr": self.lr, "pred": pred.cpu(), "solved": solved.cpu()})
            net.adam_step(self.lr, first_bad=self.first_bad)
        return self._metrics(sums, [min(MB, N - i) for i in starts], "train_epoch")

    def evaluate(self, idx) -> Dict[str, float]:
        """``eval_step`` over the dataset rows ``idx`` in batches of BATCH_SIZE, in order (bc_runner.py:123-134): no
        gradient, no update; the same three figures."""
        idx = torch.as_tensor(idx, device=self.device).to(torch.int32).contiguous()
        n, MB = idx.numel(), self.MB
        if not n:
            raise ValueError("AssignLearner.evaluate: no rows")
        starts = list(range(0, n, MB))
        sums = torch.zeros((len(starts), 5), dtype=torch.float64, device=self.device)
        for k, (i, j, micro) in enumerate(self.plan(idx, False)):
            part = idx[i:j]
            self.minibatch_pass(part, sums[k], part.numel(), False, micro)
        return self._metrics(sums, [min(MB, n - i) for i in starts], "evaluate")

    def predict(self, problem_idx, x, slab: Optional[int] = None):
        """The arg-max assignment for samples (problem_idx (n,), x (n, V)) through msat_assign_loss' predict-only
        mode, ``slab`` samples at a time (default: the inference chunk).  -> (pred (n, V) u8, num_unsat (n,) int32,
        solved (n,) u8) on the device; no host read but the slabs' row totals."""
        dev, V = self.device, self.V
        pidx = torch.as_tensor(problem_idx, device=dev).to(torch.int32).contiguous()
        xs = torch.as_tensor(x, device=dev).to(torch.uint8).contiguous()
        n = pidx.numel()
        if xs.shape != (n, V):
            raise ValueError(f"predict: expected x ({n}, {V}), got {tuple(xs.shape)}")
        pred = torch.empty((n, V), dtype=torch.uint8, device=dev)
        unsat = torch.empty((n,), dtype=torch.int32, device=dev)
        solved = torch.empty((n,), dtype=torch.uint8, device=dev)
        for m0, m1, tot in self.micro_batches(pidx, int(slab) if slab else self.chunk):
            gb = self._batch(pidx[m0:m1], xs[m0:m1], totals=tot)
            logits, _, _ = self.net.forward(gb, critic=False)
            self._loss(logits, m1 - m0, None, 1, pidx[m0:m1], None, pred[m0:m1], unsat[m0:m1], solved[m0:m1], None)
        return pred, unsat, solved
