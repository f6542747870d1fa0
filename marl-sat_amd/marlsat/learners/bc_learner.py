"""Behavioural-cloning pre-training of the actor on the device -- drop-in for ``train_step`` and the
epoch loop of src/runners/behavioral_cloning.py (:239-282).

The dataset is (instance id, corrupted assignment, joint greedy labels) per sample
(runners/behavioral_cloning.preprocess); the GNN input is re-derived on the device from
(instance, assignment), as in the MAPPO learner.  One epoch is one keyed device permutation of the N
samples cut into minibatches ``perm[i:i+MINIBATCH_SIZE]`` (the last one may be short and is averaged over
its own size, :272-276); each minibatch is one gradient of the joint cross-entropy
``-mean(log_softmax(logits)[label])`` over (sample, agent) (msat_bc_loss; micro-batched like MAPPO, exact:
per-sample terms add) followed by one Adam step at the constant LEARNING_RATE (``optax.adam(LEARNING_RATE)``,
:225 -- no schedule, ANNEAL_LR is ignored).  Only the encoder, the actor and the agent embedding receive
gradient: the critic head is not evaluated, so its gradient is exactly 0 and Adam leaves it bitwise unchanged.
``actor_only=True`` also leaves the critic's graph out of every micro-batch (assemble(actor_only=True)): the
full batch encodes it, saves its tape and back-propagates an exactly-zero gradient through it.

Action mode 0 only (the reference's labels are mode-0 indices) and a single process (BC is a small offline
job; MAPPO's tests cover the gradient all-reduce).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _lib
from ..envs.multi_agent_sat_env import ProblemPool, SATEnv
from .base import ACTOR, FULL, Learner, gather_rows
from .gnn import GNNActorCritic

L_ = _lib.lib


class BCLearner(Learner):
    """``trace``: a list receives, per Adam step, the minibatch rows, the parameters it started from, the gradient
    and the learning rate."""

    name = "BC"

    def __init__(self, config: dict, env: SATEnv, network: GNNActorCritic, pool: ProblemPool,
                 micro_bytes: Optional[float] = None, actor_only: bool = False, templates: str = "host"):
        if env.action_mode != 0:
            raise ValueError(f"BCLearner: action_mode {env.action_mode} is not supported: the reference's BC labels "
                             f"(compute_joint_labels_parallel_greedy) are mode-0 indices (a local variable or the "
                             f"no-op)")
        self._init_shared(config, network, env.device, templates, micro_bytes)
        self.env = env
        self.MB = int(config["MINIBATCH_SIZE"])
        if self.MB < 1:
            raise ValueError(f"MINIBATCH_SIZE={self.MB} must be >= 1")
        self.lr = float(config.get("LEARNING_RATE", 3e-4))
        self.A, self.M = env.num_agents, env.max_vars_per_agent
        self.actor_only = bool(actor_only)
        self._plan_pool(pool, ACTOR if self.actor_only else FULL, env.num_vars, env.num_agents, self.MB, 1)
        self.N = 0
        self.data: Optional[Dict[str, torch.Tensor]] = None
        self.minibatch_losses = None  # the last epoch's per-minibatch mean losses (numpy, set by train_epoch)

    def set_data(self, problem_idx, assignments, labels) -> None:
        """The dataset, kept on the device: problem_idx (N,) into the pool, assignments (N, V) u8, labels (N, A)
        int32 in [0, M] (M = no-op)."""
        dev = self.device
        pidx = torch.as_tensor(problem_idx, device=dev).to(torch.int32).contiguous()
        x = torch.as_tensor(assignments, device=dev).to(torch.uint8).contiguous()
        lab = torch.as_tensor(labels, device=dev).to(torch.int32).contiguous()
        N = pidx.numel()
        if pidx.dim() != 1 or x.shape != (N, self.env.num_vars) or lab.shape != (N, self.A):
            raise ValueError(f"set_data: expected problem_idx (N,), assignments (N, {self.env.num_vars}), labels "
                             f"(N, {self.A}); got {tuple(pidx.shape)}, {tuple(x.shape)}, {tuple(lab.shape)}")
        if N and (int(pidx.min()) < 0 or int(pidx.max()) >= self.pool.clauses.shape[0]):
            raise ValueError("set_data: problem_idx outside the pool")
        self.N = N
        self.data = {"pidx": pidx, "x": x, "labels": lab}

    def gather_rows(self, idx: torch.Tensor):
        """The dataset rows ``idx`` (int32, device) in one launch (msat_gather_rows): (pidx, x, labels)."""
        return gather_rows(idx, [self.data["pidx"], self.data["x"], self.data["labels"]])

    def minibatch_grad(self, idx: torch.Tensor, sums: torch.Tensor, mb_size: int) -> None:
        """net.grads = d(loss)/d(params) of the joint cross-entropy over the dataset rows ``idx``; ``sums`` (4,)
        fp64 accumulates (nll, correct, valid rows, invalid rows).  The mean divides by ``mb_size`` samples, so
        micro-batch gradients add up to the minibatch's."""
        net, dev, A, M = self.net, self.device, self.A, self.M
        idx = idx.to(torch.int32).contiguous()
        net.grads.zero_()
        for m0, m1, tot in self.micro_batches(self.data["pidx"].index_select(0, idx.long()), self.micro):
            mi = idx[m0:m1].contiguous()
            S = mi.numel()
            pidx, x, lab = self.gather_rows(mi)
            gb = self._batch(pidx, x, totals=tot)
            logits, _, state = net.forward(gb, critic=False, save=True)
            dlog = torch.empty_like(logits)
            rows = torch.empty((2 * S * A,), device=dev)
            _lib.check(L_.msat_bc_loss(logits.data_ptr(), S, A, M, lab.data_ptr(), mb_size, dlog.data_ptr(),
                                       rows.data_ptr(), sums.data_ptr(), _lib.stream_ptr(dev)), "msat_bc_loss")
            net.backward(gb, state, dlog, None)
            del state

    def train_epoch(self, generator: torch.Generator) -> Dict[str, float]:
        """One pass over the dataset (behavioral_cloning.py:269-280): an Adam step per minibatch; returns the mean
        of the minibatch mean losses and the accuracy (rows whose argmax is the label / valid rows), both from one
        device -> host read."""
        if not self.N:
            raise ValueError("BCLearner.train_epoch: no data (set_data first)")
        net, N, MB, A = self.net, self.N, self.MB, self.A
        starts = list(range(0, N, MB))
        sums = torch.zeros((len(starts), 4), dtype=torch.float64, device=self.device)
        perm = self.permutation(generator)
        for k, i in enumerate(starts):
            idx = perm[i:i + MB]
            self.minibatch_grad(idx, sums[k], idx.numel())
            if self.trace is not None:
                self.trace.append({"idx": idx.cpu(), "params": net.params.clone(), "grads": net.grads.clone(),
                                   "lr": self.lr})
            net.adam_step(self.lr, first_bad=self.first_bad)
        s = sums.cpu()
        bad_labels = int(s[:, 3].sum())
        if bad_labels:
            raise ValueError(f"BC: {bad_labels} label(s) of this epoch point at a masked (padded, -inf logit) or "
                             f"out-of-range action slot; the reference's loss is inf / NaN there.  Labels must be in "
                             f"[0, M] = [0, {self.M}] and inside the agent's own variables or the no-op")
        self.check_finite()
        sizes = torch.tensor([min(MB, N - i) for i in starts], dtype=torch.float64)
        self.minibatch_losses = (s[:, 0] / (sizes * A)).numpy()  # each minibatch's mean, in Adam-step order
        loss = float(self.minibatch_losses.mean())
        return {"loss": loss, "accuracy": float(s[:, 1].sum() / max(float(s[:, 2].sum()), 1.0))}
