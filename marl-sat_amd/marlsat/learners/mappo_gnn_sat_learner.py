"""MAPPO train cycle on the device — drop-in for ``make_train_cycle`` /
``SATDataWrapper`` / ``GNN_ActorCritic`` of src/learners/mappo_gnn_sat_learner.py.

One ``train_cycle(runner_state, update_idx)`` is the reference's jitted
``_train_cycle`` (:382-729):
  1. rollout of NUM_STEPS batched steps (:383-494): actor + critic forward on the
     current global states, Categorical sampling, fused env step with the
     rollout's auto-reset (done envs redraw a pool instance + assignment);
  2. bootstrap value, GAE and global advantage normalisation (:497-532);
  3. UPDATE_EPOCHS x (T*B / MINIBATCH_SIZE) PPO minibatch steps (:563-659), each a
     gradient over the whole minibatch (micro-batched to bound activation memory,
     exact: gradients of per-sample terms add) followed by one Adam step;
  4. the reference's metrics dict (:661-719).
Transitions store (instance id, assignment) instead of the dense GNN input
(the reference's dense A_pos/A_neg per transition is ~2.9 TB at
uf200 x 4096 x 512); the global state is re-derived on the device when needed.
Multi-GPU: one process per GPU with its own env shard; the flat gradient is
all-reduced (RCCL via torch.distributed) before every Adam step and the
advantage moments / metric sums once per cycle.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from ..envs.multi_agent_sat_env import ObsDict, ProblemPool, SATEnv, SATState
from ..random import Key, as_key, split
from .base import ACTOR, FULL, GRAPH0, Learner, activation_plan, gather_rows, sample_rows, spans
from .collectives import allreduce_grads, allreduce_sums, global_moments, world_size
from .gnn import GNNActorCritic
from .ops import gae as device_gae

L_ = _lib.lib


# ------------------------------------------------------------ schedules ----
def learning_rate_at(count: int, config: dict) -> float:
    """mappo_runner.py:171-193: optax.linear_schedule over Adam step counts (else constant)."""
    if not config.get("ANNEAL_LR", False):
        return float(config.get("LEARNING_RATE", 3e-4))
    n = config.get("NUM_UPDATES", 1)
    lr0 = config.get("LEARNING_RATE", 3e-4) * config.get("LR_START_FACTOR", 1.0)
    lr1 = config.get("LR_END_FLOOR", 1e-5)
    frac = 1.0 - min(max(count, 0), n) / n
    return (lr0 - lr1) * frac + lr1


def ent_coef_at(update_idx: int, config: dict) -> float:
    """learner:534-558."""
    if not config.get("ANNEAL_ENT", False):
        return float(config["ENT_COEF"])
    n = config["NUM_UPDATES"]
    c0, c1 = config["ENT_COEF"], config.get("ENT_COEF_END", 0.0)
    start = n * (1.0 - config.get("ANNEAL_ENT_FRAC", 0.333))
    if update_idx < start:
        return float(c0)
    frac = min(1.0, max(0.0, (update_idx - start) / (n - start)))
    return float(c0 - (c0 - c1) * frac)


# ------------------------------------------------------------- wrapper ----
@dataclass
class GNNInput:
    """graph_constructor.GNNInput (batched).  The dense adjacency is materialised on demand."""

    static_var_features: torch.Tensor  # (B,V,3)
    assignment: torch.Tensor  # (B,V)
    clause_features: torch.Tensor  # (B,C,3)
    _state: SATState = field(repr=False)

    def _dense(self, sign: int) -> torch.Tensor:
        st = self._state
        cl = st.clauses.long()  # (B,C,K)
        B, C, K = cl.shape
        V = st.env.num_vars
        A = torch.zeros((B, V, C), dtype=torch.float32, device=cl.device)
        keep = (cl > 0) if sign > 0 else (cl < 0)
        b = torch.arange(B, device=cl.device)[:, None, None].expand_as(cl)[keep]
        c = torch.arange(C, device=cl.device)[None, :, None].expand_as(cl)[keep]
        v = (cl.abs() - 1)[keep]
        A.index_put_((b, v, c), torch.ones_like(v, dtype=torch.float32), accumulate=True)
        return A

    @property
    def A_pos(self) -> torch.Tensor:
        return self._dense(+1)

    @property
    def A_neg(self) -> torch.Tensor:
        return self._dense(-1)


@dataclass
class GNNWrapperState:
    env_state: SATState


class SATDataWrapper:
    """learner:93-195 — adds the GNN global state to every reset / step (batched)."""

    def __init__(self, env: SATEnv):
        self._env = env

    def __getattr__(self, name):  # JaxMARLWrapper attribute delegation
        return getattr(self._env, name)

    def _global_state(self, st: SATState) -> GNNInput:
        svf = st.pool.static_var_features()[st.problem_idx.long()]
        return GNNInput(svf, st.variable_assignments, self._env.clause_features(st), st)

    def reset(self, problem_clauses, key=None, *, assignments=None):
        obs, st = self._env.reset(problem_clauses, key, assignments=assignments)
        return (obs, self._global_state(st)), GNNWrapperState(st)

    def step(self, key, state: GNNWrapperState, actions):
        obs, st, reward, done, info = self._env.step_env(key, state.env_state, actions)
        return (obs, self._global_state(st)), GNNWrapperState(st), reward, done, info


# -------------------------------------------------------------- learner ----
@dataclass
class RunnerState:
    env_state: SATState
    obs: torch.Tensor  # (B,A,D) last local obs
    rng: Key
    rollout_counter: int = 0


class MAPPOLearner(Learner):
    """Device implementation of make_train_cycle's _train_cycle (see module docstring).  ``trace``: a list makes
    ppo_update record, per Adam step, the minibatch rows, the parameters it started from, the (all-reduced) gradient
    and the learning rate."""

    name = "MAPPO"
    nonfinite_hint = (" -- assigned 0, that variable is a constant LayerNorm row at zero-initialised biases and its "
                      "gradient grows ~1000x per message-passing layer past fp32 range, in the reference as here "
                      "(tests/test_isolated_variable.py; filter the pool with generate_problem_pool(skip_isolated=True) "
                      "or utils.generate_cnf_dataset.has_isolated_variable)")

    def __init__(self, config: dict, env: SATEnv, network: GNNActorCritic, pool: ProblemPool,
                 dist=None, micro_bytes: Optional[float] = None, templates: str = "host"):
        """templates: "host" builds the graph templates with graphs.build_templates and uploads them; "device"
        builds them with graphs.build_templates_device (the same arrays; the host builder for a shape past the
        kernels' LDS bound)."""
        self._init_shared(config, network, env.device, templates, micro_bytes)
        self.env = env
        self.dist = dist
        self.world = world_size(dist)
        self.B = int(config["NUM_ENVS"])
        self.T = int(config["NUM_STEPS"])
        self.MB = int(config["MINIBATCH_SIZE"])
        N = self.T * self.B
        if N % self.MB:
            raise ValueError(f"NUM_STEPS*NUM_ENVS={N} must be divisible by MINIBATCH_SIZE={self.MB} (learner:582-592)")
        self.n_minibatches = N // self.MB
        self.pool = None
        self.set_pool(pool)
        self.A, self.M = env.num_agents, env.max_vars_per_agent
        self.mode = env.action_mode
        self._alloc_rollout(self.T, self.B, env.num_vars,
                            (self.T, self.B, self.A) if self.mode == 0 else (self.T, self.B, self.A, self.M))

    def set_pool(self, pool: ProblemPool) -> None:
        """Train on another pool of the same (V, C, K) from now on: replaces the pool, its graph templates and its
        static variable features, and plans the micro-batch and the two inference chunks again from the new
        templates' row counts.  The network, the optimiser state and the rollout buffers stay.  A RunnerState made
        over the old pool is invalid (its env state names the old pool's instances): call init_runner_state again."""
        old = self.pool
        if old is not None and (pool.num_vars, pool.num_clauses, pool.clause_width) != (
                old.num_vars, old.num_clauses, old.clause_width):
            raise ValueError(f"set_pool: the new pool is (V, C, K) = ({pool.num_vars}, {pool.num_clauses}, "
                             f"{pool.clause_width}); the learner's is ({old.num_vars}, {old.num_clauses}, "
                             f"{old.clause_width})")
        if pool.num_vars != self.env.num_vars or pool.num_clauses != self.env.num_clauses:
            raise ValueError(f"pool is V={pool.num_vars}, C={pool.num_clauses}; env is V={self.env.num_vars}, "
                             f"C={self.env.num_clauses}")
        self._plan_pool(pool, FULL, self.env.num_vars, self.env.num_agents, self.MB, self.B)
        # the inference chunk of an actor-only batch (policy(actor_only=True)): the same budget over fewer rows
        _, self.actor_chunk = activation_plan(self.cfg, sample_rows(self.tpl, ACTOR), self.net.H, self.net.L, self.MB,
                                              self.B, self.micro_bytes)

    # ------------------------------------------------------------ helpers ----
    def init_runner_state(self, key) -> RunnerState:
        """mappo_runner.py:288-303: B envs reset onto uniformly drawn training problems."""
        k = as_key(key)
        k_reset, k_run = split(k, 2)
        obs, st = self.env.reset_from_pool(self.pool, self.B, k_reset)
        return RunnerState(st, obs, k_run, 0)

    def policy(self, st: SATState, key: Key, greedy: bool = False, critic: bool = True, temperature: float = 1.0,
               row_offset: Optional[int] = None, actor_only: bool = False):
        """Actor (+ critic) on the current states (learner:391-403): actions, log_probs, values.
        greedy: argmax actions (evaluate_policy, runner:38-46); critic=False skips the value head.
        temperature != 1.0 (sampling only): Gumbel-max on logits / temperature, log_probs under that
        distribution (msat_sample_actions_t).  row_offset (sampling only; the policy solver's slabs): env b
        draws the stream of env row_offset + b of one undivided batch, whatever the chunk size
        (msat_sample_actions_from).  With neither, the calls are exactly what they were.
        actor_only (needs critic=False): encode the agents' graphs alone (assemble(actor_only=True)); every
        row of the encoder is independent of its neighbours, so the logits, actions and log_probs are those of
        the full batch.  The chunk index enters the sampling counter unless row_offset names the streams, so
        the chunk stays self.chunk there; greedy or with row_offset the larger actor-only chunk is used."""
        if not (0.0 < float(temperature) < math.inf):
            raise ValueError(f"temperature must be in (0, inf), got {temperature}")
        if actor_only and critic:
            raise ValueError("policy: actor_only=True needs critic=False (an actor-only batch has no critic graph)")
        tempered = not greedy and (float(temperature) != 1.0 or row_offset is not None)
        if greedy and row_offset is not None:
            row_offset = None  # argmax draws nothing
        B = st.num_envs
        A, M = self.A, self.M
        act = torch.empty((B, A) if self.mode == 0 else (B, A, M), dtype=torch.int32, device=self.device)
        logp = torch.empty(act.shape, dtype=torch.float32, device=self.device)
        val = torch.empty((B,), dtype=torch.float32, device=self.device)
        W = M + 1 if self.mode == 0 else 2
        # the chunk boundaries decide the sampled actions when the chunk index is in the counter (below)
        chunk = self.actor_chunk if actor_only and (greedy or row_offset is not None) else self.chunk
        for c, (b0, b1) in enumerate(spans(B, chunk)):
            gb = self._batch(st.problem_idx[b0:b1], st.variable_assignments[b0:b1], ACTOR if actor_only else FULL)
            logits, value, _ = self.net.forward(gb, critic=critic)
            if critic:
                val[b0:b1] = value
            rows = logits.numel() // W
            if tempered:
                inv_t = 1.0 / float(temperature)
                if row_offset is None:
                    _lib.check(L_.msat_sample_actions_t(logits.data_ptr(), rows, W, inv_t, key.seed,
                                                        (key.counter << 16) + c, act[b0:b1].data_ptr(),
                                                        logp[b0:b1].data_ptr(), _lib.stream_ptr(self.device)),
                               "msat_sample_actions_t")
                else:  # rows per env = rows // (b1 - b0); no chunk index: the row names its stream
                    _lib.check(L_.msat_sample_actions_from(logits.data_ptr(), rows, W,
                                                           (int(row_offset) + b0) * (rows // (b1 - b0)), inv_t,
                                                           key.seed, key.counter << 16, act[b0:b1].data_ptr(),
                                                           logp[b0:b1].data_ptr(), _lib.stream_ptr(self.device)),
                               "msat_sample_actions_from")
                continue
            _lib.check(L_.msat_sample_actions(logits.data_ptr(), rows, W, 1 if greedy else 0, key.seed,
                                              (key.counter << 16) + c, act[b0:b1].data_ptr(), logp[b0:b1].data_ptr(),
                                              _lib.stream_ptr(self.device)), "msat_sample_actions")
        return act, logp, val

    def critic_values(self, pidx: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        n = pidx.shape[0]
        out = torch.empty((n,), dtype=torch.float32, device=self.device)
        for b0, b1 in spans(n, self.chunk * (self.A + 1)):  # critic-only samples are ~A+1 times smaller
            _, v, _ = self.net.forward(self._batch(pidx[b0:b1], x[b0:b1], GRAPH0), actor=False)
            out[b0:b1] = v
        return out

    # ------------------------------------------------------------- rollout ----
    def rollout(self, rs: RunnerState) -> RunnerState:
        tr, env = self.tr, self.env
        out_views = [{k: tr[k][t] for k in ("reward", "done", "solved", "num_unsatisfied", "episode_step")}
                     for t in range(self.T)]
        for t in range(self.T):
            st = rs.env_state
            tr["pidx"][t].copy_(st.problem_idx)
            tr["x"][t].copy_(st.variable_assignments)
            rs.rng, k_act, k_env = (lambda ks: (ks[0], ks[1], ks[2]))(split(rs.rng, 3))
            act, logp, val = self.policy(st, k_act)
            tr["action"][t].copy_(act)
            tr["log_prob"][t].copy_(logp)
            tr["value"][t].copy_(val)
            obs, _ = env.step_raw(st, tr["action"][t], autoreset=True, key=k_env, obs=rs.obs, out=out_views[t])
            rs.rollout_counter += 1
        return rs

    # ----------------------------------------------------------------- GAE ----
    def compute_advantages(self, rs: RunnerState):
        self.last_val.copy_(self.critic_values(rs.env_state.problem_idx, rs.env_state.variable_assignments))
        c = self.cfg
        device_gae(self.tr["reward"], self.tr["value"], self.tr["done"], self.last_val, c["GAMMA"], c["GAE_LAMBDA"],
                   normalize=False, out=(self.adv, self.targets))
        n = self.adv.numel()
        _lib.check(L_.msat_moments(self.adv.data_ptr(), n, self.moments.data_ptr(), self.mom_ws.data_ptr(),
                                   _lib.stream_ptr(self.device)), "msat_moments")
        mean, std = global_moments(self.moments, n, self.dist)
        _lib.check(L_.msat_standardize(self.adv.data_ptr(), n, mean, std, _lib.stream_ptr(self.device)),
                   "msat_standardize")

    # ------------------------------------------------------------- update ----
    def minibatch_grad(self, idx: torch.Tensor, ent: float, sums: torch.Tensor, mb_size: int) -> None:
        """net.grads = d(loss)/d(params) of the PPO loss (learner:597-645) over the flat transition rows
        ``idx``; ``sums`` (3,) fp64 accumulates (value, actor, entropy) row sums.  Loss means divide by
        ``mb_size`` (the minibatch size), so micro-batch gradients add up to the minibatch's."""
        c, net, dev = self.cfg, self.net, self.device
        A, M = self.A, self.M
        idx = idx.to(torch.int32)
        net.grads.zero_()
        for m0, m1, tot in self.micro_batches(self.tr["pidx"].reshape(-1).index_select(0, idx.long()), self.micro):
            mi = idx[m0:m1]
            S = mi.numel()
            pidx, x, act, olp, g_, vold, tg = self.gather_rows(mi)
            gb = self._batch(pidx, x, totals=tot)
            logits, value, state = net.forward(gb, save=True)
            dlog = torch.empty_like(logits)
            dval = torch.empty_like(value)
            rows = torch.empty((2 * S * A + S,), device=dev)
            _lib.check(L_.msat_ppo_loss(
                logits.data_ptr(), S, A, M, self.mode, net.base, net.rem, act.data_ptr(), olp.data_ptr(),
                g_.data_ptr(), value.data_ptr(), vold.data_ptr(), tg.data_ptr(), float(c["CLIP_EPS"]),
                float(c["VF_CLIP"]), ent, float(c["VF_COEF"]), mb_size, dlog.data_ptr(), dval.data_ptr(),
                rows.data_ptr(), sums.data_ptr(), _lib.stream_ptr(dev)), "msat_ppo_loss")
            net.backward(gb, state, dlog, dval)
            del state

    def gather_rows(self, idx: torch.Tensor):
        """The transition rows ``idx`` (int32, device) of the flat (T*B) buffers, in one launch
        (msat_gather_rows): (pidx, x, action, log_prob, advantage, value, target)."""
        return gather_rows(idx, [self.tr["pidx"], self.tr["x"], self.tr["action"], self.tr["log_prob"], self.adv,
                                 self.tr["value"], self.targets], lead=2)

    def ppo_update(self, update_idx: int, generator: torch.Generator):
        c, net, dev = self.cfg, self.net, self.device
        N, MB, E = self.T * self.B, self.MB, int(c["UPDATE_EPOCHS"])
        ent = ent_coef_at(update_idx, c)
        losses = torch.zeros((E, self.n_minibatches, 3), dtype=torch.float64, device=dev)
        A, M = self.A, self.M
        n_ent = MB * A * (M if self.mode == 1 else 1)
        for e in range(E):
            perm = self.permutation(generator)
            for k in range(self.n_minibatches):
                idx = perm[k * MB:(k + 1) * MB]
                self.minibatch_grad(idx, ent, losses[e, k], MB)
                scale = allreduce_grads(net.grads, self.dist)
                lr = learning_rate_at(net.adam_count, c)
                if self.trace is not None:
                    self.trace.append({"idx": idx.cpu(), "params": net.params.clone(),
                                       "grads": net.grads.clone() * scale, "lr": lr})
                net.adam_step(lr, grad_scale=scale, first_bad=self.first_bad)
        self.check_finite()
        # per-minibatch means over the UNION minibatch (learner:708-719 reports each minibatch's loss
        # triple over the whole minibatch): the row sums of every rank are added once per cycle, then
        # divided by the union's row counts (every rank's slice has MB rows)
        allreduce_sums(losses, self.dist)
        w = self.world
        losses[..., 0] /= MB * w
        losses[..., 1] /= MB * A * w
        losses[..., 2] /= n_ent * w
        return losses, ent

    # ------------------------------------------------------------ metrics ----
    def metrics(self, losses, ent):
        tr, dev = self.tr, self.device
        N = self.T * self.B
        vpred = self.critic_values(tr["pidx"].reshape(N), tr["x"].reshape(N, -1))
        out = torch.empty((11,), dtype=torch.float64, device=dev)
        # out[0..9) = sums over the transitions (msat_cycle_metrics), then the env and row counts
        _lib.check(L_.msat_cycle_metrics(N, tr["reward"].data_ptr(), tr["done"].data_ptr(), tr["solved"].data_ptr(),
                                         tr["num_unsatisfied"].data_ptr(), tr["episode_step"].data_ptr(),
                                         self.targets.data_ptr(), vpred.data_ptr(), out.data_ptr(),
                                         _lib.stream_ptr(dev)), "msat_cycle_metrics")
        out[9] = float(self.B)
        out[10] = float(N)
        allreduce_sums(out, self.dist)
        o = out.tolist()
        s = [o[0], o[9], o[1], o[2], o[3], o[4]]  # reward, envs, done, solved, unsat*done, steps*solved
        t1, t2, d1, d2, n = o[5], o[6], o[7], o[8], o[10]
        var_t = t2 / n - (t1 / n) ** 2
        var_d = d2 / n - (d1 / n) ** 2
        lc = losses.cpu().numpy()
        return {
            "mean_episodic_return": s[0] / s[1],
            "solve_rate": s[3] / max(s[2], 1.0),
            "avg_unsatisfied_clauses": s[4] / max(s[2], 1.0),
            "avg_steps_to_solve": s[5] / max(s[3], 1.0),
            "explained_variance": 1.0 - var_d / max(var_t, 1e-8),
            "epoch_value_losses": lc[..., 0],
            "epoch_actor_losses": lc[..., 1],
            "epoch_entropies": lc[..., 2],
            "current_ent_coef": ent,
        }

    def train_cycle(self, rs: RunnerState, update_idx: int, generator: torch.Generator):
        rs = self.rollout(rs)
        self.compute_advantages(rs)
        losses, ent = self.ppo_update(update_idx, generator)
        return rs, self.metrics(losses, ent)


def make_train_cycle(config, env: SATEnv, network: GNNActorCritic, pool: ProblemPool, dist=None):
    """learner:381-732 — returns (learner, train_cycle(runner_state, update_idx, generator))."""
    learner = MAPPOLearner(config, env, network, pool, dist=dist)
    return learner, learner.train_cycle


# reference class name (learner:198)
GNN_ActorCritic = GNNActorCritic
