"""Single-agent PPO baseline on the device -- drop-in for ``collect_rollouts`` / ``evaluate_policy``
(src/runners/single_rl_runner.py:94-245) and ``make_update`` (src/learners/single_rl_learner.py:72-199).

One agent flips one of all V variables per step (``SatEnv``'s kernel path: vars_per_agent = V, action mode 0,
``MSAT_REWARD_SINGLE_DELTA``).  One ``train_cycle`` is a cycle of the reference's loop (runner:372-428):
  1. every env is reset onto a freshly drawn pool instance (runner:376-395), then NUM_STEPS batched steps: policy +
     value forward of ``GNNSingleActorCritic`` on the current states (ONE encoder pass per sample), Categorical
     sampling, fused env step with auto-reset;
  2. bootstrap value and GAE (learner:82-104), not normalised globally;
  3. UPDATE_EPOCHS x NUM_MINIBATCHES minibatch steps (learner:161-195).  Per minibatch: its advantages are
     standardised over the WHOLE minibatch (learner:142, msat_moments + msat_standardize_pop, on the device), then
     micro-batches of forward -> msat_ppo_single_loss -> backward add up to the minibatch's gradient (exact: the
     loss means divide by the minibatch size), then clip_by_global_norm and Adam(eps = 1e-5) (learner:52-60).
Transitions store (instance id, assignment), as in the MAPPO learner; the graph is re-derived on the device.  Inside
the minibatch loop the host reads the device once (the micro-batches' row totals, graphs.batch_totals).
Single process only.  Deviations from the reference are listed in DESIGN.md §16.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from .. import _lib
from ..envs.multi_agent_sat_env import ProblemPool, SATEnv, SATState
from ..random import Key, as_key, split
from .base import GRAPH0, Learner, gather_rows, spans
from .ops import gae as device_gae
from .single_gnn import GNNSingleActorCritic

L_ = _lib.lib
ADAM_EPS = 1e-5  # optax.adam(..., eps=1e-5), learner:52-60


def total_adam_steps(config: dict) -> int:
    """The schedule's horizon (learner:38-43): cycles x epochs x minibatches."""
    return int(config["NUM_CYCLES"]) * int(config["UPDATE_EPOCHS"]) * int(config["NUM_MINIBATCHES"])


def learning_rate_at(count: int, config: dict) -> float:
    """learner:36-50: LR * max(0, 1 - count / total) with ``count`` the Adam steps already taken; constant LR
    without ANNEAL_LR."""
    lr = float(config["LR"])
    if not config.get("ANNEAL_LR", False):
        return lr
    return lr * max(0.0, 1.0 - count / total_adam_steps(config))


def max_grad_norm(config: dict) -> float:
    """learner:52-60: clip_by_global_norm(1.0) under the schedule, 0.5 at a constant rate; MAX_GRAD_NORM overrides."""
    v = config.get("MAX_GRAD_NORM")
    return float(v) if v is not None else (1.0 if config.get("ANNEAL_LR", False) else 0.5)


def make_single_env(num_vars: int, num_clauses: int, max_steps: int, c_bonus: float, device=None) -> SATEnv:
    """The kernel-path env under ``marlsat.envs.sat_env.SatEnv``: one agent owning every variable."""
    return SATEnv(num_vars, num_clauses, max_steps, vars_per_agent=num_vars, action_mode=0, r_sat=float(c_bonus),
                  reward_mode=_lib.REWARD_SINGLE_DELTA, device=device)


@dataclass
class SingleRunnerState:
    env_state: Optional[SATState]
    rng: Key


class SinglePPOLearner(Learner):
    """``trace``: a list receives, per Adam step, the minibatch rows, the parameters it started from, the normalised
    advantages, the gradient before and after the clip, the norm before the clip (a device scalar) and the learning
    rate; and per reset and env step its key."""

    name = "single PPO"

    def __init__(self, config: dict, env: SATEnv, network: GNNSingleActorCritic, pool: ProblemPool,
                 micro_bytes: Optional[float] = None, templates: str = "host"):
        if env.num_agents != 1 or env.action_mode != 0 or env.reward_mode != _lib.REWARD_SINGLE_DELTA:
            raise ValueError("SinglePPOLearner: the env must be the single-agent one (make_single_env: vars_per_agent "
                             "= V, action mode 0, REWARD_SINGLE_DELTA)")
        if pool.num_vars != env.num_vars or pool.num_clauses != env.num_clauses:
            raise ValueError(f"pool is V={pool.num_vars}, C={pool.num_clauses}; env is V={env.num_vars}, "
                             f"C={env.num_clauses}")
        self._init_shared(config, network, env.device, templates, micro_bytes)
        self.env = env
        self.B, self.T = int(config["NUM_ENVS"]), int(config["NUM_STEPS"])
        self.V = env.num_vars
        self.n_minibatches, self.epochs = int(config["NUM_MINIBATCHES"]), int(config["UPDATE_EPOCHS"])
        N = self.T * self.B
        if self.n_minibatches < 1 or N % self.n_minibatches:
            raise ValueError(f"NUM_STEPS*NUM_ENVS={N} must be divisible by NUM_MINIBATCHES={self.n_minibatches} "
                             f"(learner:169-172 reshapes the shuffled batch into equal minibatches)")
        self.MB = N // self.n_minibatches
        self.max_norm = max_grad_norm(config)
        if not (0.0 < self.max_norm < float("inf")):
            raise ValueError(f"MAX_GRAD_NORM must be positive and finite, got {self.max_norm}")
        self._plan_pool(pool, GRAPH0, env.num_vars, 1, self.MB, self.B)
        self.minibatch_terms = None  # the last update's per-minibatch (actor, vl, ent) means, Adam-step order
        self.grad_norms = None  # the last update's pre-clip norms, Adam-step order (numpy)
        self._alloc_rollout(self.T, self.B, self.V, (self.T, self.B))
        self.clip_ws = torch.zeros((int(L_.msat_clip_global_norm_workspace_doubles(self.net.size)),),
                                   dtype=torch.float64, device=self.device)

    # -------------------------------------------------------------- policy ----
    def init_runner_state(self, key) -> SingleRunnerState:
        return SingleRunnerState(None, as_key(key))

    def _reset(self, key: Key, problem_idx=None, assignments=None, num_envs: Optional[int] = None) -> SATState:
        n = self.B if num_envs is None else num_envs
        _, st = self.env.reset_from_pool(self.pool, n, key, problem_idx=problem_idx, assignments=assignments,
                                         with_obs=False)
        # No reset queue: it lists an env for a reset workgroup when next_step + 1 >= max_steps, the multi-agent
        # time-out rule; under SINGLE_DELTA an env is done only at step0 >= max_steps (sat_env.py:106), so a listed
        # env would be reset one step early, with done = 0.
        st.reset_queue = None
        return st

    def policy(self, st: SATState, key: Key, greedy: bool = False):
        """Logits and value of the current states in inference chunks (graph 0 alone), then Categorical sampling
        (argmax when greedy): actions (B, 1) int32, log_probs (B,), values (B,)."""
        B, V, dev = st.num_envs, self.V, self.device
        act = torch.empty((B, 1), dtype=torch.int32, device=dev)
        logp = torch.empty((B,), dtype=torch.float32, device=dev)
        val = torch.empty((B,), dtype=torch.float32, device=dev)
        for c, (b0, b1) in enumerate(spans(B, self.chunk)):
            logits, value, _ = self.net.forward(self._batch(st.problem_idx[b0:b1], st.variable_assignments[b0:b1]))
            val[b0:b1] = value
            _lib.check(L_.msat_sample_actions(logits.data_ptr(), b1 - b0, V, 1 if greedy else 0, key.seed,
                                              (key.counter << 16) + c, act[b0:b1].data_ptr(), logp[b0:b1].data_ptr(),
                                              _lib.stream_ptr(dev)), "msat_sample_actions")
        return act, logp, val

    def values(self, st: SATState) -> torch.Tensor:
        out = torch.empty((st.num_envs,), dtype=torch.float32, device=self.device)
        for b0, b1 in spans(st.num_envs, self.chunk):
            _, v, _ = self.net.forward(self._batch(st.problem_idx[b0:b1], st.variable_assignments[b0:b1]),
                                       actor=False)
            out[b0:b1] = v
        return out

    # ------------------------------------------------------------- rollout ----
    def rollout(self, rs: SingleRunnerState) -> SingleRunnerState:
        """runner:376-403 + :94-189: all envs onto fresh pool instances, then T steps with auto-reset."""
        tr, env = self.tr, self.env
        rs.rng, k_reset = split(rs.rng, 2)
        rs.env_state = st = self._reset(k_reset)
        if self.trace is not None:
            self.trace.append({"kind": "reset", "key": k_reset})
        out_views = [{k: tr[k][t] for k in ("reward", "done", "solved", "num_unsatisfied", "episode_step")}
                     for t in range(self.T)]
        for t in range(self.T):
            tr["pidx"][t].copy_(st.problem_idx)
            tr["x"][t].copy_(st.variable_assignments)
            rs.rng, k_act, k_env = split(rs.rng, 3)
            act, logp, val = self.policy(st, k_act)
            tr["action"][t].copy_(act[:, 0])
            tr["log_prob"][t].copy_(logp)
            tr["value"][t].copy_(val)
            if self.trace is not None:
                self.trace.append({"kind": "step", "t": t, "key": k_env})
            env.step_raw(st, act, autoreset=True, key=k_env, with_obs=False, out=out_views[t])
        return rs

    def compute_advantages(self, rs: SingleRunnerState) -> None:
        """Bootstrap value + GAE (learner:82-104); the advantages stay raw (normalised per minibatch)."""
        self.last_val.copy_(self.values(rs.env_state))
        c = self.cfg
        device_gae(self.tr["reward"], self.tr["value"], self.tr["done"], self.last_val, c["GAMMA"], c["GAE_LAMBDA"],
                   normalize=False, out=(self.adv, self.targets))

    # -------------------------------------------------------------- update ----
    def gather_rows(self, idx: torch.Tensor):
        """The transition rows ``idx`` (int32, device) of the flat (T*B) buffers in one launch (msat_gather_rows):
        (pidx, x, action, log_prob, advantage, target)."""
        return gather_rows(idx, [self.tr["pidx"], self.tr["x"], self.tr["action"], self.tr["log_prob"], self.adv,
                                 self.targets], lead=2)

    def minibatch_grad(self, idx: torch.Tensor, sums: torch.Tensor) -> torch.Tensor:
        """net.grads = d(loss)/d(params) of the PPO loss (learner:118-158) over the flat transition rows ``idx``;
        ``sums`` (4,) fp64 accumulates (actor, vl, ent, invalid rows).  Returns the minibatch's normalised
        advantages."""
        c, net, dev, V = self.cfg, self.net, self.device, self.V
        idx = idx.to(torch.int32).contiguous()
        MB = idx.numel()
        st = _lib.stream_ptr(dev)
        net.grads.zero_()
        pidx, x, act, olp, adv, tg = self.gather_rows(idx)
        # the normalisation is over the whole minibatch (learner:142), before it is cut into micro-batches
        _lib.check(L_.msat_moments(adv.data_ptr(), MB, self.moments.data_ptr(), self.mom_ws.data_ptr(), st),
                   "msat_moments")
        _lib.check(L_.msat_standardize_pop(adv.data_ptr(), MB, self.moments.data_ptr(), st), "msat_standardize_pop")
        for m0, m1, tot in self.micro_batches(pidx, self.micro):  # the minibatch loop's one host read
            S = m1 - m0
            gb = self._batch(pidx[m0:m1], x[m0:m1], totals=tot)
            logits, value, state = net.forward(gb, save=True)
            dlog, dval = torch.empty_like(logits), torch.empty_like(value)
            rows = torch.empty((3 * S,), device=dev)
            _lib.check(L_.msat_ppo_single_loss(
                logits.data_ptr(), S, V, act[m0:m1].data_ptr(), olp[m0:m1].data_ptr(), adv[m0:m1].data_ptr(),
                value.data_ptr(), tg[m0:m1].data_ptr(), float(c["CLIP_EPS"]), float(c["ENT_COEF"]),
                float(c["VF_COEF"]), MB, dlog.data_ptr(), dval.data_ptr(), rows.data_ptr(), sums.data_ptr(), st),
                "msat_ppo_single_loss")
            net.backward(gb, state, dlog, dval)
            del state
        return adv

    def ppo_update(self, generator: torch.Generator) -> Dict[str, float]:
        """learner:161-195 -> the cycle's loss quadruple (means over the minibatches): total, value, policy,
        entropy."""
        c, net, dev = self.cfg, self.net, self.device
        E, K, MB = self.epochs, self.n_minibatches, self.MB
        sums = torch.zeros((E, K, 4), dtype=torch.float64, device=dev)
        norms = torch.zeros((E, K), dtype=torch.float32, device=dev)
        st = _lib.stream_ptr(dev)
        for e in range(E):
            perm = self.permutation(generator)
            for k in range(K):
                idx = perm[k * MB:(k + 1) * MB]
                adv_n = self.minibatch_grad(idx, sums[e, k])
                rec = None
                if self.trace is not None:
                    rec = {"kind": "adam", "idx": idx.cpu(), "params": net.params.clone(), "adv_n": adv_n.clone(),
                           "grads": net.grads.clone(), "max_norm": self.max_norm, "count": net.adam_count}
                _lib.check(L_.msat_clip_global_norm(net.grads.data_ptr(), net.size, self.max_norm,
                                                    self.clip_ws.data_ptr(), norms[e, k].data_ptr(), st),
                           "msat_clip_global_norm")
                lr = learning_rate_at(net.adam_count, c)
                if rec is not None:
                    rec.update(clipped=net.grads.clone(), norm=norms[e, k], lr=lr)
                    self.trace.append(rec)
                net.adam_step(lr, eps=ADAM_EPS, first_bad=self.first_bad)
        self.check_finite()
        s = sums.cpu().numpy().reshape(E * K, 4)  # one read per cycle
        if s[:, 3].any():
            raise ValueError(f"single PPO: {int(s[:, 3].sum())} stored action(s) outside [0, {self.V})")
        self.minibatch_terms = s[:, :3] / MB
        self.grad_norms = norms.cpu().numpy().reshape(E * K)
        actor, vl, ent = self.minibatch_terms.mean(0)
        total = (self.minibatch_terms[:, 0] + float(c["VF_COEF"]) * self.minibatch_terms[:, 1]
                 - float(c["ENT_COEF"]) * self.minibatch_terms[:, 2]).mean()
        return {"loss_total": float(total), "loss_value": float(vl), "loss_policy": float(actor),
                "entropy": float(ent), "grad_norm": float(self.grad_norms.mean())}

    # ------------------------------------------------------------- metrics ----
    def rollout_stats(self) -> Dict[str, float]:
        """runner:399-448: value and reward mean / std over the rollout, episodes = dones + NUM_ENVS (the episodes
        the cycle started), solve rate = solved dones / episodes."""
        tr = self.tr
        done = tr["done"].bool()
        v = torch.stack([tr["value"].double().mean(), tr["value"].double().std(unbiased=False),
                         tr["reward"].double().mean(), tr["reward"].double().std(unbiased=False),
                         done.sum().double(), (done & tr["solved"].bool()).sum().double()]).tolist()
        episodes = int(v[4]) + self.B
        return {"value_mean": v[0], "value_std": v[1], "reward_mean": v[2], "reward_std": v[3],
                "train_ep_num": episodes, "train_solve_rate": v[5] / episodes if episodes else 0.0}

    def train_cycle(self, rs: SingleRunnerState, generator: torch.Generator):
        rs = self.rollout(rs)
        self.compute_advantages(rs)
        stats = self.ppo_update(generator)
        stats.update(self.rollout_stats())
        return rs, stats

    # ---------------------------------------------------------- evaluation ----
    def evaluate(self, problem_idx, max_steps: int, key=None, assignments=None, record: Optional[list] = None,
                 early_exit: bool = True):
        """runner:192-245: one greedy episode per entry of ``problem_idx`` without auto-reset, at most ``max_steps``
        steps, from random assignments (or the given ones); the bookkeeping is msat_episode_track.  Stops once every
        env has finished.  An env that never finishes counts ``max_steps`` steps and is not solved (runner:222-228).
        "Solved" is the kernel's flag at the first done.  ``record``: a list that receives per step
        (actions, rewards, dones, solveds) as host arrays; early_exit=False runs all ``max_steps`` steps (the later
        ones change no result)."""
        dev = self.device
        pidx = torch.as_tensor(problem_idx, device=dev).to(torch.int32).contiguous()
        n = int(pidx.numel())
        if n == 0:
            return {"eval_solve_rate": 0.0, "eval_avg_len": float("inf"), "eval_avg_return": 0.0, "eval_episodes": 0}
        k_reset, k_run = split(as_key(key), 2)
        st = self._reset(k_reset, problem_idx=pidx, assignments=assignments, num_envs=n)
        out = self.env._step_out(n)
        ret = torch.zeros((n,), dtype=torch.float32, device=dev)
        ln = torch.zeros((n,), dtype=torch.int32, device=dev)
        sv = torch.zeros((n,), dtype=torch.uint8, device=dev)
        fin = torch.zeros((n,), dtype=torch.uint8, device=dev)
        for t in range(int(max_steps)):
            act, _, _ = self.policy(st, k_run.fold(t), greedy=True)
            self.env.step_raw(st, act, autoreset=False, key=k_run, with_obs=False, out=out)
            _lib.check(L_.msat_episode_track(n, t, out["reward"].data_ptr(), out["done"].data_ptr(),
                                             out["solved"].data_ptr(), ret.data_ptr(), ln.data_ptr(), sv.data_ptr(),
                                             fin.data_ptr(), _lib.stream_ptr(dev)), "msat_episode_track")
            if record is not None:
                record.append(tuple(a.cpu().numpy().copy() for a in (act[:, 0], out["reward"], out["done"],
                                                                    out["solved"])))
            if early_exit and bool(fin.all()):  # evaluation is off the training path: one read per step
                break
        finished = fin.bool()
        lens = torch.where(finished, ln, torch.full_like(ln, int(max_steps)))
        self.eval_episodes = {"return": ret.cpu().numpy(), "len": lens.cpu().numpy(), "solved": sv.cpu().numpy(),
                              "finished": fin.cpu().numpy()}
        return {"eval_solve_rate": float(sv.float().mean()), "eval_avg_len": float(lens.float().mean()),
                "eval_avg_return": float(ret.mean()), "eval_episodes": n}
