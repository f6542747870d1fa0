"""float64 restatements of the single-agent PPO baseline's device pieces (torch / NumPy on the CPU), the references
of tests/test_single_*_gpu.py and tests/test_clip_global_norm_gpu.py: the loss (msat_ppo_single_loss), the
population standardisation, clip_by_global_norm, the shared-encoder network's head (GNNSingleActorCritic), the
learning-rate schedule and the episode bookkeeping.  Built on oracle/net.py (encoder, critic, clip, log_softmax,
entropy, adam_update) so that ties and clip edges follow the conventions msat_ppo_loss is held to."""
import numpy as np
import torch

from oracle import net as onet


# ------------------------------------------------------------------------ loss ----
def single_terms(lg, val, action, old_logp, adv, targets, clip_eps):
    """Per-row (actor, vl, ent, ratio, lp) of single_rl_learner.py:118-158 on torch tensors (differentiable in lg and
    val): oracle.net's clip / log_softmax / entropy, so ties and clip edges follow msat_ppo_loss' conventions."""
    lp = torch.gather(onet.log_softmax(lg), -1, action.long()[:, None])[:, 0]
    ratio = torch.exp(lp - old_logp)
    actor = -torch.minimum(ratio * adv, onet.clip(ratio, 1.0 - clip_eps, 1.0 + clip_eps) * adv)
    return actor, (val - targets) ** 2, onet.entropy(lg), ratio, lp


def single_total(terms, ent_coef, vf_coef, minibatch):
    actor, vl, ent = terms[:3]
    return (actor.sum() + vf_coef * vl.sum() - ent_coef * ent.sum()) / float(minibatch)


def single_loss(logits, action, old_logp, adv, value, targets, clip_eps, ent_coef, vf_coef, minibatch):
    """single_rl_learner.py:118-158 in float64 on the given (fp32) inputs.  logits (S, V), the rest (S,).
    -> dict: dlogits (S, V), dvalue (S,), terms (S, 3) = (actor, vl, ent), valid (S,), ratio (S,), lp (S,).
    Rows whose action is outside [0, V) are invalid: zeros throughout, and none of their other inputs is used.
    clip_eps / ent_coef / vf_coef are taken as the float32 values the device receives, widened."""
    S, V = logits.shape
    a = np.asarray(action, np.int64)
    valid = (a >= 0) & (a < V)
    vt = torch.from_numpy(valid)
    f64 = lambda x: torch.from_numpy(np.asarray(x, np.float64).copy())
    zero_rows = lambda x: np.where(valid, np.asarray(x, np.float64), 0.0)  # an invalid row's inputs are not read
    lg = f64(np.where(valid[:, None], np.asarray(logits, np.float64), 0.0)).requires_grad_(True)
    val = f64(zero_rows(value)).requires_grad_(True)
    eps, ec, vc = (float(np.float32(c)) for c in (clip_eps, ent_coef, vf_coef))
    actor, vl, ent, ratio, lp = single_terms(lg, val, torch.from_numpy(np.clip(a, 0, V - 1)), f64(zero_rows(old_logp)),
                                             f64(zero_rows(adv)), f64(zero_rows(targets)), eps)
    z = torch.zeros((), dtype=torch.float64)
    actor, vl, ent = (torch.where(vt, t, z) for t in (actor, vl, ent))
    total = single_total((actor, vl, ent), ec, vc, minibatch)
    total.backward()
    return {"dlogits": lg.grad.numpy(), "dvalue": val.grad.numpy(),
            "terms": torch.stack([actor, vl, ent], 1).detach().numpy(), "valid": valid,
            "ratio": ratio.detach().numpy(), "lp": lp.detach().numpy(), "total": float(total.detach())}


def near_kink(ratio, clip_eps, valid, tol=1e-6):
    """Rows whose float64 ratio lies within tol of a clip edge: the surrogate's gradient jumps there."""
    eps = float(np.float32(clip_eps))
    return valid & ((np.abs(ratio - (1.0 - eps)) <= tol) | (np.abs(ratio - (1.0 + eps)) <= tol))


# ----------------------------------------------------- standardise / clip ----
def standardize_pop(x):
    """single_rl_learner.py:142 in float64: (x - mean) / (std + 1e-8), population std."""
    x = np.asarray(x, np.float64)
    return (x - x.mean()) / (x.std() + 1e-8)


def global_norm(g):
    return float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2)))


def clip_global_norm(g, max_norm):
    """optax.clip_by_global_norm in float64 -> (clipped, norm, touched); norm < max_norm leaves g as it is."""
    g64 = np.asarray(g, np.float64)
    norm = global_norm(g64)
    m = float(np.float32(max_norm))
    if norm < m:
        return g64.copy(), norm, False
    return g64 * (m / norm), norm, True


# -------------------------------------------------------------- schedule ----
def single_lr(count, lr, anneal, total_steps):
    """single_rl_learner.py:52-60: linear decay to 0 over the run's Adam steps, from the steps already taken."""
    return lr * max(0.0, 1.0 - count / total_steps) if anneal else lr


# ----------------------------------------------------------------- network ----
def single_param_shapes(H, L):
    """Flax param tree of GNNSingleActorCritic: oracle.net's encoder and critic head, and the three actor layers."""
    s = {k: v for k, v in onet.param_shapes(H, L, 1, 1).items() if k.startswith(("encoder/", "critic_"))}
    s["actor_dense_1/kernel"], s["actor_dense_1/bias"] = (2 * H, 128), (128,)
    s["actor_dense_2/kernel"], s["actor_dense_2/bias"] = (128, 64), (64,)
    s["actor_output/kernel"], s["actor_output/bias"] = (64, 1), (1,)
    return s


def single_logits(P, L, svf, x, cf, A_pos, A_neg):
    """The shared-encoder actor head of GNNSingleActorCritic: three dense layers on [H_v+ | H_v-] of every
    variable -> (B, V) logits.  (oracle.net's own dense / relu, so that kink_bound sees the head's ReLUs.)"""
    Hp, Hn, _ = onet.encoder(P, L, svf, x, cf, A_pos, A_neg)
    h = onet._relu(onet._dense(P, "actor_dense_1", torch.cat([Hp, Hn], -1)))
    h = onet._relu(onet._dense(P, "actor_dense_2", h))
    return onet._dense(P, "actor_output", h)[..., 0]


def single_forward(P, L, args):
    """(logits (B, V), value (B,)) of the single-agent network on args = (svf, x, cf, A_pos, A_neg)."""
    return single_logits(P, L, *args), onet.critic(P, L, *args)


# ------------------------------------------------------------- evaluation ----
def episode_track(rewards, dones, solveds):
    """single_rl_runner.py:218-229 without auto-reset, as a loop: rewards (T, B) float32, dones / solveds (T, B).
    -> ret (B,) float32 accumulated in step order, len (B,), solved (B,), finished (B,)."""
    T, B = rewards.shape
    ret = np.zeros(B, np.float32)
    ln = np.zeros(B, np.int32)
    sv = np.zeros(B, np.uint8)
    fin = np.zeros(B, np.uint8)
    for t in range(T):
        for b in range(B):
            if fin[b]:
                continue
            ret[b] = np.float32(ret[b] + np.float32(rewards[t, b]))
            if dones[t, b]:
                ln[b], sv[b], fin[b] = t + 1, 1 if solveds[t, b] else 0, 1
    return ret, ln, sv, fin
