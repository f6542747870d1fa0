"""float64 restatements of the assignment predictor's device pieces (torch / NumPy on the CPU), the references of
tests/test_assign_*_gpu.py: the network's head (GNNAssignmentPredictor) on oracle/net.py's encoder, and the
per-variable two-class cross-entropy (msat_assign_loss) as a differentiable torch function."""
import numpy as np
import torch

from oracle import net as onet


def assign_param_shapes(H, L):
    """Flax param tree of GNNAssignmentPredictor: oracle.net's encoder and the three head layers."""
    s = {k: v for k, v in onet.param_shapes(H, L, 1, 1).items() if k.startswith("encoder/")}
    s["assign_dense_0/kernel"], s["assign_dense_0/bias"] = (2 * H, 128), (128,)
    s["assign_dense_1/kernel"], s["assign_dense_1/bias"] = (128, 64), (64,)
    s["assign_output/kernel"], s["assign_output/bias"] = (64, 2), (2,)
    return s


def assign_logits(P, L, svf, x, cf, A_pos, A_neg):
    """Three dense layers on [H_v+ | H_v-] of every variable -> (B, V, 2) logits.  (oracle.net's own dense / relu, so
    that kink_bound sees the head's ReLUs.)"""
    Hp, Hn, _ = onet.encoder(P, L, svf, x, cf, A_pos, A_neg)
    h = onet._relu(onet._dense(P, "assign_dense_0", torch.cat([Hp, Hn], -1)))
    h = onet._relu(onet._dense(P, "assign_dense_1", h))
    return onet._dense(P, "assign_output", h)


def graph_args(pool, inst, x, V, C):
    """oracle.net's encoder inputs (svf, x, cf, A_pos, A_neg) for samples (inst, x) of an (N, C, 3) pool."""
    from oracle.sat_env import OracleSATEnv

    ora = OracleSATEnv(V, C, 10, vars_per_agent=V)
    _, ost = ora.reset(pool[inst], x.astype(np.int32))
    Ap, An = onet.dense_graph(pool[inst], V)
    return (torch.from_numpy(ora.static_var_features(pool[inst])).double(), torch.from_numpy(x).double(),
            torch.from_numpy(ora.clause_features(ost)).double(), Ap, An)


def assign_nll(logits, labels):
    """Per-row -log softmax(logits)[label] for logits (..., 2) (torch, differentiable) and labels (...) in {0, 1}:
    softplus(-d) with d = l[label] - l[1 - label], the form msat_assign_loss states."""
    lab = labels.long()
    own = torch.gather(logits, -1, lab[..., None])[..., 0]
    other = torch.gather(logits, -1, (1 - lab)[..., None])[..., 0]
    d = own - other
    return torch.clamp(-d, min=0.0) + torch.log1p(torch.exp(-d.abs()))


def assign_loss(logits, labels, minibatch):
    """bc_learner.py:28-31: the mean over (batch, variable) of the two-class cross-entropy, the batch mean dividing
    by ``minibatch``.  logits (B, V, 2), labels (B, V)."""
    return assign_nll(logits, labels).sum() / float(minibatch * logits.shape[1])
