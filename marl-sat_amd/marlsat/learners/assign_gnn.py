"""Assignment predictor on the device: the shared encoder and one head that gives every variable two logits,
"false" and "true" in an expert solution (src/learners/bc_learner.py, src/runners/bc_runner.py).

The reference's model class (``src.models.base_gnn.SATGNN``) is not in the reference tree, so, as for the single-agent
baseline (single_gnn.py), the head is this project's on the encoder every network here shares:

  * the encoder is ``GNNActorCritic``'s, unchanged (same kernels, precision switches, launch layer, ``adam_step``),
    on the sample's graph 0 -- all V variables, all C clauses;
  * per variable row ``relu([H_v+ | H_v-] @ s0_w + s0_b) -> relu(. @ s1_w + s1_b) -> . @ so_w + so_b`` with widths
    2H -> 128 -> 64 -> 2: single_gnn.py's actor head (``VarRowsHead``) with a 2-wide last layer.

The input is a critic-only graph batch (``assemble(..., critic_only=True)``): graph 0's variable rows are the
instance's variables in order, so the head's (S * V, 2) output is ``msat_assign_loss``'s logit matrix as it stands.
There is no critic, no id embedding and no parameter whose shape depends on V, C or an agent split: one parameter
buffer serves batches of any V (one V per batch), DESIGN.md §17.
"""
from __future__ import annotations

from . import params as P
from .gnn import GNNActorCritic, HeadTape
from .graphs import GraphBatch
from .single_gnn import VarRowsHead


class GNNAssignmentPredictor(VarRowsHead, GNNActorCritic):
    """Encoder + per-variable two-class head (params.assign_layout); size-free."""

    def __init__(self, gnn_hidden_dim: int, gnn_num_message_passing_steps: int, device=None, seed: int = 0):
        # the parent's per-agent bookkeeping (A, M, base, rem) is unused: no head of this network reads it
        super().__init__(gnn_hidden_dim, gnn_num_message_passing_steps, 1, 1, 0, 1, device=device, seed=seed)
        self.V = None  # no size of its own

    def _spec(self) -> P.Spec:
        return P.assign_spec(self.H, self.L)

    # ------------------------------------------------------------ heads ----
    def actor_head(self, b: GraphBatch, Hp, Hn, Hc, ht: HeadTape):
        return self._var_rows_head(b, Hp, Hn, ht, "assign", self._e(b.Nv, 2), 2)

    def actor_head_backward(self, b, ht: HeadTape, dlogits, dHp, dHn, dHc):
        self._var_rows_head_backward(b, ht, dlogits, dHp, dHn, "assign", 2)

    def critic_head(self, *a, **k):
        raise ValueError("GNNAssignmentPredictor has no critic head")

    def _check_heads(self, b: GraphBatch, actor: bool, critic: bool, what: str):
        """The head reads graph 0 alone: the batch must be critic-only, its variable rows sample-major (S, V) for
        one V, whatever that V is."""
        if critic:
            raise ValueError(f"{what}: the assignment predictor has no critic (forward(critic=False), dvalue None)")
        if b.g0 != 0 or b.G != 1:
            raise ValueError(f"{what}: the assignment predictor takes a critic-only batch (graph 0 alone, G = 1), "
                             f"got graphs {b.g0}..{b.g0 + b.G - 1}")
        if b.S < 1 or b.Nv % b.S:
            raise ValueError(f"{what}: the batch's {b.Nv} variable rows are not {b.S} samples of one size")

    def forward(self, b: GraphBatch, actor: bool = True, critic: bool = False, save: bool = False):
        """-> (logits (S * V, 2), None, state).  ``critic=True`` raises."""
        return super().forward(b, actor, critic, save)
