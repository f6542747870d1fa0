"""Single-agent GNN actor-critic on the device: ONE encoder pass per sample feeds both heads.

The reference baseline's model (``src.models.ac_gnn.ACGNN``, single_rl_learner.py / single_rl_runner.py) is not in
the reference tree; what the runner says about it is its parameter tree (single_rl_runner.py:248-275): a GNN body,
``actor_dense_1`` / ``actor_dense_2`` / ``actor_output`` and a critic head.  So the head is this project's:

  * the encoder and the critic head are ``GNNActorCritic``'s, unchanged (same kernels, precision switches, launch
    layer and ``adam_step``), on the sample's graph 0 -- all V variables, all C clauses;
  * the actor head reads the same final variable states: per variable row
    ``relu([H_v+ | H_v-] @ s0_w + s0_b) -> relu(. @ s1_w + s1_b) -> . @ so_w + so_b`` is that variable's flip logit.

The input is a critic-only graph batch (``assemble(..., critic_only=True)``, G = 1): graph 0's variable rows are the
instance's V variables in order, so the last layer's (S * V, 1) output is the (S, V) logit matrix as it stands.  No
pool kernel, no no-op slot, no mask, no id embedding.  (The clause features are ``assemble``'s [is_sat, ntrue/3, 1],
not ``SatEnv.get_obs``' [sat, unsat, 1]: the model that consumed those is missing)
"""
from __future__ import annotations

import numpy as np
import torch

from . import params as P
from .gnn import GNNActorCritic, HeadTape
from .graphs import GraphBatch


class VarRowsHead:
    """The three-layer head over graph 0's variable rows, shared by the networks that read a critic-only batch
    (this file's actor, assign_gnn.py's predictor): per row ``relu([H_v+ | H_v-] @ s0_w + s0_b) ->
    relu(. @ s1_w + s1_b) -> . @ so_w + so_b`` with widths 2H -> 128 -> 64 -> ``nout``, the parameters under
    ``<pre>.s0 / .s1 / .so``.  Mixed into a GNNActorCritic (its launch layer and parameter views)."""

    def _var_rows_head(self, b: GraphBatch, Hp, Hn, ht: HeadTape, pre: str, out, nout: int):
        H, R, e = self.H, b.Nv, self._e
        h1, hn, h2 = e(R, 128), e(R, 128), e(R, 64)
        # [H_v+ | H_v-] @ s0_w as two products over the weight's row blocks, added and rectified in one pass
        self._linear(Hp, H, f"{pre}.s0_w", f"{pre}.s0_b", h1, 128, R, 128, H)
        self._linear(Hn, H, f"{pre}.s0_w", None, hn, 128, R, 128, H, row0=H)
        self._call("msat_bcast_add_relu", h1.data_ptr(), hn.data_ptr(), R, 1, 128)
        self._linear(h1, 128, f"{pre}.s1_w", f"{pre}.s1_b", h2, 64, R, 64, 128)
        self._call("msat_relu", h2.data_ptr(), h2.numel())
        self._linear(h2, 64, f"{pre}.so_w", f"{pre}.so_b", out, nout, R, nout, 64)
        ht.my, ht.h1, ht.h2 = (Hp, Hn), h1, h2
        return out

    def _var_rows_head_backward(self, b: GraphBatch, ht: HeadTape, dout, dHp, dHn, pre: str, nout: int):
        H, R, e = self.H, b.Nv, self._e
        Hp, Hn = ht.my
        dh2, dh1 = e(R, 64), e(R, 128)
        self._linear_backward(ht.h2, 64, f"{pre}.so_w", f"{pre}.so_b", dout, nout, R, nout, 64, dx=dh2, lddx=64)
        self._call("msat_relu_bwd", dh2.data_ptr(), ht.h2.data_ptr(), dh2.numel())
        self._linear_backward(ht.h1, 128, f"{pre}.s1_w", f"{pre}.s1_b", dh2, 64, R, 64, 128, dx=dh1, lddx=128)
        self._call("msat_relu_bwd", dh1.data_ptr(), ht.h1.data_ptr(), dh1.numel())
        # on top of what dHp / dHn already hold (the critic head's backward, or zeros)
        self._linear_backward(Hp, H, f"{pre}.s0_w", f"{pre}.s0_b", dh1, 128, R, 128, H, dx=dHp, lddx=H, acc=1)
        self._linear_backward(Hn, H, f"{pre}.s0_w", None, dh1, 128, R, 128, H, dx=dHn, lddx=H, acc=1, row0=H)


class GNNSingleActorCritic(VarRowsHead, GNNActorCritic):
    """Shared-encoder actor-critic over all V variables (params.single_layout)."""

    def __init__(self, gnn_hidden_dim: int, gnn_num_message_passing_steps: int, num_vars: int, device=None,
                 seed: int = 0):
        # one agent owning every variable, action mode 0: what the parent's bookkeeping (base, rem) then holds
        super().__init__(gnn_hidden_dim, gnn_num_message_passing_steps, 1, num_vars, 0, num_vars, device=device,
                         seed=seed)

    def _spec(self) -> P.Spec:
        return P.single_spec(self.H, self.L)

    def reset_heads(self, seed: int) -> None:
        """Both heads back to ``seed``'s initial draw (the resume rule, single_rl_runner.py:248-275); the optimiser
        state is the caller's to clear."""
        fresh = torch.from_numpy(self.spec.init_flat(seed)).to(self.device)
        for head in P.SINGLE_HEADS:
            for sfx in ("_w", "_b"):
                o, shp = self.tab[head + sfx]
                n = int(np.prod(shp))
                self.params[o: o + n].copy_(fresh[o: o + n])

    # ------------------------------------------------------------ heads ----
    def actor_head(self, b: GraphBatch, Hp, Hn, Hc, ht: HeadTape):
        return self._var_rows_head(b, Hp, Hn, ht, "actor", self._e(b.S, self.V), 1)

    def actor_head_backward(self, b, ht: HeadTape, dlogits, dHp, dHn, dHc):
        self._var_rows_head_backward(b, ht, dlogits, dHp, dHn, "actor", 1)

    def _check_heads(self, b: GraphBatch, actor: bool, critic: bool, what: str):
        """Both heads read graph 0 alone: the batch must be critic-only, its variable rows sample-major (S, V)."""
        if b.g0 != 0 or b.G != 1:
            raise ValueError(f"{what}: the single-agent network takes a critic-only batch (graph 0 alone, G = 1), "
                             f"got graphs {b.g0}..{b.g0 + b.G - 1}")
        if b.Nv != b.S * self.V:
            raise ValueError(f"{what}: the batch has {b.Nv} variable rows, not {b.S} samples x {self.V} variables")
