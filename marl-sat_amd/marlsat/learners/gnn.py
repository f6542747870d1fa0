"""GNN actor-critic on the device: forward, backward and Adam over the HIP kernels.

Mirrors ``GNN_ActorCritic`` (src/learners/mappo_gnn_sat_learner.py:198-355) and
``GNNEncoder`` (:19-82) on a ragged graph batch (graphs.py).  Every matmul is the
fp32 MFMA GEMM of gemm.hip, the message passing is the signed literal gathers,
GRU + LayerNorm and the heads are fused kernels; torch only allocates memory.

Per message step l the forward keeps, for the backward pass, the step inputs
(Hp, Hn, Hc), the gathered clause input, the var-side messages and the six GRU
gate pre-activations; the backward walks the steps in reverse, accumulating
every weight gradient through the split-M weight-gradient GEMM (fixed reduction
order: the whole update is bitwise reproducible).

This file is the network: encoder, heads, forward, backward, Adam.  Which export runs each matrix product,
its operands, labels and FLOP / byte accounting are the launch layer, matmul.py (``Matmul``, the base class).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from . import params as P
from .graphs import GraphBatch
from .matmul import DgradSide, Matmul, WgradSide

L_ = _lib.lib

# Arithmetic of the matrix work (README "Kernel-path switches"): "fp16x2" (default) runs the GRU
# forward and the backward's data / weight gradients on fp16 MFMAs with a two-way fp32 split, falling
# back per tile to "bf16x3" (three-way bf16 split) where fp16's range fails; "bf16x3" runs that
# fallback throughout; "fp32" keeps every product on fp32 MFMA (the accuracy reference path).
PRECISION = os.environ.get("MARLSAT_PRECISION", "fp16x2")
PRECISION_CODES = {"fp16x2": 0, "bf16x3": 1, "fp32": 2}  # MSAT_PRECISION_* (include/marlsat_net.h)
if PRECISION not in PRECISION_CODES:
    raise ValueError(f"MARLSAT_PRECISION must be fp16x2, bf16x3 or fp32, got {PRECISION!r}")
# the library's weight-gradient path follows the same validated value (set once, not re-read per call)
_lib.check(L_.msat_set_precision(PRECISION_CODES[PRECISION]), "msat_set_precision")


@dataclass
class StepTape:
    Hp: torch.Tensor
    Hn: torch.Tensor
    Hc: torch.Tensor
    GIN: torch.Tensor  # (Nc, 2H) clause GRU input: gathered [sum H_v+ | sum H_v-] (fused) or messages (ref)
    G4c: torch.Tensor  # (Nc, 4H) clause GRU pre-activations [r | z | gin | ghn]
    NV: torch.Tensor  # (Nv, 2H) var GRU inputs: gathered [sum H_c over + | over -] (fused) or messages (ref)
    G4p: torch.Tensor  # (Nv, 4H) update_v_pos pre-activations
    G4n: torch.Tensor  # (Nv, 4H) update_v_neg pre-activations


@dataclass
class HeadTape:
    pooled: Optional[torch.Tensor] = None
    c0: Optional[torch.Tensor] = None
    c1: Optional[torch.Tensor] = None
    my: Optional[torch.Tensor] = None
    ctx: Optional[torch.Tensor] = None
    h1: Optional[torch.Tensor] = None
    n1: Optional[torch.Tensor] = None
    h2: Optional[torch.Tensor] = None  # mode 1 second hidden layer


def _a(t) -> int:
    """Device address of a tensor, or the byte pointer itself."""
    return t if isinstance(t, int) else t.data_ptr()


class _BackwardPlan(NamedTuple):
    """How one backward of the fused encoder runs: the kernel-path switches, resolved once per encode_backward."""
    packed: bool  # backward rows [dan | dar | daz | dan r] (4H): dGh = cols H..4H, dGi = cols 0..3H in gate
    #               order (n, r, z); needs the x3 path (its F planes are split with the gate blocks rotated)
    rot: int  # column rotation of the F blocks' planes and of dF's weight gradient (2H when packed)
    flags: int  # msat_gru_ln_bwd_g4f(e) flags
    h2: bool  # fp16x2 weight gradients
    dh2: bool  # fp16x2 data gradients
    need_rexp: bool  # the GRU backward writes each row's scale exponent (either fp16x2 product reads it)
    dual: bool  # a cell's two data gradients in one launch, its two weight gradients in another
    planes: bool  # the packed rows as fp16x2 planes (read only by the dual products)
    pl: dict  # {weight block: bf16x3 planes, or None off the x3 path}
    pl2: Optional[dict]  # {weight block: fp16x2 planes} (dh2)
    wbad: Optional[dict]  # {weight block: pointer to its fp16 overflow flag} (dh2)


class _Cell(NamedTuple):
    """One GRU cell's backward at one message step (_cell_backward, _cell_backward_ref)."""
    name: str  # "gru_vp" | "gru_vn" | "gru_c"
    Hx: torch.Tensor  # previous state (R, H)
    G4: torch.Tensor  # the forward's gate pre-activations (R, 4H)
    dH: torch.Tensor  # incoming gradient of the cell's output
    k: int  # LayerNorm row
    X: int  # the input operand's gathered / message columns: pointer, ld, width
    ldx: int
    kx: int
    dX: int  # where d(those columns) is written: pointer, ld
    lddx: int
    feat: int = 0  # the input's feature columns (x, svf, counts): pointer, ld, count
    ldf: int = 0
    nfeat: int = 0
    fk: Optional[str] = None  # fused: the folded matrix' key in the plan, its view and its gradient's
    F: Optional[torch.Tensor] = None
    gF: Optional[torch.Tensor] = None


class GNNActorCritic(Matmul):
    """Device GNN_ActorCritic with flat parameters (params.py layout)."""

    def __init__(self, gnn_hidden_dim: int, gnn_num_message_passing_steps: int, num_agents: int,
                 max_vars_per_agent: int, action_mode: int, num_vars: int, agent_id_embed_dim: int = 16,
                 device=None, seed: int = 0):
        self.H, self.L = gnn_hidden_dim, gnn_num_message_passing_steps
        self.A, self.M, self.mode, self.E = num_agents, max_vars_per_agent, action_mode, agent_id_embed_dim
        self.V = num_vars
        self.base, self.rem = divmod(num_vars, num_agents)
        self.CW = 5 * self.H + self.E
        super().__init__(torch.device(device) if device is not None else
                         torch.device("cuda", torch.cuda.current_device()))
        self.spec = self._spec()
        self.layout = self.spec.layout
        self.tab, self.size = P.offsets(self.layout)
        self.params = torch.from_numpy(self.spec.init_flat(seed)).to(self.device)
        self.grads = torch.zeros_like(self.params)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.adam_count = 0

    # ----------------------------------------------------------- plumbing ----
    def _spec(self) -> P.Spec:
        """The parameter tree (params.Spec); a network with another layout replaces it (single_gnn.py)."""
        return P.spec(self.H, self.L, self.A, self.M, self.mode, self.E)

    def load_flax(self, tree):
        self.params.copy_(torch.from_numpy(self.spec.from_flax(tree)))

    def to_flax(self, grads: bool = False):
        return self.spec.to_flax((self.grads if grads else self.params).detach().cpu().numpy())

    def p(self, name: str) -> torch.Tensor:
        o, shp = self.tab[name]
        return self.params[o: o + int(np.prod(shp))].view(shp)

    def g(self, name: str) -> torch.Tensor:
        o, shp = self.tab[name]
        return self.grads[o: o + int(np.prod(shp))].view(shp)

    def _e(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    flops = 0  # matmul FLOPs issued (2*M*N*K per GEMM), for the MFMA roofline

    # bench.py's per-kernel roofline: a dict makes the MFMA kernels' launches record
    # {label: [(start event, end event, fp32-equivalent algorithmic FLOPs)]} on the launch stream
    ktimer: Optional[dict] = None

    # fp32-accurate bf16x3 split GEMM for the backward's C (+)= dG @ W^T products (gemm_x3.hip)
    use_x3 = PRECISION != "fp32"

    # fp16x2 data gradients of the packed backward rows (gemm_x3.hip gemm_h2r16_kernel)
    use_dgrad_h2 = PRECISION == "fp16x2"

    # a cell's two data gradients / two weight gradients in one launch each (gemm_x3.hip *_dual_kernel;
    # the fp16x2 path always takes them: -4 % against separate launches, round 2)
    use_dual = True

    # the packed backward rows as fp16x2 planes (gnn_kernels.hip flags bit 3): split once per row in the GRU
    # backward instead of once per consumer and k tile; the dual products read the planes (round 5)
    use_planes = os.environ.get("MARLSAT_PLANES", "1") != "0"

    # fp16x2 whole-row weight gradients of the GRU backward's packed rows (gemm_x3.hip wgrad_w_kernel<2>):
    # the backward writes each row's scale exponent, the kernel scales G per row split
    use_wgrad_h2 = PRECISION == "fp16x2"

    # split GRU kernels (fp32-accurate, 16x16x32 MFMAs, register-A) for the fused encoder at H = 128:
    # bf16x3 (gru_fused.hip x3r), and the fp16x2 kernel below with x3r as its fixup; else fp32 MFMA
    use_gru_x3 = PRECISION != "fp32"

    # fp16x2 operands for the register-A GRU forward (gru_fused.hip kRH2: three fp16 MFMAs per product
    # instead of six bf16 ones, two weight planes instead of three; tiles whose activations leave fp16's
    # range are recomputed in bf16x3 by the same launch pair); MARLSAT_GRU_H2=0 keeps bf16x3 throughout
    use_gru_h2 = PRECISION == "fp16x2"

    # ------------------------------------------------------- dense layers ----
    def _linear(self, x, ldx, w: str, b: Optional[str], out, ldo, M, N, K, row0=0):
        """out[M, N] = x[M, K] @ W[row0:row0 + K] (+ b): parameters by name, x / out tensors or byte pointers."""
        self._gemm(_a(x), ldx, self.p(w).data_ptr() + 4 * row0 * N, N, 0, _a(out), ldo,
                   self.p(b).data_ptr() if b else None, M, N, K)

    def _linear_backward(self, x, ldx, w: str, b: Optional[str], dy, ldy, M, N, K, dx=None, lddx=0, acc=0, row0=0):
        """Of y = x @ W[row0:row0 + K] + b, in this order: dx (+)= dy W^T (if dx; acc: accumulate),
        g(W) += x^T dy, g(b) += column sums of dy (if b)."""
        if dx is not None:
            self._gemm(_a(dy), ldy, self.p(w).data_ptr() + 4 * row0 * N, N, 1, _a(dx), lddx, None, M, K, N, acc)
        self._wgrad(_a(x), ldx, _a(dy), ldy, self.g(w).data_ptr() + 4 * row0 * N, N, M, K, N)
        if b:
            self._colsum(_a(dy), ldy, M, N, self.g(b).data_ptr())

    # ---------------------------------------------------------- encoder ----
    def encode(self, b: GraphBatch, save: bool):
        return self._encode_fused(b, save) if self.fuse_phi else self._encode_ref(b, save)

    def encode_backward(self, b: GraphBatch, tape: List[StepTape], Hc_final, dHp, dHn, dHc):
        if self.fuse_phi:
            self._encode_backward_fused(b, tape, Hc_final, dHp, dHn, dHc)
        else:
            self._encode_backward_ref(b, tape, Hc_final, dHp, dHn, dHc)

    def _embed(self, b: GraphBatch):
        """literal / clause embeddings (learner:57-59): vfeat[:, 1:4] = svf, cfeat = clause features."""
        H = self.H
        Hp, Hn, Hc = self._e(b.Nv, H), self._e(b.Nv, H), self._e(b.Nc, H)
        self._linear(self._ptr(b.vfeat, 1), 8, "enc.lpe_w", "enc.lpe_b", Hp, H, b.Nv, H, 3)
        self._linear(self._ptr(b.vfeat, 1), 8, "enc.lne_w", "enc.lne_b", Hn, H, b.Nv, H, 3)
        self._linear(b.cfeat, 3, "enc.ce_w", "enc.ce_b", Hc, H, b.Nc, H, 3)
        return Hp, Hn, Hc

    def _embed_backward(self, b: GraphBatch, dHp, dHn, dHc):
        H = self.H
        self._linear_backward(self._ptr(b.vfeat, 1), 8, "enc.lpe_w", "enc.lpe_b", dHp, H, b.Nv, H, 3)
        self._linear_backward(self._ptr(b.vfeat, 1), 8, "enc.lne_w", "enc.lne_b", dHn, H, b.Nv, H, 3)
        self._linear_backward(b.cfeat, 3, "enc.ce_w", "enc.ce_b", dHc, H, b.Nc, H, 3)

    # Fused encoder ("gather first, phi folded into the GRU input matrix").  Per message step
    # the reference computes m_c+ = A+^T (H_v+ Wcp + bcp) and feeds [m_c+ | m_c-] through
    # update_c's input matrix Wi_c (learner:66-69); by linearity
    #     [m_c+ | m_c-] Wi_c = [A+^T H_v+ | A-^T H_v-] [[Wcp Wi_c+], [Wcn Wi_c-]] + n+ (bcp Wi_c+) + n- (bcn Wi_c-)
    # with n+/- the clause row's positive / negative slot counts, and likewise on the var side
    # n_v+ Wi_vp,n = (A+ H_c)(Wv+ Wi_vp,n) + deg+ (bv+ Wi_vp,n)  (learner:72-79).  So each step
    # is two gathers of the node STATES plus the three fused GRU kernels, with the folded
    # matrices F (rows: [products | count-column rows]) rebuilt once per forward; the phi GEMMs
    # (forward, input-gradient and weight-gradient) disappear and the weight gradients of
    # phi / Wi are recovered from dF once per backward (_unfuse_grads).  Same function,
    # different fp32 association: parity is the 1e-5 fp32 bar, not bitwise.
    # the fp32 path is the reference's operation order: phi stays unfolded there unless MARLSAT_FUSE_PHI says so
    fuse_phi = os.environ.get("MARLSAT_FUSE_PHI", "0" if PRECISION == "fp32" else "1") != "0"

    def _fold_views(self):
        """Views of the folded matrices F_c (2H+4 rows), F_v+, F_v- (H+8 rows) and of their gradients
        (each block 16-row aligned in one buffer, zero rows between)."""
        H = self.H
        c, v = 2 * H + 4, H + 8
        cp, vp = (c + 15) // 16 * 16, (v + 15) // 16 * 16
        if getattr(self, "_F", None) is None:
            self._F = torch.zeros((cp + 2 * vp, 3 * H), dtype=torch.float32, device=self.device)
            self._gF = torch.zeros_like(self._F)
        sl = lambda T: (T[:c], T[cp:cp + v], T[cp + vp:cp + vp + v])
        return sl(self._F), sl(self._gF)

    def _fold_weights(self):
        """F_c (2H+4, 3H) = [Wcp Wi_c[:H]; Wcn Wi_c[H:]; bcp Wi_c[:H]; bcn Wi_c[H:]; 0; 0]
        F_v+ (H+8, 3H) = [Wv+ Wi_vp[:H]; Wi_vp[H:H+4]; bv+ Wi_vp[:H]; 0; 0; 0]
        F_v- (H+8, 3H) = [Wv- Wi_vn[:H]; Wi_vn[H:H+4]; 0; bv- Wi_vn[:H]; 0; 0]  (pad rows stay 0)."""
        H, pp = self.H, self._ptr
        (Fc, Fp, Fn), _ = self._fold_views()
        W3 = 3 * H
        wic = self.p("enc.gru_c_wi")
        # F multiplies every row of every step: computed in fp64 and rounded once (a plain fp32 product's
        # rounding is a systematic weight error that 16 GRU + LayerNorm steps accumulate coherently)
        for half, nm in ((0, "phi_cp"), (1, "phi_cn")):
            B = pp(wic[half * H])
            self._gemm64(self.p(f"enc.{nm}_w").data_ptr(), H, 0, B, W3, 0, pp(Fc[half * H]), W3, H, W3, H)
            self._gemm64(self.p(f"enc.{nm}_b").data_ptr(), H, 0, B, W3, 0, pp(Fc[2 * H + half]), W3, 1, W3, H)
        wv, bv = self.p("enc.phi_v_w"), self.p("enc.phi_v_b")
        for half, cell, F in ((0, "gru_vp", Fp), (1, "gru_vn", Fn)):
            wi = self.p(f"enc.{cell}_wi")
            self._gemm64(pp(wv, half * H), 2 * H, 0, wi.data_ptr(), W3, 0, F.data_ptr(), W3, H, W3, H)
            F[H:H + 4].copy_(wi[H:H + 4])
            self._gemm64(pp(bv, half * H), H, 0, wi.data_ptr(), W3, 0, pp(F[H + 4 + half]), W3, 1, W3, H)

    def _unfuse_grads(self):
        """dF -> phi / Wi gradients (F = W Wi: dW = dF Wi^T, dWi = W^T dF; bias rows likewise)."""
        H, pp = self.H, self._ptr
        _, (gFc, gFp, gFn) = self._fold_views()
        W3 = 3 * H
        wic, gwic = self.p("enc.gru_c_wi"), self.g("enc.gru_c_wi")
        for half, nm in ((0, "phi_cp"), (1, "phi_cn")):
            B, gB = pp(wic[half * H]), pp(gwic[half * H])
            self._gemm64(pp(gFc[half * H]), W3, 0, B, W3, 1, self.g(f"enc.{nm}_w").data_ptr(), H, H, H, W3, 1)
            self._gemm64(pp(gFc[2 * H + half]), W3, 0, B, W3, 1, self.g(f"enc.{nm}_b").data_ptr(), H, 1, H, W3, 1)
            self._gemm64(self.p(f"enc.{nm}_w").data_ptr(), H, 1, pp(gFc[half * H]), W3, 0, gB, W3, H, W3, H, 1)
            self._gemm64(self.p(f"enc.{nm}_b").data_ptr(), H, 1, pp(gFc[2 * H + half]), W3, 0, gB, W3, H, W3, 1, 1)
        wv, bv = self.p("enc.phi_v_w"), self.p("enc.phi_v_b")
        gwv, gbv = self.g("enc.phi_v_w"), self.g("enc.phi_v_b")
        for half, cell, gF in ((0, "gru_vp", gFp), (1, "gru_vn", gFn)):
            wi, gwi = self.p(f"enc.{cell}_wi"), self.g(f"enc.{cell}_wi")
            self._gemm64(gF.data_ptr(), W3, 0, wi.data_ptr(), W3, 1, pp(gwv, half * H), 2 * H, H, H, W3, 1)
            self._gemm64(pp(gF[H + 4 + half]), W3, 0, wi.data_ptr(), W3, 1, pp(gbv, half * H), H, 1, H, W3, 1)
            self._gemm64(pp(wv, half * H), 2 * H, 1, gF.data_ptr(), W3, 0, gwi.data_ptr(), W3, H, W3, H, 1)
            self._gemm64(pp(bv, half * H), H, 1, pp(gF[H + 4 + half]), W3, 0, gwi.data_ptr(), W3, H, W3, 1, 1)
            self._colsum(pp(gF[H]), 4 * W3, 1, 4 * W3, pp(gwi[H]))  # the x / svf rows map 1:1

    def _encode_fused(self, b: GraphBatch, save: bool):
        H, e, pp = self.H, self._e, self._ptr
        Nv, Nc = b.Nv, b.Nc
        self._fold_weights()
        (Fc, Fp, Fn), _ = self._fold_views()
        cells = {"gru_c": Fc, "gru_vp": Fp, "gru_vn": Fn}
        wt = dict.fromkeys(cells)
        if self.use_gru_x3 and H == 128:
            pl, _ = self._split_t({**cells, **{"h" + c: self.p(f"enc.{c}_wh") for c in cells}}, f16=False)
            wt = {c: {"wi": pl[c], "wh": pl["h" + c][0]} for c in cells}
            if self.use_gru_h2:  # per cell (wi planes, wh planes, pointer to its [wi, wh overflowed] flags)
                pl2, bad = self._split_t({(c, m): W for c, F in cells.items()
                                          for m, W in enumerate((F, self.p(f"enc.{c}_wh")))}, f16=True)
                self._h2bad = bad.view(len(cells), 2)
                for i, c in enumerate(cells):
                    wt[c]["h2"] = (pl2[c, 0][0], pl2[c, 1][0], pp(bad, 2 * i))
        Hp, Hn, Hc = self._embed(b)
        tape: List[StepTape] = []
        ln = self.p("enc.ln")
        for l in range(self.L):
            GIN = e(Nc, 2 * H)  # [A+^T H_v+ | A-^T H_v-]
            self._call("msat_clause_gather2", Hp.data_ptr(), Hn.data_ptr(), H, b.slots.data_ptr(), GIN.data_ptr(),
                       2 * H, Nc, H, 0, 0)
            Hc1 = e(Nc, H)
            G4c = e(Nc, 4 * H) if save else None
            self._gru("gru_c", [(GIN.data_ptr(), 2 * H, 2 * H), (b.cdeg.data_ptr(), 4, 4)], Hc, ln[3 * l], Hc1, G4c,
                      Nc, wi=Fc, wt=wt["gru_c"])
            NV = e(Nv, 2 * H)  # [A+ H_c | A- H_c]
            self._call("msat_var_gather2", Hc1.data_ptr(), Hc1.data_ptr(), H, b.ptr.data_ptr(), b.inc.data_ptr(),
                       NV.data_ptr(), pp(NV, H), 2 * H, Nv, H, 0)
            outs = []
            for half, cell, Hx, k, F in ((0, "gru_vp", Hp, 3 * l + 1, Fp), (1, "gru_vn", Hn, 3 * l + 2, Fn)):
                Hx1 = e(Nv, H)
                G4 = e(Nv, 4 * H) if save else None
                # input [n_v | x | svf | n+ n- 0 0] against F rows [fold | Wi x/svf | count rows]
                self._gru(cell, [(pp(NV, half * H), 2 * H, H), (b.vfeat.data_ptr(), 8, 8)], Hx, ln[k], Hx1, G4, Nv,
                          wi=F, wt=wt[cell])
                outs.append((G4, Hx1))
            if save:
                tape.append(StepTape(Hp, Hn, Hc, GIN, G4c, NV, outs[0][0], outs[1][0]))
            Hp, Hn, Hc = outs[0][1], outs[1][1], Hc1
        return Hp, Hn, Hc, tape

    def _backward_plan(self, Fc, Fp, Fn) -> _BackwardPlan:
        H = self.H
        packed = self.use_x3
        rot = 2 * H if packed else 0
        mats = {"wh_c": (self.p("enc.gru_c_wh"), 0), "wh_vp": (self.p("enc.gru_vp_wh"), 0),
                "wh_vn": (self.p("enc.gru_vn_wh"), 0), "Fc": (Fc[:2 * H], rot), "Fp": (Fp[:H], rot),
                "Fn": (Fn[:H], rot)}
        pl = self._split_rot(mats, f16=False)[0] if self.use_x3 else dict.fromkeys(mats)
        dh2 = packed and self.use_dgrad_h2
        pl2, wbad = self._split_rot(mats, f16=True) if dh2 else (None, None)
        h2 = packed and self.use_wgrad_h2
        dual = h2 and dh2 and self.use_dual
        planes = dual and self.use_planes
        return _BackwardPlan(packed, rot, 3 | (4 if packed else 0) | (8 if planes else 0), h2, dh2, h2 or dh2, dual,
                             planes, pl, pl2, wbad)

    def _cell_backward(self, pn: _BackwardPlan, c: _Cell, R: int) -> torch.Tensor:
        """GRU + LayerNorm backward of one cell of the fused encoder over its R rows, then its four products:
        dH0 += dGh Wh^T and dX = dGi F^T, g(Wh) += Hx^T dGh and gF += X^T dGi.  -> dH0, the gradient of Hx."""
        H, W3, e, pp = self.H, 3 * self.H, self._e, self._ptr
        ln, dln = self.p("enc.ln"), self.g("enc.ln")
        if pn.packed:
            D = e(R, 4 * H)
            dgi, dgh, ldd = D.data_ptr(), pp(D, H), 4 * H
        else:
            dGI, dGH = e(R, W3), e(R, W3)
            dgi, dgh, ldd = dGI.data_ptr(), dGH.data_ptr(), W3
        dH0 = e(R, H)  # written (not accumulated) by the backward kernel: flags bit 1
        part = self.scr.get_part(int(L_.msat_gru_ln_bwd_partial_floats(R, H)))
        rexp = torch.empty(R, dtype=torch.int32, device=self.device) if pn.need_rexp else None
        # the dF rows under the fold (var cells: x, svf, n+, n-; clause cell: n+, n-) come from the same pass:
        # feature-weighted gate sums
        args = (c.dH.data_ptr(), H, c.G4.data_ptr(), 4 * H, c.Hx.data_ptr(), H, pp(ln[c.k]), dgi, ldd, dgh, ldd,
                dH0.data_ptr(), H, pp(dln[c.k]), pp(dln[c.k], H), self.g(f"enc.{c.name}_bi").data_ptr(),
                pp(self.g(f"enc.{c.name}_bh"), 2 * H), c.feat, c.ldf, c.nfeat, pp(c.gF[c.kx]), part.data_ptr(), R, H,
                pn.flags)
        if pn.need_rexp:
            self._call("msat_gru_ln_bwd_g4fe", *args, rexp.data_ptr())
        else:
            self._call("msat_gru_ln_bwd_g4f", *args)
        whk = "wh_" + c.name[4:]
        gwh = self.g(f"enc.{c.name}_wh").data_ptr()
        if pn.dual:  # dh and d(gathered) in one launch, dWh and dF in another (same packed rows)
            pb = dgi if pn.planes else None
            self._dgrad_dual(
                DgradSide(dgh, ldd, pn.pl2[whk], pn.pl[whk], pn.wbad[whk], dH0.data_ptr(), H, H, 1),
                DgradSide(dgi, ldd, pn.pl2[c.fk], pn.pl[c.fk], pn.wbad[c.fk], c.dX, c.lddx, c.kx, 0), rexp, R, W3,
                pbase=pb)
            self._wgrad_h2_dual(WgradSide(c.Hx.data_ptr(), H, dgh, ldd, gwh, W3, H, W3, 0),
                                WgradSide(c.X, c.ldx, dgi, ldd, c.gF.data_ptr(), W3, c.kx, W3, 2 * H), rexp, R,
                                pbase=pb)
            return dH0
        hx = lambda key: (pn.pl2[key], pn.wbad[key], rexp) if pn.dh2 else None
        wexp = rexp if pn.h2 else None
        self._dgrad(dgh, ldd, self.p(f"enc.{c.name}_wh"), pn.pl[whk], dH0.data_ptr(), H, R, H, W3, 1, hx(whk))
        self._wgrad(c.Hx.data_ptr(), H, dgh, ldd, gwh, W3, R, H, W3, rexp=wexp)
        # input path: d(gathered) and dF rows [fold | x/svf | counts]; in packed rows dGi's gate blocks are (n | r z)
        self._dgrad(dgi, ldd, c.F, pn.pl[c.fk], c.dX, c.lddx, R, c.kx, W3, 0, hx(c.fk))
        self._wgrad(c.X, c.ldx, dgi, ldd, c.gF.data_ptr(), W3, R, c.kx, W3, rot=pn.rot, rexp=wexp)
        return dH0

    def _encode_backward_fused(self, b: GraphBatch, tape: List[StepTape], Hc_final, dHp, dHn, dHc):
        H, e, pp = self.H, self._e, self._ptr
        Nv, Nc = b.Nv, b.Nc
        (Fc, Fp, Fn), (gFc, gFp, gFn) = self._fold_views()
        self._gF.zero_()
        pn = self._backward_plan(Fc, Fp, Fn)
        for l in range(self.L - 1, -1, -1):
            t = tape[l]
            dNV = e(Nv, 2 * H)
            var_cells = (("gru_vp", t.Hp, t.G4p, dHp, "Fp", Fp, gFp), ("gru_vn", t.Hn, t.G4n, dHn, "Fn", Fn, gFn))
            dHp, dHn = [self._cell_backward(pn, _Cell(
                cell, Hx, G4, dHx, 3 * l + 1 + half, pp(t.NV, half * H), 2 * H, H, pp(dNV, half * H), 2 * H,
                b.vfeat.data_ptr(), 8, 6, fk, F, gF), Nv)
                for half, (cell, Hx, G4, dHx, fk, F, gF) in enumerate(var_cells)]
            # var gather backward: dH_c (+)= A+^T dNV+ + A-^T dNV-  (one merged clause gather)
            self._call("msat_clause_gather2", dNV.data_ptr(), pp(dNV, H), 2 * H, b.slots.data_ptr(), dHc.data_ptr(),
                       H, Nc, H, 1, 1)
            dGIN = e(Nc, 2 * H)
            dHc = self._cell_backward(pn, _Cell("gru_c", t.Hc, t.G4c, dHc, 3 * l, t.GIN.data_ptr(), 2 * H, 2 * H,
                                                dGIN.data_ptr(), 2 * H, b.cdeg.data_ptr(), 4, 2, "Fc", Fc, gFc), Nc)
            # clause gather backward: dH_v+/- (+)= A+/- dGIN+/-
            self._call("msat_var_gather2", dGIN.data_ptr(), pp(dGIN, H), 2 * H, b.ptr.data_ptr(), b.inc.data_ptr(),
                       dHp.data_ptr(), dHn.data_ptr(), H, Nv, H, 1)
        self._embed_backward(b, dHp, dHn, dHc)
        self._unfuse_grads()

    def _encode_ref(self, b: GraphBatch, save: bool):
        H, e, pp = self.H, self._e, self._ptr
        Nv, Nc = b.Nv, b.Nc
        Hp, Hn, Hc = self._embed(b)
        tape: List[StepTape] = []
        ln = self.p("enc.ln")
        for l in range(self.L):
            MV = e(Nv, 2 * H)
            self._linear(Hp, H, "enc.phi_cp_w", "enc.phi_cp_b", MV, 2 * H, Nv, H, H)
            self._linear(Hn, H, "enc.phi_cn_w", "enc.phi_cn_b", pp(MV, H), 2 * H, Nv, H, H)
            GIN = e(Nc, 2 * H)
            self._call("msat_clause_gather", MV.data_ptr(), 2 * H, b.slots.data_ptr(), GIN.data_ptr(), 2 * H, Nc, H, 0)
            Hc1 = e(Nc, H)
            G4c = e(Nc, 4 * H) if save else None
            self._gru("gru_c", [(GIN.data_ptr(), 2 * H, 2 * H)], Hc, ln[3 * l], Hc1, G4c, Nc)
            TPN = e(Nc, 2 * H)
            self._linear(Hc1, H, "enc.phi_v_w", "enc.phi_v_b", TPN, 2 * H, Nc, 2 * H, H)
            NV = e(Nv, 2 * H)
            self._call("msat_var_gather", TPN.data_ptr(), 2 * H, b.ptr.data_ptr(), b.inc.data_ptr(), NV.data_ptr(),
                       2 * H, Nv, H, 0)
            outs = []
            for half, cell, Hx, k in ((0, "gru_vp", Hp, 3 * l + 1), (1, "gru_vn", Hn, 3 * l + 2)):
                # input [n_v | x | svf] (learner:75,78)
                Hx1 = e(Nv, H)
                G4 = e(Nv, 4 * H) if save else None
                self._gru(cell, [(pp(NV, half * H), 2 * H, H), (b.vfeat.data_ptr(), 8, 4)], Hx, ln[k], Hx1, G4, Nv)
                outs.append((G4, Hx1))
            if save:
                tape.append(StepTape(Hp, Hn, Hc, GIN, G4c, NV, outs[0][0], outs[1][0]))
            Hp, Hn, Hc = outs[0][1], outs[1][1], Hc1
        return Hp, Hn, Hc, tape

    def _cell_backward_ref(self, c: _Cell, R: int) -> torch.Tensor:
        """GRU + LayerNorm backward of one cell in the reference's operation order (fp32 MFMA products), its
        hidden path and its input path.  -> dH0, the gradient of Hx."""
        H, W3, pp = self.H, 3 * self.H, self._ptr
        ln, dln = self.p("enc.ln"), self.g("enc.ln")
        dGI, dGH = self._e(R, W3), self._e(R, W3)
        dH0 = torch.zeros((R, H), dtype=torch.float32, device=self.device)
        part = self.scr.get_part(int(L_.msat_gru_ln_bwd_partial_floats(R, H)))
        self._call("msat_gru_ln_bwd_g4", c.dH.data_ptr(), H, c.G4.data_ptr(), 4 * H, c.Hx.data_ptr(), H, pp(ln[c.k]),
                   dGI.data_ptr(), W3, dGH.data_ptr(), W3, dH0.data_ptr(), H, pp(dln[c.k]), pp(dln[c.k], H),
                   self.g(f"enc.{c.name}_bi").data_ptr(), pp(self.g(f"enc.{c.name}_bh"), 2 * H), part.data_ptr(), R, H,
                   1)
        # hidden path, then the input path [messages | x | svf]
        self._linear_backward(c.Hx, H, f"enc.{c.name}_wh", None, dGH, W3, R, W3, H, dx=dH0, lddx=H, acc=1)
        self._linear_backward(c.X, c.ldx, f"enc.{c.name}_wi", None, dGI, W3, R, W3, c.kx, dx=c.dX, lddx=c.lddx)
        if c.nfeat:
            self._linear_backward(c.feat, c.ldf, f"enc.{c.name}_wi", None, dGI, W3, R, W3, c.nfeat, row0=c.kx)
        return dH0

    def _encode_backward_ref(self, b: GraphBatch, tape: List[StepTape], Hc_final, dHp, dHn, dHc):
        H, e, pp = self.H, self._e, self._ptr
        Nv, Nc = b.Nv, b.Nc
        for l in range(self.L - 1, -1, -1):
            t = tape[l]
            Hc1 = tape[l + 1].Hc if l + 1 < self.L else Hc_final
            dNV = e(Nv, 2 * H)
            # input [n_v | x | svf] (learner:75,78)
            dHp, dHn = [self._cell_backward_ref(_Cell(cell, Hx, G4, dHx, 3 * l + 1 + half, pp(t.NV, half * H), 2 * H, H,
                                                      pp(dNV, half * H), 2 * H, b.vfeat.data_ptr(), 8, 4), Nv)
                        for half, (cell, Hx, G4, dHx) in enumerate((("gru_vp", t.Hp, t.G4p, dHp),
                                                                    ("gru_vn", t.Hn, t.G4n, dHn)))]
            # var gather backward = clause gather of dNV
            dTPN = e(Nc, 2 * H)
            self._call("msat_clause_gather", dNV.data_ptr(), 2 * H, b.slots.data_ptr(), dTPN.data_ptr(), 2 * H, Nc, H,
                       0)
            self._linear_backward(Hc1, H, "enc.phi_v_w", "enc.phi_v_b", dTPN, 2 * H, Nc, 2 * H, H, dx=dHc, lddx=H,
                                  acc=1)
            dGIN = e(Nc, 2 * H)
            dHc = self._cell_backward_ref(_Cell("gru_c", t.Hc, t.G4c, dHc, 3 * l, t.GIN.data_ptr(), 2 * H, 2 * H,
                                                dGIN.data_ptr(), 2 * H), Nc)
            # clause gather backward = var gather of dGIN
            dMV = e(Nv, 2 * H)
            self._call("msat_var_gather", dGIN.data_ptr(), 2 * H, b.ptr.data_ptr(), b.inc.data_ptr(), dMV.data_ptr(),
                       2 * H, Nv, H, 0)
            for half, nm, Hx, dst in ((0, "phi_cp", t.Hp, dHp), (1, "phi_cn", t.Hn, dHn)):
                self._linear_backward(Hx, H, f"enc.{nm}_w", f"enc.{nm}_b", pp(dMV, half * H), 2 * H, Nv, H, H, dx=dst,
                                      lddx=H, acc=1)
        self._embed_backward(b, dHp, dHn, dHc)

    # ------------------------------------------------------------ heads ----
    def _gr(self, b: GraphBatch):
        return b.vbase.data_ptr(), b.nv.data_ptr(), b.cbase.data_ptr(), b.nc.data_ptr()

    def critic_head(self, b: GraphBatch, Hp, Hn, Hc, ht: HeadTape):
        H, S, e = self.H, b.S, self._e
        pooled, c0, c1, val = e(S, 6 * H), e(S, 128), e(S, 64), e(S)
        self._call("msat_critic_pool", Hp.data_ptr(), Hn.data_ptr(), Hc.data_ptr(), H, *self._gr(b), b.G, S,
                   pooled.data_ptr())
        self._linear(pooled, 6 * H, "crit.d0_w", "crit.d0_b", c0, 128, S, 128, 6 * H)
        self._call("msat_relu", c0.data_ptr(), c0.numel())
        self._linear(c0, 128, "crit.d1_w", "crit.d1_b", c1, 64, S, 64, 128)
        self._call("msat_relu", c1.data_ptr(), c1.numel())
        self._linear(c1, 64, "crit.out_w", "crit.out_b", val, 1, S, 1, 64)
        ht.pooled, ht.c0, ht.c1 = pooled, c0, c1
        return val

    def critic_head_backward(self, b, Hp, Hn, Hc, ht: HeadTape, dval, dHp, dHn, dHc):
        H, S, e = self.H, b.S, self._e
        dc1, dc0, dpooled = e(S, 64), e(S, 128), e(S, 6 * H)
        self._linear_backward(ht.c1, 64, "crit.out_w", "crit.out_b", dval, 1, S, 1, 64, dx=dc1, lddx=64)
        self._call("msat_relu_bwd", dc1.data_ptr(), ht.c1.data_ptr(), dc1.numel())
        self._linear_backward(ht.c0, 128, "crit.d1_w", "crit.d1_b", dc1, 64, S, 64, 128, dx=dc0, lddx=128)
        self._call("msat_relu_bwd", dc0.data_ptr(), ht.c0.data_ptr(), dc0.numel())
        self._linear_backward(ht.pooled, 6 * H, "crit.d0_w", "crit.d0_b", dc0, 128, S, 128, 6 * H, dx=dpooled,
                              lddx=6 * H)
        self._call("msat_critic_pool_bwd", Hp.data_ptr(), Hn.data_ptr(), Hc.data_ptr(), H, *self._gr(b), b.G, S,
                   dpooled.data_ptr(), dHp.data_ptr(), dHn.data_ptr(), dHc.data_ptr())

    def actor_head(self, b: GraphBatch, Hp, Hn, Hc, ht: HeadTape):
        H, S, A, M, CW, e = self.H, b.S, self.A, self.M, self.CW, self._e
        SA = S * A
        R = SA * M
        my, ctx = e(R, 2 * H), e(SA, CW)
        # agent i's graph is slot (1 - g0) + i of its sample: after the critic's in a full batch, else first
        self._call("msat_actor_pool_from", Hp.data_ptr(), Hn.data_ptr(), Hc.data_ptr(), H, *self._gr(b), b.G, 1 - b.g0,
                   S, A, M, self.base, self.rem, self.p("actor.id_emb").data_ptr(), self.E, my.data_ptr(),
                   ctx.data_ptr())
        ht.my, ht.ctx = my, ctx
        Pm, h1 = e(SA, 128), e(R, 128)
        if self.mode == 0:  # first layer [my | ctx] @ flip_d_w: the ctx rows (2H on) once per agent, broadcast
            self._linear(ctx, CW, "actor.flip_d_w", None, Pm, 128, SA, 128, CW, row0=2 * H)
            self._linear(my, 2 * H, "actor.flip_d_w", "actor.flip_d_b", h1, 128, R, 128, 2 * H)
            self._call("msat_bcast_add_relu", h1.data_ptr(), Pm.data_ptr(), SA, M, 128)
            fl, n1, no, logits = e(R), e(SA, 64), e(SA), e(S, A, M + 1)
            self._linear(h1, 128, "actor.flip_o_w", "actor.flip_o_b", fl, 1, R, 1, 128)
            self._linear(ctx, CW, "actor.noop_d_w", "actor.noop_d_b", n1, 64, SA, 64, CW)
            self._call("msat_relu", n1.data_ptr(), n1.numel())
            self._linear(n1, 64, "actor.noop_o_w", "actor.noop_o_b", no, 1, SA, 1, 64)
            self._call("msat_assemble_logits", fl.data_ptr(), no.data_ptr(), SA, A, M, self.base, self.rem,
                       logits.data_ptr())
            ht.h1, ht.n1 = h1, n1
            return logits
        # mode 1: [my | id embedding] @ d0_w, the embedding columns of ctx (5H on) against d0_w's rows 2H on
        self._linear(self._ptr(ctx, 5 * H), CW, "actor.d0_w", None, Pm, 128, SA, 128, self.E, row0=2 * H)
        self._linear(my, 2 * H, "actor.d0_w", "actor.d0_b", h1, 128, R, 128, 2 * H)
        self._call("msat_bcast_add_relu", h1.data_ptr(), Pm.data_ptr(), SA, M, 128)
        h2, logits = e(R, 64), e(S, A, M, 2)
        self._linear(h1, 128, "actor.d1_w", "actor.d1_b", h2, 64, R, 64, 128)
        self._call("msat_relu", h2.data_ptr(), h2.numel())
        self._linear(h2, 64, "actor.out_w", "actor.out_b", logits, 2, R, 2, 64)
        self._call("msat_mask_var_logits", logits.data_ptr(), SA, A, M, self.base, self.rem)
        ht.h1, ht.h2 = h1, h2
        return logits

    def actor_head_backward(self, b, ht: HeadTape, dlogits, dHp, dHn, dHc):
        H, S, A, M, CW, e = self.H, b.S, self.A, self.M, self.CW, self._e
        SA = S * A
        R = SA * M
        dmy, dctx, dh1, dP = e(R, 2 * H), e(SA, CW), e(R, 128), e(SA, 128)
        if self.mode == 0:
            dfl, dno, dn1 = e(R), e(SA), e(SA, 64)
            self._call("msat_split_dlogits", dlogits.data_ptr(), SA, M, dfl.data_ptr(), dno.data_ptr())
            self._linear_backward(ht.h1, 128, "actor.flip_o_w", "actor.flip_o_b", dfl, 1, R, 1, 128, dx=dh1, lddx=128)
            self._call("msat_relu_bwd", dh1.data_ptr(), ht.h1.data_ptr(), dh1.numel())
            self._call("msat_group_sum", dh1.data_ptr(), SA, M, 128, dP.data_ptr())
            self._linear_backward(ht.my, 2 * H, "actor.flip_d_w", "actor.flip_d_b", dh1, 128, R, 128, 2 * H, dx=dmy,
                                  lddx=2 * H)
            self._linear_backward(ht.ctx, CW, "actor.flip_d_w", None, dP, 128, SA, 128, CW, dx=dctx, lddx=CW,
                                  row0=2 * H)
            self._linear_backward(ht.n1, 64, "actor.noop_o_w", "actor.noop_o_b", dno, 1, SA, 1, 64, dx=dn1, lddx=64)
            self._call("msat_relu_bwd", dn1.data_ptr(), ht.n1.data_ptr(), dn1.numel())
            self._linear_backward(ht.ctx, CW, "actor.noop_d_w", "actor.noop_d_b", dn1, 64, SA, 64, CW, dx=dctx,
                                  lddx=CW, acc=1)  # on top of the flip head's dctx
        else:
            dh2 = e(R, 64)
            self._linear_backward(ht.h2, 64, "actor.out_w", "actor.out_b", dlogits, 2, R, 2, 64, dx=dh2, lddx=64)
            self._call("msat_relu_bwd", dh2.data_ptr(), ht.h2.data_ptr(), dh2.numel())
            self._linear_backward(ht.h1, 128, "actor.d1_w", "actor.d1_b", dh2, 64, R, 64, 128, dx=dh1, lddx=128)
            self._call("msat_relu_bwd", dh1.data_ptr(), ht.h1.data_ptr(), dh1.numel())
            self._call("msat_group_sum", dh1.data_ptr(), SA, M, 128, dP.data_ptr())
            self._linear_backward(ht.my, 2 * H, "actor.d0_w", "actor.d0_b", dh1, 128, R, 128, 2 * H, dx=dmy,
                                  lddx=2 * H)
            dctx.zero_()  # only the embedding columns get a gradient here
            self._linear_backward(self._ptr(ht.ctx, 5 * H), CW, "actor.d0_w", None, dP, 128, SA, 128, self.E,
                                  dx=self._ptr(dctx, 5 * H), lddx=CW, row0=2 * H)
        did = e(SA, self.E)
        self._call("msat_actor_pool_bwd_from", H, *self._gr(b), b.G, 1 - b.g0, S, A, M, self.base, self.rem, self.E,
                   dmy.data_ptr(), dctx.data_ptr(), dHp.data_ptr(), dHn.data_ptr(), dHc.data_ptr(), did.data_ptr())
        self._colsum(did.data_ptr(), A * self.E, S, A * self.E, self.g("actor.id_emb").data_ptr())

    # ---------------------------------------------------------- top level ----
    def _check_heads(self, b: GraphBatch, actor: bool, critic: bool, what: str):
        """The heads a batch can feed: the critic pool reads slot 0 of each sample as graph 0 and the actor pool
        A slots from graph 1 on, so a head on a batch without its graphs would silently pool the wrong rows."""
        if critic and b.g0 != 0:
            raise ValueError(f"{what}: the batch is actor-only (graphs {b.g0}..{b.g0 + b.G - 1}): no critic graph")
        if actor and b.g0 + b.G != self.A + 1:
            raise ValueError(f"{what}: the batch holds graphs {b.g0}..{b.g0 + b.G - 1} of 0..{self.A}, not the "
                             f"agents' (critic-only batch?)")

    def forward(self, b: GraphBatch, actor: bool = True, critic: bool = True, save: bool = False):
        self._check_heads(b, actor, critic, "forward")
        Hp, Hn, Hc, tape = self.encode(b, save)
        ht = HeadTape()
        logits = self.actor_head(b, Hp, Hn, Hc, ht) if actor else None
        value = self.critic_head(b, Hp, Hn, Hc, ht) if critic else None
        state = (Hp, Hn, Hc, tape, ht) if save else None
        return logits, value, state

    def backward(self, b: GraphBatch, state, dlogits: Optional[torch.Tensor], dvalue: Optional[torch.Tensor]):
        """Accumulate parameter gradients (self.grads += ...) for upstream grads of logits / value."""
        self._check_heads(b, dlogits is not None, dvalue is not None, "backward")
        Hp, Hn, Hc, tape, ht = state
        dHp = torch.zeros_like(Hp)
        dHn = torch.zeros_like(Hn)
        dHc = torch.zeros_like(Hc)
        if dvalue is not None:
            self.critic_head_backward(b, Hp, Hn, Hc, ht, dvalue, dHp, dHn, dHc)
        if dlogits is not None:
            self.actor_head_backward(b, ht, dlogits, dHp, dHn, dHc)
        self.encode_backward(b, tape, Hc, dHp, dHn, dHc)

    def adam_step(self, lr: float, grad_scale: float = 1.0, b1=0.9, b2=0.999, eps=1e-8,
                  first_bad: Optional[torch.Tensor] = None):
        """One optax.adam step.  first_bad (device int32 scalar, INT32_MAX when clean): set to the smallest
        Adam count whose update left a parameter non-finite (msat_adam_checked; no host sync)."""
        self.adam_count += 1
        self._call("msat_adam_checked", self.params.data_ptr(), self.grads.data_ptr(), self.adam_m.data_ptr(),
                   self.adam_v.data_ptr(), self.size, float(lr), b1, b2, eps, self.adam_count, float(grad_scale),
                   first_bad.data_ptr() if first_bad is not None else None)


GNNActorCritic._counters = GNNActorCritic  # the launch layer counts into this class's flops / ktimer


def path_switches(precision: str) -> dict:
    """GNNActorCritic's kernel-path switches for one MARLSAT_PRECISION value (README "Kernel-path switches"):
    'fp16x2' = phi folded, fp16x2 GRU forward and data / weight gradients (bf16x3 fixups); 'bf16x3' = phi
    folded, the bf16x3 kernels throughout; 'fp32' = fp32 MFMA kernels in the reference's operation order
    (phi not folded)."""
    if precision not in PRECISION_CODES:
        raise ValueError(f"precision must be one of {sorted(PRECISION_CODES)}, got {precision!r}")
    split, h2 = precision != "fp32", precision == "fp16x2"
    return {"fuse_phi": split, "use_x3": split, "use_gru_x3": split, "use_gru_h2": h2, "use_dgrad_h2": h2,
            "use_wgrad_h2": h2}


def set_precision(precision: str) -> dict:
    """Switch the process's matrix arithmetic (the class switches above and the library's weight-gradient path,
    msat_set_precision) to one precision path; returns the previous switches (restore_precision undoes it)."""
    prev = {k: getattr(GNNActorCritic, k) for k in path_switches(precision)}
    prev["_code"] = int(L_.msat_get_precision())
    for k, v in path_switches(precision).items():
        setattr(GNNActorCritic, k, v)
    _lib.check(L_.msat_set_precision(PRECISION_CODES[precision]), "msat_set_precision")
    return prev


def restore_precision(prev: dict) -> None:
    for k, v in prev.items():
        if k != "_code":
            setattr(GNNActorCritic, k, v)
    _lib.check(L_.msat_set_precision(prev["_code"]), "msat_set_precision")
