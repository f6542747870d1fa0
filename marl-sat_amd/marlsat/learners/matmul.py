"""The launch layer under the GNN actor-critic (gnn.py): which library export runs a matrix product, with which
label, FLOP and byte count.  ``Matmul`` is the base class of ``GNNActorCritic``: grow-only scratch, one launch
helper (FLOP count, bench.py's per-kernel timing record, return-code check), the GEMM / data-gradient /
weight-gradient / column-sum / GRU-forward wrappers over it, and the weight splitters of the bf16x3 and fp16x2
kernels.  It knows nothing of the network's structure; the subclass supplies device, H, p() and the counters.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .. import _lib

L_ = _lib.lib


class _Scratch:
    """Grow-only device scratch (ones vector, wgrad workspace, LN partials, GRU tile flags)."""

    def __init__(self, device):
        self.device = device
        self.ones = torch.ones(1, device=device)
        self.ws = torch.empty(1, device=device)
        self.part = torch.empty(1, device=device)
        self.flags = None

    def get_ones(self, n):
        if self.ones.numel() < n:
            self.ones = torch.ones(max(n, 2 * self.ones.numel()), device=self.device)
        return self.ones

    def get_ws(self, nbytes):
        n = (nbytes + 3) // 4 + 1
        if self.ws.numel() < n:
            self.ws = torch.empty(max(n, 2 * self.ws.numel()), device=self.device)
        return self.ws

    def get_flags(self, n):
        if self.flags is None or self.flags.numel() < n:
            self.flags = torch.empty(max(n, 1024), dtype=torch.int32, device=self.device)
        return self.flags

    def get_part(self, n):
        if self.part.numel() < n:
            self.part = torch.empty(max(n, 2 * self.part.numel()), device=self.device)
        return self.part


class DgradSide(NamedTuple):
    """One C (+)= A @ W^T product of a dual data-gradient launch."""
    A: int  # pointer to the dG rows (a packed buffer's fp32 column address, also when it holds planes)
    lda: int
    h2: torch.Tensor  # W's fp16x2 planes
    x3: torch.Tensor  # W's bf16x3 planes (the kernel's fallback body when the fp16 split overflowed)
    wbad: int  # pointer to the split's overflow flag
    C: int
    ldc: int
    N: int
    acc: int


class WgradSide(NamedTuple):
    """One W[:, (n + rot) % N] (+)= (A^T G)[:, n] product of a dual weight-gradient launch."""
    A: int
    lda: int
    G: int  # pointer into the dG rows, as DgradSide.A
    ldg: int
    W: int
    ldw: int
    K: int
    N: int
    rot: int


class Matmul:
    """Launch wrappers; `_counters` is the class whose `flops` / `ktimer` the launches update (GNNActorCritic)."""

    _counters = None

    def __init__(self, device):
        self.device = device
        self.scr = _Scratch(device)

    @property
    def stream(self):
        return _lib.stream_ptr(self.device)

    @staticmethod
    def _ptr(t: torch.Tensor, col: int = 0) -> int:
        return t.data_ptr() + col * t.element_size()

    def _launch(self, export: str, label: Optional[str], flop, nbytes, *args, counted=None):
        """Call L_.<export>(*args, stream) and check its return code.  `flop` (2*M*N*K per product; `counted`
        where the roofline's count differs from the timed one) goes to the counters' `flops`; under bench.py's
        ktimer a launch with a label records (start, end, algorithmic fp32 FLOPs, algorithmic HBM bytes: operands
        read once + results written, no re-reads or workspaces) under that label."""
        c = self._counters
        c.flops += flop if counted is None else counted
        kt = c.ktimer
        fn = getattr(L_, export)
        if kt is None or label is None:
            rc = fn(*args, self.stream)
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args, self.stream)
            e1.record()
            kt.setdefault(label, []).append((e0, e1, float(flop), float(nbytes)))
        if rc:
            _lib.check(rc, export)

    def _call(self, export: str, *args):
        """A launch outside the roofline (gathers, pools, elementwise kernels, splits): no FLOPs, never timed."""
        self._launch(export, None, 0, 0, *args)

    @staticmethod
    def _span(p0: int, p1: int, width: int, ld: int) -> int:
        """Floats per row read by two row windows [p, p + width) (byte pointers) of one row-major buffer
        with ld floats per row: their union if they overlap within a row, else both."""
        lo, hi = min(p0, p1), max(p0, p1) + 4 * width
        return (hi - lo) // 4 if hi - lo <= 4 * ld else 2 * width

    def _gemm(self, A, lda, B, ldb, transB, C, ldc, bias, M, N, K, acc=0):
        self._launch("msat_gemm", "msat_gemm (fp32 MFMA)", 2 * M * N * K, 4.0 * (M * K + N * K + M * N * (1 + acc)),
                     A, lda, B, ldb, transB, C, ldc, bias, M, N, K, acc)

    def _gemm64(self, A, lda, transA, B, ldb, transB, C, ldc, M, N, K, acc=0):
        """fp64-accumulated small product, one rounding per element (the folded weights, gemm.hip)."""
        self._launch("msat_gemm_f64acc", None, 0, 0, A, lda, transA, B, ldb, transB, C, ldc, M, N, K, acc)

    def _split_rot(self, mats, f16: bool):
        """Row-major planes of each (rows, 3H) weight block, for the backward's C (+)= dG @ W^T products (once
        per backward).  mats: {key: (matrix, column rotation)}; rotation 2H puts the gate blocks in (n, r, z)
        order, the order of the packed backward rows' dGi columns.  bf16x3 planes (gemm_x3.hip), or with f16 the
        fp16x2 planes (2^10 W).  -> ({key: planes tensor}, {key: wbad pointer}); wbad[key] = 1 if the block
        overflowed fp16 (f16 only: one int32 per block, kept alive under "_bad")."""
        bad = torch.empty(len(mats), dtype=torch.int32, device=self.device) if f16 else None
        out, bp = {}, {}
        for i, (key, (Wm, rot)) in enumerate(mats.items()):
            rows, cols = Wm.shape
            buf = torch.empty((2 if f16 else 3) * rows * cols + 8, dtype=torch.int16, device=self.device)
            if f16:
                bp[key] = self._ptr(bad, i)
                self._launch("msat_split_f16x2_rot", None, 0, 0, Wm.data_ptr(), rows, cols, cols, rot, buf.data_ptr(),
                             bp[key])
            else:
                self._launch("msat_split_bf16x3_rot", None, 0, 0, Wm.data_ptr(), rows, cols, cols, rot,
                             buf.data_ptr())
            out[key] = buf
        if f16:
            out["_bad"] = bad  # keep-alive
        return out, bp

    def _split_t(self, mats, f16: bool):
        """{key: (K, 3H) matrix} -> ({key: (W^T planes (3H, Kp) each, Kp)}, flags), Kp = K rounded up to 32: the
        GRU forward's register-A operands, transposed, zero-padded and split in one pass (once per forward).
        bf16x3 planes (flags None), or with f16 the fp16x2 planes (weights scaled by 2^10) and flags = one int32
        per matrix in mats' order, 1 if it overflowed fp16 (device flags read by the GRU launch)."""
        bad = torch.empty(len(mats), dtype=torch.int32, device=self.device) if f16 else None
        out = {}
        for i, (key, Wm) in enumerate(mats.items()):
            K, N = Wm.shape
            Kp = (K + 31) // 32 * 32
            buf = torch.empty((2 if f16 else 3) * N * Kp + 8, dtype=torch.int16, device=self.device)
            if f16:
                self._launch("msat_split_f16x2_t", None, 0, 0, Wm.data_ptr(), K, N, Wm.stride(0), Kp, buf.data_ptr(),
                             self._ptr(bad, i))
            else:
                self._launch("msat_split_bf16x3_t", None, 0, 0, Wm.data_ptr(), K, N, Wm.stride(0), Kp,
                             buf.data_ptr())
            out[key] = (buf, Kp)
        return out, bad

    def _dgrad_dual(self, p0: DgradSide, p1: DgradSide, rexp, M, K, pbase=None):
        """Both C (+)= A @ W^T products over the same M rows (row exponents rexp) in one fp16x2 launch
        (gemm_x3.hip *_dual_kernel).  pbase: the packed buffer's base when it holds fp16x2 planes (A pointers
        are then its fp32 column addresses)."""
        if M == 0:
            return
        fl = 2.0 * M * K * (p0.N + p1.N)
        nb = 4.0 * M * (self._span(p0.A, p1.A, K, p0.lda) + p0.N * (1 + p0.acc) + p1.N * (1 + p1.acc) + 1)
        sides = lambda q0, q1: tuple(v for q in (q0, q1) for v in q._replace(h2=q.h2.data_ptr(), x3=q.x3.data_ptr()))
        if pbase is not None:  # fp32 column c of a packed row -> its hi-plane element c (same bytes per row)
            pa = lambda p: p._replace(A=pbase + (p.A - pbase) // 2, lda=2 * p.lda)
            self._launch("msat_gemm_h2_dual_planes", "gemm_h2r16_kernel (dgrad, fp16x2 planes)", fl, nb,
                         *sides(pa(p0), pa(p1)), p0.lda, rexp.data_ptr(), M, K)
            return
        self._launch("msat_gemm_h2_dual", "gemm_h2r16_kernel (dgrad, fp16x2)", fl, nb, *sides(p0, p1),
                     rexp.data_ptr(), M, K)

    def _wgrad_h2_dual(self, p0: WgradSide, p1: WgradSide, rexp, M, acc=1, pbase=None):
        """Both W[:, (n + rot) % N] (+)= (A^T G)[:, n] products over the same M rows of G's buffer (row exponents
        rexp) in one fp16x2 launch.  pbase: as _dgrad_dual (G's buffer holds fp16x2 planes)."""
        if M == 0:
            return
        fl = 2.0 * M * (p0.K * p0.N + p1.K * p1.N)
        ws = self.scr.get_ws(int(L_.msat_gemm_wgrad_dual_workspace_bytes(M, p0.K, p0.N, p1.K, p1.N)))
        nb = 4.0 * M * (p0.K + p1.K + self._span(p0.G, p1.G, p0.N, p0.ldg) + 1)  # A rows, G rows, rexp
        if pbase is not None:
            pg = lambda p: p._replace(G=pbase + (p.G - pbase) // 2, ldg=2 * p.ldg)
            self._launch("msat_gemm_wgrad_h2_dual_planes", "wgrad_w_dual_pl_kernel + fixup + reduce (fp16x2 planes)",
                         fl, nb, *pg(p0), *pg(p1), p0.ldg, rexp.data_ptr(), M, acc, ws.data_ptr())
            return
        self._launch("msat_gemm_wgrad_h2_dual", "wgrad_w_kernel<2> + fixup + reduce (fp16x2)", fl, nb, *p0, *p1,
                     rexp.data_ptr(), M, acc, ws.data_ptr())

    def _dgrad(self, A, lda, Wm: torch.Tensor, planes, C, ldc, M, N, K, acc, h2=None):
        """C[M,N] (+)= A[M,K] @ Wm[:N]^T (Wm rows = N, row stride K): the fp32-accurate bf16x3 split GEMM on
        `planes` (gemm_x3.hip), the fp32 MFMA GEMM without them.  h2 = (fp16x2 planes, wbad pointer, A's row
        exponents): the fp16x2 kernel (gemm_h2r16_kernel; its bf16x3 body on `planes` if the split overflowed)."""
        if h2 is not None and M > 0:
            p2, wbad, rexp = h2
            self._launch("msat_gemm_h2", "gemm_h2r16_kernel (dgrad, fp16x2)", 2 * M * N * K,
                         4.0 * M * (K + N * (1 + acc) + 1), A, lda, rexp.data_ptr(), p2.data_ptr(), planes.data_ptr(),
                         wbad, C, ldc, None, M, N, K, acc)
        elif planes is None:
            self._gemm(A, lda, Wm.data_ptr(), K, 1, C, ldc, None, M, N, K, acc)
        else:
            self._launch("msat_gemm_x3", "gemm_x3r16_kernel (dgrad, bf16x3)", 2 * M * N * K,
                         4.0 * M * (K + N * (1 + acc)), A, lda, planes.data_ptr(), C, ldc, None, M, N, K, acc)

    def _wgrad(self, A, lda, G, ldg, W, ldw, M, K, N, acc=1, rot=0, rexp=None):
        """W[:, (n + rot) % N] (+)= (A^T G)[:, n] (rot: the packed rows' gate-block rotation).  rexp (G's row scale
        exponents, written by the GRU backward): the fp16x2 whole-row kernel, which scales G per row split
        (gemm_x3.hip wgrad_w_kernel<2>)."""
        if M == 0:
            return
        ws = self.scr.get_ws(int(L_.msat_gemm_wgrad_workspace_bytes(M, K, N)))
        if rexp is not None:
            self._launch("msat_gemm_wgrad_h2", "wgrad_w_kernel<2> + fixup + reduce (fp16x2)", 2 * M * N * K,
                         4.0 * M * (K + N + 1), A, lda, G, ldg, rexp.data_ptr(), W, ldw, M, K, N, rot, acc,
                         ws.data_ptr())
            return
        if K <= 8:
            label = "wgrad_skinny + reduce (K <= 8)"
        elif N <= 384:
            label = "wgrad_w_kernel<3> + reduce (bf16x3)"
        else:
            label = "wgrad_x3_kernel + reduce (bf16x3)"
        self._launch("msat_gemm_wgrad_rot", label, 2 * M * N * K, 4.0 * M * (K + N), A, lda, G, ldg, W, ldw, M, K, N,
                     rot, acc, ws.data_ptr())

    def _colsum(self, G, ldg, M, N, out, acc=1):
        if M == 0:
            return
        ws = self.scr.get_part(int(L_.msat_colsum_workspace_floats(M, N)))
        self._launch("msat_colsum", None, 0, 0, G, ldg, M, N, out, acc, ws.data_ptr())

    def _gru(self, cell: str, segs, hprev: torch.Tensor, ln_row: torch.Tensor, out: torch.Tensor,
             g4: Optional[torch.Tensor], R: int, wi: Optional[torch.Tensor] = None, wt=None):
        """One fused GRU cell + LayerNorm (msat_gru_ln_fused_fwd): segs = [(ptr, ld, width)] of x;
        wi overrides the cell's input matrix (the phi-folded matrices of the fused encoder);
        wt = {"wi": (W^T planes, kxp), "wh": planes[, "h2": fp16x2 planes]} selects the register-A
        bf16x3 kernel (msat_gru_ln_fused_fwd_x3r) or, with "h2", the fp16x2 one + its bf16x3 fixup
        (gru_fused.hip kRH2: three fp16 MFMAs per product instead of six bf16 ones, two weight planes instead of
        three; tiles whose activations leave fp16's range are recomputed in bf16x3 by the same launch pair)."""
        H = self.H
        segs = list(segs) + [(0, 0, 0)] * (3 - len(segs))
        kx = sum(w for _, _, w in segs)
        x = [v for seg in segs for v in seg] + [hprev.data_ptr(), H]
        bi, bh = self.p(f"enc.{cell}_bi").data_ptr(), self.p(f"enc.{cell}_bh").data_ptr()
        tail = (self._ptr(ln_row), self._ptr(ln_row, H), out.data_ptr(), H, g4.data_ptr() if g4 is not None else 0,
                4 * H, R, H)
        # the roofline counts kx rounded up to the MFMA's 16, the timed record the algorithmic kx
        counted, fl = 2 * R * 3 * H * (H + (kx + 15) // 16 * 16), 2.0 * R * 3 * H * (H + kx)
        nb = 4.0 * R * (kx + 2 * H + (4 * H if g4 is not None else 0))  # x, h in; h' (+ tape) out
        if isinstance(wt, dict) and wt.get("h2"):  # fp16x2 register-A kernel + bf16x3 fixup of flagged tiles
            h2wi, h2wh, wbad = wt["h2"]
            flags = self.scr.get_flags((R + 127) // 128)
            self._launch("msat_gru_ln_fused_fwd_h2r", "gru_ln_fused_fwd_h2s_kernel (fp16x2, + x3r fixup launch)", fl,
                         nb, *x, h2wi.data_ptr(), h2wh.data_ptr(), wt["wi"][0].data_ptr(), wt["wh"].data_ptr(),
                         wt["wi"][1], bi, bh, *tail, flags.data_ptr(), wbad, counted=counted)
        elif isinstance(wt, dict):  # register-A bf16x3 kernel: W^T planes {"wi": (planes, kxp), "wh": planes}
            self._launch("msat_gru_ln_fused_fwd_x3r", "gru_ln_fused_fwd_x3r_kernel (bf16x3)", fl, nb, *x,
                         wt["wi"][0].data_ptr(), wt["wi"][1], bi, wt["wh"].data_ptr(), bh, *tail, counted=counted)
        else:  # the plain fp32 kernel is not in the roofline table
            self._launch("msat_gru_ln_fused_fwd", None, fl, nb, *x,
                         (self.p(f"enc.{cell}_wi") if wi is None else wi).data_ptr(), bi,
                         self.p(f"enc.{cell}_wh").data_ptr(), bh, *tail, counted=counted)
