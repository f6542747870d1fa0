"""GPU: the transposed weight splitters of the register-A GRU kernels on their own.

msat_split_bf16x3_t: planes[q][n][k] bitwise the torch restatement p = bf16(x), m = bf16(x - p), l = bf16(x - p - m)
(round to nearest even) of W[k][n], exact zeros for K <= k < Kp.  msat_split_f16x2_t: the same with x 2^10 and
two fp16 parts, and *bad = 1 exactly when a scaled weight inside the (K, N) operand is not in (-2^15, 2^15).
W sits inside NaN guard rows and ld gaps; a canary tail follows the planes."""
import pytest
import torch

from gemm_placement import CANARY, Placement, operand

pytestmark = pytest.mark.gpu

# (K, N, ldw, Kp); the last is past one grid pass of 4096 x 256 elements (N Kp = 1,056,768)
SHAPES = [(1, 4, 4, 32), (136, 384, 384, 160), (260, 384, 400, 288), (4, 768, 772, 1376)]
LAST = 12345.678  # the large shape's final element: the second grid pass must reach it
SPECIAL = [0.0, -0.0, 1e-40, -1e-45, 1e-30, -1e-30, 1e30, -1e30, float.fromhex("0x1.fffffep+3"),
           float.fromhex("-0x1.000002p-1"), float.fromhex("0x1.abcdeep-7")]


def _weights(K, N, special=True):
    g = torch.Generator(device="cuda").manual_seed(K * 1000 + N)
    W = torch.randn(K, N, device="cuda", generator=g)
    if special:
        flat = W.view(-1)
        idx = torch.arange(len(SPECIAL), device="cuda") * 7 % flat.numel()
        flat[idx[:min(len(SPECIAL), flat.numel())]] = torch.tensor(SPECIAL, device="cuda")[:flat.numel()]
        W[K - 1, N - 1] = LAST
    return W


def _planes(nparts, N, Kp, tail=4096):
    n = nparts * N * Kp
    buf = torch.full((n + tail,), CANARY & 0x7FFF, dtype=torch.int16, device="cuda")
    snap = buf[n:].clone()

    def check():
        assert torch.equal(buf[n:], snap), "wrote past the planes"

    return buf, buf[:n].view(nparts, N, Kp), check


def _padded_t(W, Kp):
    """(N, Kp) float32 on the CPU (IEEE subnormals, no flush): W^T with exact zeros for k >= K."""
    K, N = W.shape
    X = torch.zeros(N, Kp)
    X[:, :K] = W.cpu().t()
    return X


@pytest.mark.parametrize("K,N,ldw,Kp", SHAPES)
def test_split_bf16x3_t_planes(K, N, ldw, Kp):
    from marlsat import _lib

    W = _weights(K, N)
    w = operand(W, Placement(0, ldw - N))
    buf, planes, check = _planes(3, N, Kp)
    _lib.check(_lib.lib.msat_split_bf16x3_t(w.ptr, K, N, ldw, Kp, buf.data_ptr(), _lib.stream_ptr()), "split_bf16x3_t")
    torch.cuda.synchronize()
    w.check()
    check()
    X = _padded_t(W, Kp)
    p = X.bfloat16()
    m = (X - p.float()).bfloat16()
    lo = (X - p.float() - m.float()).bfloat16()
    for q, ref in enumerate((p, m, lo)):
        assert torch.equal(planes[q].cpu(), ref.view(torch.int16)), f"plane {q}"
    assert not bool(planes[:, :, K:].any()), "padding k must be exact (+0) zeros"
    assert float(planes[0, N - 1, K - 1].cpu().view(torch.bfloat16)) == float(torch.tensor(LAST).bfloat16())


@pytest.mark.parametrize("K,N,ldw,Kp", SHAPES)
def test_split_f16x2_t_planes(K, N, ldw, Kp):
    from marlsat import _lib

    W = _weights(K, N)
    w = operand(W, Placement(0, ldw - N))
    buf, planes, check = _planes(2, N, Kp)
    bad = torch.full((3,), 7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.msat_split_f16x2_t(w.ptr, K, N, ldw, Kp, buf.data_ptr(), bad.data_ptr() + 4, _lib.stream_ptr()),
               "split_f16x2_t")
    torch.cuda.synchronize()
    w.check()
    check()
    X = _padded_t(W, Kp) * 1024.0
    p = X.half()
    lo = (X - p.float()).half()
    for q, ref in enumerate((p, lo)):
        assert torch.equal(planes[q].cpu(), ref.view(torch.int16)), f"plane {q}"
    assert not bool(planes[:, :, K:].any()), "padding k must be exact (+0) zeros"
    assert bad.tolist() == [7, 1, 7]  # 1e30 is among the values; the neighbours of *bad are not touched


def _bad_of(W, ldw, Kp):
    from marlsat import _lib

    K, N = W.shape
    w = operand(W, Placement(0, ldw - N))
    buf, _, check = _planes(2, N, Kp, tail=64)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.msat_split_f16x2_t(w.ptr, K, N, w.ld, Kp, buf.data_ptr(), bad.data_ptr(), _lib.stream_ptr()),
               "split_f16x2_t")
    torch.cuda.synchronize()
    w.check()
    check()
    return int(bad)


@pytest.mark.parametrize("K,N,ldw,Kp", SHAPES)
def test_split_f16x2_t_bad_flag(K, N, ldw, Kp):
    """*bad, pre-set to 7: 0 for in-range weights -- also with NaN in every ld gap and guard row, which operand()
    puts there --, 1 at |W| = 32 and 0 at the float just below, 1 for one NaN, one Inf, and when the only offender
    is the operand's last element."""
    W = _weights(K, N, special=False)
    assert float(W.abs().max()) < 32.0
    assert _bad_of(W, ldw, Kp) == 0
    below = float.fromhex("0x1.fffffep+4")  # the float32 just below 32
    for v, want in ((32.0, 1), (-32.0, 1), (below, 0), (-below, 0), (float("nan"), 1), (float("inf"), 1),
                    (float("-inf"), 1)):
        for pos in ((0, 0), (K - 1, N - 1), (K // 2, N // 3)):
            Wv = W.clone()
            Wv[pos] = v
            assert _bad_of(Wv, ldw, Kp) == want, (v, pos)


def test_split_f16x2_t_bad_flag_ignores_gaps_and_guards():
    """Out-of-range finite values in the ld gap and the guard rows (1e30 instead of NaN) leave *bad at 0."""
    from marlsat import _lib

    K, N, ldw, Kp = SHAPES[2]
    W = _weights(K, N, special=False)
    w = operand(W, Placement(0, ldw - N), fill=1.0e30)
    buf, _, check = _planes(2, N, Kp, tail=64)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.msat_split_f16x2_t(w.ptr, K, N, ldw, Kp, buf.data_ptr(), bad.data_ptr(), _lib.stream_ptr()),
               "split_f16x2_t")
    torch.cuda.synchronize()
    check()
    assert int(bad) == 0


def test_split_bf16x3_t_empty_writes_nothing():
    from marlsat import _lib

    buf, _, check = _planes(3, 4, 32, tail=64)
    buf.fill_(CANARY & 0x7FFF)
    snap = buf.clone()
    for K, N in ((0, 4), (4, 0), (0, 0)):
        assert _lib.lib.msat_split_bf16x3_t(None, K, N, 4, 32, buf.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, snap)
