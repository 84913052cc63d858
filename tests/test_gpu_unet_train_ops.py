"""The U-Net train step's helper kernels (csrc/unet_train.hip) and the sampler's
DDPM update (csrc/unet_ops.hip), each alone through its C-ABI entry point
against a float64 reference built on the CPU from the same fp32 inputs, at the
smallest shapes that reach every branch: K-ring reloads and I/J tails of the
small GEMM with every stride pattern the model uses, accumulate branches,
256-thread tails, the P > 4096 split of the weight-gradient GEMM, the scalar
fallback / 32-tensor chunking / step > 1 of the multi-tensor Adam, the 64-tensor
chunking of concat / split, every residue of L in the train encoder.

Every output a kernel may partly write is prefilled with a sentinel and the
elements outside the addressed region must come back untouched.  Gates are
quoted with their basis next to each test; every measured error goes to
record_error."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ertdiff
from ertdiff import _lib
from oracle import ref_numpy as RN
from conftest import record_error

pytestmark = pytest.mark.gpu
SENT = 777.25            # sentinel: exactly representable, far from any result
EPS32 = float(torch.finfo(torch.float32).eps)


def _rel(a, b):
    return RN.rel_l2(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())


def _ulp(ref):
    """fp32 spacing at |ref| (float64 array in, float64 array out)."""
    r = np.abs(np.asarray(ref, np.float64)).astype(np.float32)
    return np.spacing(r).astype(np.float64)


def _ulps(got, ref):
    """max |got - ref| in fp32 ulps of ref."""
    got = got.detach().double().cpu().numpy()
    ref = np.asarray(ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else ref,
                     np.float64)
    return float(np.max(np.abs(got - ref) / _ulp(ref))) if got.size else 0.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _arr(vals, ctype=ctypes.c_void_p):
    return (ctype * len(vals))(*vals)


def _ptr(t, off=0):
    """device address of element `off` of a float32 tensor's storage view"""
    return t.data_ptr() + 4 * off


# ---------------------------------------------------------------------------------
# ertd_gemm_small
# ---------------------------------------------------------------------------------
GEMM_GATE = 2e-6


def _gemm_case(dev, Abuf, aoff, sA, Bbuf, boff, sB, Cinit, coff, sC, bias, I, J, K, batch, alpha, acc):
    """Run C[b][i][j] (+)= alpha sum_k A[b][i][k] B[b][k][j] (+ bias[j]) on flat fp32
    CPU buffers with element offsets / strides (s_ = (row, col, batch) as the C ABI
    orders them); returns the rel-L2 of the addressed region against float64 and
    asserts everything else in the C buffer is untouched."""
    A = torch.as_strided(Abuf.double(), (batch, I, K), (sA[2], sA[0], sA[1]), aoff)
    Bm = torch.as_strided(Bbuf.double(), (batch, K, J), (sB[2], sB[0], sB[1]), boff)
    val = alpha * (A @ Bm)
    if bias is not None:
        val = val + bias.double()[None, None, :]
    want = Cinit.double().clone()
    mask = torch.zeros(Cinit.numel(), dtype=torch.bool)
    cs = ((batch, I, J), (sC[2], sC[0], sC[1]), coff)
    torch.as_strided(mask, *cs).fill_(True)
    assert int(mask.sum()) == batch * I * J                      # the case addresses no element twice
    wv = torch.as_strided(want, *cs)
    if acc:
        wv.add_(val)
    else:
        wv.copy_(val)
    dA, dB, dC = Abuf.to(dev), Bbuf.to(dev), Cinit.to(dev)
    db = None if bias is None else bias.to(dev)
    rc = _lib.lib().ertd_gemm_small(_ptr(dA, aoff), *sA, _ptr(dB, boff), *sB, _ptr(dC, coff), *sC,
                                    None if db is None else db.data_ptr(), I, J, K, batch,
                                    float(alpha), int(acc), _lib.stream_of(dev))
    assert rc == 0
    got = dC.cpu()
    assert torch.equal(got[~mask], Cinit[~mask]), "wrote outside the addressed region"
    return RN.rel_l2(got[mask].double().numpy(), want[mask].numpy())


@pytest.mark.parametrize("K,I,J,batch,alpha,bias,acc", [
    (1, 1, 1, 1, 1.0, 0, 0),
    (31, 31, 33, 3, -0.37, 1, 1),
    (32, 65, 32, 1, 1.0, 1, 0),
    (33, 31, 33, 1, -0.37, 0, 1),
    (128, 65, 32, 3, 1.0, 0, 0),        # all 4 ring slots, no reload
    (128, 31, 33, 1, -0.37, 1, 1),
    (129, 31, 33, 3, 1.0, 1, 1),        # first reload of ring slot 0 (one ragged k)
    (129, 65, 32, 1, 1.0, 0, 0),
    (160, 1, 1, 3, -0.37, 1, 0),        # a whole reloaded tile
    (160, 31, 33, 1, 1.0, 0, 0),
    (257, 65, 32, 1, -0.37, 0, 1),      # every slot reloaded, a third trip round the outer loop
    (257, 31, 33, 3, 1.0, 1, 0),
    (300, 31, 33, 3, 1.0, 1, 0),
    (300, 65, 32, 1, -0.37, 0, 1),
])
def test_gemm_small_k_ring_tails_flags(K, I, J, batch, alpha, bias, acc, cuda_dev):
    """Row-major A (I, K), B (K, J) into a C with padded rows and batches.
    Gate 2e-6 rel-L2 against float64: torch's fp32 matmul measures 2.9e-7 for
    K <= 512, a k-ordered fma chain is expected within a few times that."""
    g = _gen(1000 * K + 10 * I + J + batch)
    lda, ldb, ldc = K + 2, J + 1, J + 3
    sa_b, sb_b, sc_b = I * lda + 3, K * ldb + 5, I * ldc + 7
    Abuf = torch.randn(batch * sa_b + 4, generator=g)
    Bbuf = torch.randn(batch * sb_b + 4, generator=g)
    Cinit = torch.randn(batch * sc_b + 9, generator=g) if acc else torch.full((batch * sc_b + 9,), SENT)
    bv = torch.randn(J, generator=g) if bias else None
    err = _gemm_case(cuda_dev, Abuf, 1, (lda, 1, sa_b), Bbuf, 2, (ldb, 1, sb_b), Cinit, 3,
                     (ldc, 1, sc_b), bv, I, J, K, batch, alpha, acc)
    record_error(f"gemm_small_K{K}_I{I}_J{J}_b{batch}_a{alpha}_bias{bias}_acc{acc}", err)
    assert err < GEMM_GATE, err


def _model_gemm_patterns():
    """(name, builder) for every stride pattern ertdiff/unet_train.py passes to
    ertd_gemm_small, at reduced sizes.  A builder returns the _gemm_case arguments
    after the device."""
    Bn, Kd, O, ld = 5, 48, 40, 47                 # dense: x (Bn, Kd), w (O, Kd), dy rows strided by ld
    C, N, B = 48, 40, 2                           # attention: qkv (B, 3, C, N)
    CN = C * N
    pats = []

    def dense(name, f):
        pats.append((name, f))

    def rn(g, n):
        return torch.randn(n, generator=g)

    # linear: y (Bn, O) = x W^T + b
    dense("linear", lambda g: (rn(g, Bn * Kd), 0, (Kd, 1, 0), rn(g, O * Kd), 0, (1, Kd, 0),
                               torch.full((Bn * O + 5,), SENT), 0, (O, 1, 0), rn(g, O),
                               Bn, O, Kd, 1, 1.0, 0))
    # linear_backward: dw (O, Kd) = dy^T x, dy (Bn, O) a column block of a wider matrix
    dense("linear_bwd_dw", lambda g: (rn(g, Bn * ld + 3), 3, (1, ld, 0), rn(g, Bn * Kd), 0, (Kd, 1, 0),
                                      torch.full((O * Kd + 5,), SENT), 0, (Kd, 1, 0), None,
                                      O, Kd, Bn, 1, 1.0, 0))
    # ... dx (Bn, Kd) = dy W
    dense("linear_bwd_dx", lambda g: (rn(g, Bn * ld + 3), 3, (ld, 1, 0), rn(g, O * Kd), 0, (Kd, 1, 0),
                                      torch.full((Bn * Kd + 5,), SENT), 0, (Kd, 1, 0), None,
                                      Bn, Kd, O, 1, 1.0, 0))
    # ... dx with a long reduction: O = 320 split in ns = 5 ranges of 64 (batched, partials)
    O2, ld2 = 320, 323
    dense("linear_bwd_dx_split64", lambda g: (rn(g, Bn * ld2 + 3), 3, (ld2, 1, 64), rn(g, O2 * Kd), 0,
                                              (Kd, 1, 64 * Kd), torch.full((5 * Bn * Kd + 5,), SENT), 0,
                                              (Kd, 1, Bn * Kd), None, Bn, Kd, 64, 5, 1.0, 0))
    # a broadcast operand over a batch (a_b = 0): one A against 3 B's
    dense("broadcast_a_b0", lambda g: (rn(g, Bn * Kd), 0, (Kd, 1, 0), rn(g, 3 * Kd * O), 0, (O, 1, Kd * O),
                                       torch.full((3 * Bn * O + 5,), SENT), 0, (O, 1, Bn * O), None,
                                       Bn, O, Kd, 3, 1.0, 0))
    # attention forward: S[i][j] = sum_c q[c][i] k[c][j]; O[c][i] = sum_j v[c][j] P[i][j]
    dense("attn_fwd_S", lambda g: (rn(g, B * 3 * CN), 0, (1, N, 3 * CN), None, CN, (N, 1, 3 * CN),
                                   torch.full((B * N * N + 5,), SENT), 0, (N, 1, N * N), None,
                                   N, N, C, B, 1.0, 0))
    dense("attn_fwd_O", lambda g: (rn(g, B * 3 * CN), 2 * CN, (N, 1, 3 * CN), rn(g, B * N * N), 0, (1, N, N * N),
                                   torch.full((B * CN + 5,), SENT), 0, (N, 1, CN), None,
                                   C, N, N, B, 1.0, 0))
    # attention backward, into the slices of dqkv (B, 3, C, N)
    dense("attn_bwd_dV", lambda g: (rn(g, B * CN), 0, (N, 1, CN), rn(g, B * N * N), 0, (N, 1, N * N),
                                    torch.full((B * 3 * CN + 5,), SENT), 2 * CN, (N, 1, 3 * CN), None,
                                    C, N, N, B, 1.0, 0))
    dense("attn_bwd_dP", lambda g: (rn(g, B * CN), 0, (1, N, CN), rn(g, B * 3 * CN), 2 * CN, (N, 1, 3 * CN),
                                    torch.full((B * N * N + 5,), SENT), 0, (N, 1, N * N), None,
                                    N, N, C, B, 1.0, 0))
    dense("attn_bwd_dQ", lambda g: (rn(g, B * 3 * CN), CN, (N, 1, 3 * CN), rn(g, B * N * N), 0, (1, N, N * N),
                                    torch.full((B * 3 * CN + 5,), SENT), 0, (N, 1, 3 * CN), None,
                                    C, N, N, B, 1.0, 0))
    dense("attn_bwd_dK", lambda g: (rn(g, B * 3 * CN), 0, (N, 1, 3 * CN), rn(g, B * N * N), 0, (N, 1, N * N),
                                    torch.full((B * 3 * CN + 5,), SENT), CN, (N, 1, 3 * CN), None,
                                    C, N, N, B, 1.0, 0))
    return pats


@pytest.mark.parametrize("name,build", _model_gemm_patterns(), ids=[n for n, _ in _model_gemm_patterns()])
def test_gemm_small_model_stride_patterns(name, build, cuda_dev):
    """Every (a_i, a_k, a_b, b_k, b_j, b_b, c_i, c_j, c_b) pattern of linear,
    linear_backward and the attention forward / backward walk, C = 48, N = 40."""
    args = list(build(_gen(sum(map(ord, name)))))
    if args[3] is None:            # q and k (or dO-side operand and v) live in the one qkv buffer
        args[3] = args[0]
    err = _gemm_case(cuda_dev, *args)
    record_error(f"gemm_small_{name}", err)
    assert err < GEMM_GATE, err


def test_gemm_small_rejects(cuda_dev):
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    x = torch.zeros(16, device=cuda_dev)
    p = x.data_ptr()
    for I, J, K, batch in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert lib.ertd_gemm_small(p, 1, 1, 0, p, 1, 1, 0, p, 1, 1, 0, None, I, J, K, batch, 1.0, 0,
                                   st) == _lib.ERTD_EINVAL
    assert lib.ertd_gemm_small(None, 1, 1, 0, p, 1, 1, 0, p, 1, 1, 0, None, 1, 1, 1, 1, 1.0, 0,
                               st) == _lib.ERTD_EINVAL


# ---------------------------------------------------------------------------------
# ertd_softmax_rows / ertd_softmax_backward
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", [1.0, 30.0, 200.0])
@pytest.mark.parametrize("N", [1, 7, 100, 256, 300, 1000])
def test_softmax_rows_and_backward(N, mult, cuda_dev):
    """Gate 1e-6 rel-L2 against float64 (the backward evaluated on the fp32 P the
    kernel is given): torch's fp32 CPU softmax / backward measure at most
    7.7e-8 / 2.3e-7 on these cases; the margin covers the device expf and the
    reduction order."""
    rows, scale = 37, 1.0 / 16.0
    g = _gen(7 * N + int(mult))
    S = torch.randn(rows, N, generator=g) * mult
    dP = torch.randn(rows, N, generator=g)
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    Sd = S.to(cuda_dev)
    P = torch.full((rows + 1, N), SENT, device=cuda_dev)
    assert lib.ertd_softmax_rows(Sd.data_ptr(), rows, N, scale, P.data_ptr(), st) == 0
    assert bool((P[rows] == SENT).all())
    P = P[:rows]
    ref = torch.softmax(S.double() * scale, dim=-1)
    e_f = _rel(P, ref)
    dS = torch.full((rows + 1, N), SENT, device=cuda_dev)
    dPd = dP.to(cuda_dev)
    assert lib.ertd_softmax_backward(P.data_ptr(), dPd.data_ptr(), rows, N, scale, dS.data_ptr(), st) == 0
    assert bool((dS[rows] == SENT).all())
    P64 = P.cpu().double()
    ref_b = scale * P64 * (dP.double() - (P64 * dP.double()).sum(-1, keepdim=True))
    record_error(f"softmax_rows_N{N}_x{mult}", e_f)
    if N == 1:
        assert bool((P == 1.0).all()) and bool((dS[:rows] == 0.0).all())
        return
    e_b = _rel(dS[:rows], ref_b)
    record_error(f"softmax_backward_N{N}_x{mult}", e_b)
    assert e_f < 1e-6 and e_b < 1e-6, (e_f, e_b)


def test_softmax_rows_equal_large_values(cuda_dev):
    """A row of equal values 1e4 (logit 625 after the scale: expf overflows
    without the max subtraction) gives 1/N, no NaN."""
    N = 300
    S = torch.full((3, N), 1e4, device=cuda_dev)
    P = torch.empty_like(S)
    assert _lib.lib().ertd_softmax_rows(S.data_ptr(), 3, N, 1.0 / 16.0, P.data_ptr(),
                                        _lib.stream_of(cuda_dev)) == 0
    assert bool(torch.isfinite(P).all())
    assert _ulps(P, np.full((3, N), 1.0 / N)) <= 1.0


# ---------------------------------------------------------------------------------
# ertd_eltwise
# ---------------------------------------------------------------------------------
def _silu64(x):
    return x / (1.0 + torch.exp(-x))


def _silu_grad64(x):
    s = 1.0 / (1.0 + torch.exp(-x))
    return s * (1.0 + x * (1.0 - s))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
def test_eltwise(op, n, acc, cuda_dev):
    """SILU / SILU_BWD within 2 fp32 ulp of float64 per element (with accumulate:
    plus the half ulp of the one fp32 add onto the previous content); RELU,
    RELU_BWD, ADD, SCALE bitwise the same fp32 expression in torch."""
    g = _gen(100 * op + n + acc)
    x = torch.randn(n, generator=g) * 3
    y = torch.randn(n, generator=g)
    init = torch.randn(n + 7, generator=g)
    init[n:] = SENT
    alpha = -1.7
    out = init.to(cuda_dev)
    xd, yd = x.to(cuda_dev), y.to(cuda_dev)
    two = op in (1, 3, 4)
    rc = _lib.lib().ertd_eltwise(op, xd.data_ptr(), yd.data_ptr() if two else None, out.data_ptr(), n,
                                 alpha, acc, _lib.stream_of(cuda_dev))
    assert rc == 0
    got = out.cpu()
    assert bool((got[n:] == SENT).all())
    got = got[:n]
    if op in (0, 1):
        v = _silu64(x.double()) if op == 0 else y.double() * _silu_grad64(x.double())
        tol = 2.0 * _ulp(v.numpy())
        want = v
        if acc:
            want = init[:n].double() + v
            tol = tol + 0.5 * _ulp(want.numpy())
        d = np.abs(got.double().numpy() - want.numpy())
        worst = float(np.max(d / tol))
        record_error(f"eltwise_op{op}_n{n}_acc{acc}_frac_of_bound", worst)
        assert worst <= 1.0, (worst, int(np.argmax(d / tol)), float(x[int(np.argmax(d / tol))]))
        return
    if op == 2:
        v = torch.clamp_min(x, 0.0)
    elif op == 3:
        v = torch.where(x > 0, y, torch.zeros_like(y))
    elif op == 4:
        v = x + y
    else:
        v = torch.tensor(alpha, dtype=torch.float32) * x
    want = init[:n] + v if acc else v
    assert torch.equal(got, want)


def test_eltwise_rejects(cuda_dev):
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    x = torch.zeros(8, device=cuda_dev)
    p = x.data_ptr()
    assert lib.ertd_eltwise(6, p, p, p, 8, 1.0, 0, st) == _lib.ERTD_EINVAL
    assert lib.ertd_eltwise(-1, p, p, p, 8, 1.0, 0, st) == _lib.ERTD_EINVAL
    for op in (1, 3, 4):
        assert lib.ertd_eltwise(op, p, None, p, 8, 1.0, 0, st) == _lib.ERTD_EINVAL, op
    assert lib.ertd_eltwise(0, p, None, p, 0, 1.0, 0, st) == _lib.ERTD_EINVAL


# ---------------------------------------------------------------------------------
# pure data movement: bitwise against torch indexing
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Ho", [1, 3, 16])
def test_zero_insert(Ho, cuda_dev):
    B, C = 2, 3
    x = torch.randn(B, C, Ho, Ho, generator=_gen(Ho))
    n = B * C * 4 * Ho * Ho
    out = torch.full((n + 7,), SENT, device=cuda_dev)
    xd = x.to(cuda_dev)
    assert _lib.lib().ertd_zero_insert(xd.data_ptr(), B, C, Ho, out.data_ptr(), _lib.stream_of(cuda_dev)) == 0
    want = torch.zeros(B, C, 2 * Ho, 2 * Ho)
    want[:, :, ::2, ::2] = x
    got = out.cpu()
    assert torch.equal(got[:n].view_as(want), want) and bool((got[n:] == SENT).all())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("HW", [1, 100, 300])
def test_channel_slice(HW, acc, cuda_dev):
    B, Cs, c0, Cd, Cdst, d0 = 2, 7, 2, 3, 6, 1
    g = _gen(HW + acc)
    src = torch.randn(B, Cs, HW, generator=g)
    init = torch.randn(B, Cdst, HW, generator=g)
    dst, sd = init.to(cuda_dev), src.to(cuda_dev)
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    assert lib.ertd_channel_slice(sd.data_ptr(), B, Cs, c0, Cd, HW, dst.data_ptr(), Cdst, d0, acc, st) == 0
    want = init.clone()
    if acc:
        want[:, d0:d0 + Cd] += src[:, c0:c0 + Cd]
    else:
        want[:, d0:d0 + Cd] = src[:, c0:c0 + Cd]
    assert torch.equal(dst.cpu(), want)          # the other channels of dst untouched
    # slices that leave the source or the destination
    for a in ((5, 3, 6, 1), (2, 3, 6, 4), (-1, 3, 6, 1), (2, 3, 6, -1), (2, 0, 6, 1)):
        assert lib.ertd_channel_slice(sd.data_ptr(), B, Cs, a[0], a[1], HW, dst.data_ptr(), a[2], a[3],
                                      0, st) == _lib.ERTD_EINVAL, a


@pytest.mark.parametrize("ks", [1, 3])
def test_conv_weight_flip(ks, cuda_dev):
    Cout, Cin = 37, 5                            # 37 * 5 * 9 elements: several workgroups and a tail
    w = torch.randn(Cout, Cin, ks, ks, generator=_gen(ks))
    n = w.numel()
    out = torch.full((n + 7,), SENT, device=cuda_dev)
    wd = w.to(cuda_dev)
    assert _lib.lib().ertd_conv_weight_flip(wd.data_ptr(), Cout, Cin, ks, out.data_ptr(),
                                            _lib.stream_of(cuda_dev)) == 0
    want = w.transpose(0, 1).flip(2, 3).contiguous()
    got = out.cpu()
    assert torch.equal(got[:n].view_as(want), want) and bool((got[n:] == SENT).all())


def _ragged_sizes():
    """70 tensor sizes crossing the 64-tensor chunking, zero-length ones first,
    in the middle, on both sides of the chunk boundary, and last."""
    sizes = [(i * 37) % 301 + 1 for i in range(70)]
    for i in (0, 35, 63, 64, 69):
        sizes[i] = 0
    return sizes


def test_concat_and_split(cuda_dev):
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    sizes = _ragged_sizes()
    total = sum(sizes)
    gap = 3                                       # floats between consecutive tensors in the pool
    offs, o = [], 1
    for n in sizes:
        offs.append(o)
        o += n + gap
    g = _gen(70)
    pool = torch.randn(o, generator=g)
    pd = pool.to(cuda_dev)
    csz = _arr(sizes, ctypes.c_longlong)
    # concat: dst = cat(pool regions)
    dst = torch.full((total + 8,), SENT, device=cuda_dev)
    srcs = _arr([_ptr(pd, k) for k in offs])
    assert lib.ertd_concat(srcs, csz, len(sizes), dst.data_ptr(), st) == 0
    want = torch.cat([pool[k:k + n] for k, n in zip(offs, sizes)])
    got = dst.cpu()
    assert torch.equal(got[:total], want) and bool((got[total:] == SENT).all())
    # split: region k = 0.25 * src chunk k, the gaps untouched
    src = torch.randn(total, generator=g)
    sd = src.to(cuda_dev)
    out = torch.full((o,), SENT, device=cuda_dev)
    dsts = _arr([_ptr(out, k) for k in offs])
    assert lib.ertd_split(sd.data_ptr(), dsts, csz, len(sizes), 0.25, st) == 0
    want = torch.full((o,), SENT)
    base = 0
    for k, n in zip(offs, sizes):
        want[k:k + n] = torch.tensor(0.25) * src[base:base + n]
        base += n
    assert torch.equal(out.cpu(), want)
    # bad arguments
    neg = _arr([4, -1], ctypes.c_longlong)
    two = _arr([_ptr(pd, 0), _ptr(pd, 8)])
    assert lib.ertd_concat(two, neg, 2, dst.data_ptr(), st) == _lib.ERTD_EINVAL
    assert lib.ertd_split(sd.data_ptr(), two, neg, 2, 1.0, st) == _lib.ERTD_EINVAL
    assert lib.ertd_concat(two, csz, 0, dst.data_ptr(), st) == _lib.ERTD_EINVAL
    assert lib.ertd_concat(_arr([_ptr(pd, 0), None]), _arr([4, 4], ctypes.c_longlong), 2, dst.data_ptr(),
                           st) == _lib.ERTD_EINVAL


@pytest.mark.parametrize("ks,mode,H", [
    (1, 0, 1), (1, 0, 2),
    (3, 0, 1), (3, 0, 2), (3, 0, 5),             # stride 1
    (3, 1, 2), (3, 1, 4), (3, 1, 6),             # stride 2 (even H: the smallest is 2)
    (3, 2, 1), (3, 2, 2), (3, 2, 5),             # nearest-x2 upsample, then stride 1
])
def test_im2col_vs_unfold(ks, mode, H, cuda_dev):
    B, C = 2, 3
    x = torch.randn(B, C, H, H, generator=_gen(10 * ks + mode + H))
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if mode == 2 else x
    want = F.unfold(xin, ks, padding=ks // 2, stride=2 if mode == 1 else 1)
    n = want.numel()
    out = torch.full((n + 7,), SENT, device=cuda_dev)
    xd = x.to(cuda_dev)
    assert _lib.lib().ertd_im2col(xd.data_ptr(), C, B, H, ks, mode, out.data_ptr(),
                                  _lib.stream_of(cuda_dev)) == 0
    got = out.cpu()
    assert torch.equal(got[:n].view_as(want), want) and bool((got[n:] == SENT).all())


def test_im2col_rejects(cuda_dev):
    """A stride-2 patch matrix has H / 2 columns per side, the conv's output size
    only for even H (every stride-2 conv of a U-Net config has one: power-of-two
    images); odd H (H = 1 would be an empty launch) is refused."""
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    x = torch.zeros(2 * 3 * 25, device=cuda_dev)
    out = torch.full((2 * 27 * 100,), SENT, device=cuda_dev)
    for ks, mode, H in ((3, 1, 1), (3, 1, 3), (3, 1, 5), (1, 1, 2), (1, 2, 2), (2, 0, 2), (3, 3, 2),
                        (3, -1, 2), (3, 0, 0)):
        assert lib.ertd_im2col(x.data_ptr(), 3, 2, H, ks, mode, out.data_ptr(), st) == _lib.ERTD_EINVAL, \
            (ks, mode, H)
    assert bool((out == SENT).all())


# ---------------------------------------------------------------------------------
# fixed-order sums
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("H", [1, 3, 16])
def test_sum_pool2_bitwise(H, acc, cuda_dev):
    B, C = 2, 3
    g = _gen(H + acc)
    x = torch.randn(B, C, 2 * H, 2 * H, generator=g)
    n = B * C * H * H
    init = torch.randn(n + 7, generator=g)
    init[n:] = SENT
    out, xd = init.to(cuda_dev), x.to(cuda_dev)
    assert _lib.lib().ertd_sum_pool2(xd.data_ptr(), B, C, H, out.data_ptr(), acc,
                                     _lib.stream_of(cuda_dev)) == 0
    v = (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])
    want = init[:n].view_as(v) + v if acc else v
    got = out.cpu()
    assert torch.equal(got[:n].view_as(want), want) and bool((got[n:] == SENT).all())


@pytest.mark.parametrize("HW", [4, 255, 1024])
def test_channel_sums(HW, cuda_dev):
    """out_bc: the float64 sum rounded to fp32, within 1 ulp, into a column block
    of a wider matrix (ldo > C) with the neighbours untouched.  out_c (ldo = C):
    the sum over samples of the fp32 out_bc the kernel wrote, with and without
    accumulate_c: a handful of fp32 adds, each within half an ulp of the summed
    magnitudes (bound 2 ulp of sum |terms|)."""
    B, C = 3, 5
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    x = torch.randn(B, C, HW, generator=_gen(HW))
    xd = x.to(cuda_dev)
    ref = x.double().sum(2)
    ldo = C + 4
    wide = torch.full((B, ldo), SENT, device=cuda_dev)
    assert lib.ertd_channel_sums(xd.data_ptr(), B, C, HW, _ptr(wide, 2), ldo, None, 0, st) == 0
    w = wide.cpu()
    assert bool((w[:, :2] == SENT).all()) and bool((w[:, 2 + C:] == SENT).all())
    u = _ulps(w[:, 2:2 + C], ref)
    record_error(f"channel_sums_HW{HW}_ulps", u)
    assert u <= 1.0, u
    for acc in (0, 1):
        bc = torch.full((B * C + 3,), SENT, device=cuda_dev)
        init = torch.randn(C + 3, generator=_gen(HW + acc))
        init[C:] = SENT
        oc = init.to(cuda_dev)
        assert lib.ertd_channel_sums(xd.data_ptr(), B, C, HW, bc.data_ptr(), 0, oc.data_ptr(), acc, st) == 0
        bcv, ocv = bc.cpu(), oc.cpu()
        assert bool((bcv[B * C:] == SENT).all()) and bool((ocv[C:] == SENT).all())
        assert torch.equal(bcv[:B * C].view(B, C), w[:, 2:2 + C])
        terms = bcv[:B * C].view(B, C).double()
        want = terms.sum(0) + (init[:C].double() if acc else 0.0)
        mag = terms.abs().sum(0) + (init[:C].double().abs() if acc else 0.0)
        assert bool(((ocv[:C].double() - want).abs() <= 2.0 * EPS32 * mag).all())
    # out_c needs the dense layout; ldo below C is refused
    oc = torch.zeros(C, device=cuda_dev)
    assert lib.ertd_channel_sums(xd.data_ptr(), B, C, HW, wide.data_ptr(), ldo, oc.data_ptr(), 0,
                                 st) == _lib.ERTD_EINVAL
    assert lib.ertd_channel_sums(xd.data_ptr(), B, C, HW, wide.data_ptr(), C - 1, None, 0,
                                 st) == _lib.ERTD_EINVAL


# ---------------------------------------------------------------------------------
# ertd_mse_loss
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 65536, 65537, 300001])
def test_mse_loss(n, cuda_dev):
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    g = _gen(n)
    e, z = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ed, zd = e.to(cuda_dev), z.to(cuda_dev)
    nws = lib.ertd_mse_loss_ws_bytes()
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda_dev)
    loss = torch.full((2,), SENT, device=cuda_dev)
    dout = torch.full((n + 7,), SENT, device=cuda_dev)
    assert lib.ertd_mse_loss(ed.data_ptr(), zd.data_ptr(), n, loss.data_ptr(), dout.data_ptr(),
                             ws.data_ptr(), nws, st) == 0
    ref = float(((e.double() - z.double()) ** 2).mean())
    got = loss.cpu()
    assert float(got[1]) == SENT
    u = abs(float(got[0]) - ref) / float(_ulp(ref))
    record_error(f"mse_loss_n{n}_ulps", u)
    assert u <= 1.0, (u, float(got[0]), ref)
    d = dout.cpu()
    want = (e - z) * torch.tensor(2.0 / n, dtype=torch.float64).float()
    assert torch.equal(d[:n], want) and bool((d[n:] == SENT).all())
    # dout is optional: the same loss bits without it
    loss2 = torch.full((2,), SENT, device=cuda_dev)
    assert lib.ertd_mse_loss(ed.data_ptr(), zd.data_ptr(), n, loss2.data_ptr(), None, ws.data_ptr(), nws,
                             st) == 0
    assert torch.equal(loss2.cpu(), got)
    assert lib.ertd_mse_loss(ed.data_ptr(), zd.data_ptr(), n, loss2.data_ptr(), None, ws.data_ptr(),
                             nws - 1, st) == _lib.ERTD_ENOSPC


# ---------------------------------------------------------------------------------
# ertd_wgrad_gemm
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [37, 4096, 4096 + 37])
def test_wgrad_gemm(P, cuda_dev):
    """dW (M, N) = sum_b dY_b X_b^T, written and then accumulated once more; the
    last P is a ragged second split.  Gate 1e-5 (test_conv_wgrad_vs_autograd's)."""
    M, N, B = 65, 70, 3
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    g = _gen(P)
    dY, X = torch.randn(B, M, P, generator=g), torch.randn(B, N, P, generator=g)
    ref = torch.einsum("bmp,bnp->mn", dY.double(), X.double())
    nws = lib.ertd_wgrad_ws_bytes(M, N, P, B)
    assert nws == B * ((P + 4095) // 4096) * M * N * 4
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda_dev)
    out = torch.full((M * N + 7,), SENT, device=cuda_dev)
    dYd, Xd = dY.to(cuda_dev), X.to(cuda_dev)
    for acc in (0, 1):
        assert lib.ertd_wgrad_gemm(dYd.data_ptr(), Xd.data_ptr(), M, N, P, B, M * P, N * P, out.data_ptr(),
                                   acc, ws.data_ptr(), nws, st) == 0
        got = out.cpu()
        assert bool((got[M * N:] == SENT).all())
        err = RN.rel_l2(got[:M * N].view(M, N).double().numpy(), ((1 + acc) * ref).numpy())
        record_error(f"wgrad_gemm_P{P}_acc{acc}", err)
        assert err < 1e-5, (acc, err)
    assert lib.ertd_wgrad_gemm(dYd.data_ptr(), Xd.data_ptr(), M, N, P, B, M * P, N * P, out.data_ptr(), 0,
                               ws.data_ptr(), nws - 1, st) == _lib.ERTD_ENOSPC


# ---------------------------------------------------------------------------------
# ertd_adam_multi
# ---------------------------------------------------------------------------------
def test_adam_multi_five_steps_vs_float64(cuda_dev):
    """5 consecutive steps over 70 tensors (three launches of <= 32) against
    torch.optim.Adam on float64 copies with the same lr, betas and eps.  Odd
    tensors are 4-byte-offset views of a larger buffer (the scalar fallback
    beside the float4 path); every buffer carries sentinels around the tensor.
    |g| in [0.1, 2] keeps m / sqrt(v) well conditioned.  Gates per tensor and
    step: exp_avg / exp_avg_sq rel-L2 < 1e-6, the parameter delta from the start
    < 1e-5 (torch's fp32 CPU Adam: 8.8e-8 and 1.3e-6 on such inputs, the delta
    error being the rounding of p itself)."""
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    lr, b1, b2, eps = 2.0 ** -10, 0.9, 0.999, 1e-8
    size_set = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4097]
    sizes = [size_set[(i * 4 + i // 9) % 9] for i in range(70)]
    assert set(sizes) == set(size_set)
    g = _gen(5)
    offs = [i % 2 for i in range(70)]             # odd tensors: one float past the aligned base

    P0 = [0.02 * torch.randn(n, generator=g) for n in sizes]
    bufs = {k: [] for k in "pgmv"}
    for n, o, p0 in zip(sizes, offs, P0):
        for k in "pgmv":
            t = torch.full((n + 5,), SENT)
            t[o:o + n] = p0 if k == "p" else 0.0
            bufs[k].append(t.to(cuda_dev))
    ptrs = {k: _arr([_ptr(t, o) for t, o in zip(bufs[k], offs)]) for k in "pgmv"}
    csz = _arr(sizes, ctypes.c_longlong)
    ref_p = [torch.nn.Parameter(p.double()) for p in P0]
    opt = torch.optim.Adam(ref_p, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    assert lib.ertd_adam_multi(ptrs["p"], ptrs["g"], ptrs["m"], ptrs["v"], csz, 70, 0, lr, b1, b2, eps,
                               st) == _lib.ERTD_EINVAL
    worst = {"exp_avg": 0.0, "exp_avg_sq": 0.0, "delta": 0.0}
    for step in range(1, 6):
        for i, (n, o) in enumerate(zip(sizes, offs)):
            gr = (0.1 + 1.9 * torch.rand(n, generator=g)) * (2.0 * torch.randint(0, 2, (n,), generator=g) - 1.0)
            gr = gr.float()
            bufs["g"][i][o:o + n] = gr.to(cuda_dev)
            ref_p[i].grad = gr.double()
        assert lib.ertd_adam_multi(ptrs["p"], ptrs["g"], ptrs["m"], ptrs["v"], csz, 70, step, lr, b1, b2,
                                   eps, st) == 0
        opt.step()
        for i, (n, o) in enumerate(zip(sizes, offs)):
            got = {k: bufs[k][i].cpu() for k in "pmv"}
            for k in "pmv":                        # sentinels before and after the tensor
                assert bool((got[k][:o] == SENT).all()) and bool((got[k][o + n:] == SENT).all()), (i, k)
            if n == 0:
                continue
            s = opt.state[ref_p[i]]
            e_m = RN.rel_l2(got["m"][o:o + n].double().numpy(), s["exp_avg"].numpy())
            e_v = RN.rel_l2(got["v"][o:o + n].double().numpy(), s["exp_avg_sq"].numpy())
            e_d = RN.rel_l2((got["p"][o:o + n].double() - P0[i].double()).numpy(),
                            (ref_p[i].detach() - P0[i].double()).numpy())
            worst["exp_avg"] = max(worst["exp_avg"], e_m)
            worst["exp_avg_sq"] = max(worst["exp_avg_sq"], e_v)
            worst["delta"] = max(worst["delta"], e_d)
            assert e_m < 1e-6 and e_v < 1e-6 and e_d < 1e-5, (step, i, n, o, e_m, e_v, e_d)
    for k, v in worst.items():
        record_error(f"adam_multi_5steps_{k}", v)


# ---------------------------------------------------------------------------------
# ertd_gn_act_apply
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [1, 2])
def test_gn_act_apply(act, cuda_dev):
    """act(cat(x, x2) * scale + shift) on a concatenated input, within 2 fp32 ulp
    of float64 per element (act 1 GroupNorm + SiLU, 2 GroupNorm alone)."""
    B, Ca, Cb, HW = 2, 24, 8, 100
    C = Ca + Cb
    g = _gen(act)
    x = torch.randn(B, C, HW, generator=g) * 1.5
    ss = torch.stack([torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g)], -1).contiguous()
    xa, xb = x[:, :Ca].contiguous().to(cuda_dev), x[:, Ca:].contiguous().to(cuda_dev)
    n = B * C * HW
    out = torch.full((n + 7,), SENT, device=cuda_dev)
    ssd = ss.to(cuda_dev)
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    assert lib.ertd_gn_act_apply(xa.data_ptr(), Ca, xb.data_ptr(), Cb, B, HW, ssd.data_ptr(), act,
                                 out.data_ptr(), st) == 0
    v = x.double() * ss[..., 0, None].double() + ss[..., 1, None].double()
    if act == 1:
        v = _silu64(v)
    got = out.cpu()
    assert bool((got[n:] == SENT).all())
    u = _ulps(got[:n].view(B, C, HW), v)
    record_error(f"gn_act_apply_act{act}_ulps", u)
    assert u <= 2.0, u
    assert lib.ertd_gn_act_apply(xa.data_ptr(), Ca, xb.data_ptr(), Cb, B, HW, ssd.data_ptr(), 0,
                                 out.data_ptr(), st) == _lib.ERTD_EINVAL
    assert lib.ertd_gn_act_apply(xa.data_ptr(), Ca, None, Cb, B, HW, ssd.data_ptr(), act,
                                 out.data_ptr(), st) == _lib.ERTD_EINVAL


# ---------------------------------------------------------------------------------
# ertd_encoder_train_fwd / ertd_encoder_train_bwd
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 5, 253, 254, 255, 256, 4693])
def test_encoder_train_fwd_bwd(L, golden_weights, cuda_dev):
    """The train step's condition encoder alone at every residue of L and across
    strip boundaries, seed-42 weights: the pooled activations m against float64
    (2e-6, test_encoder_ragged_lengths' gate) and the four conv-parameter
    gradients of sum(g * m) for a random g against float64 autograd (1e-4,
    test_gpu_train.py's GRAD_TOL); elements whose true gradient is exactly zero
    (taps that only ever see the zero padding) must be exactly zero."""
    from synth import synth_uniform
    B = 3
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    W = {k: torch.from_numpy(np.asarray(golden_weights[f"condition_encoder.{k}"]))
         for k in ("0.weight", "0.bias", "2.weight", "2.bias")}
    Wd = {k: v.to(cuda_dev) for k, v in W.items()}
    cond_np = synth_uniform((B, 14, L), 2000 + L)
    cond = torch.from_numpy(cond_np).to(cuda_dev)
    packed = torch.empty(lib.ertd_packed_floats(), device=cuda_dev)
    assert lib.ertd_encoder_train_pack(Wd["0.weight"].data_ptr(), Wd["2.weight"].data_ptr(),
                                       packed.data_ptr(), st) == 0
    nws = lib.ertd_encoder_train_ws_bytes(B, L)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda_dev)
    m = torch.full((B * 64 + 7,), SENT, device=cuda_dev)
    assert lib.ertd_encoder_train_fwd(packed.data_ptr(), Wd["0.bias"].data_ptr(), Wd["2.bias"].data_ptr(),
                                      cond.data_ptr(), B, L, m.data_ptr(), ws.data_ptr(), nws, st) == 0
    w64 = {k: v.double().numpy() for k, v in W.items()}
    z1, _ = RN.conv1d_s2(cond_np.astype(np.float64), w64["0.weight"], w64["0.bias"])
    z2, _ = RN.conv1d_s2(np.maximum(z1, 0), w64["2.weight"], w64["2.bias"])
    m_ref = np.maximum(z2, 0).mean(axis=2)
    L2 = z2.shape[2]
    mg = m.cpu()
    assert bool((mg[B * 64:] == SENT).all())
    e_m = RN.rel_l2(mg[:B * 64].view(B, 64).double().numpy(), m_ref)
    record_error(f"encoder_train_fwd_L{L}", e_m)
    assert e_m < 2e-6, e_m
    # gradients of sum(g * m); the entry point takes g / L2
    gvec = torch.randn(B, 64, generator=_gen(L))
    Wr = {k: v.double().requires_grad_(True) for k, v in W.items()}
    a1 = F.relu(F.conv1d(torch.from_numpy(cond_np).double(), Wr["0.weight"], Wr["0.bias"], stride=2, padding=1))
    a2 = F.relu(F.conv1d(a1, Wr["2.weight"], Wr["2.bias"], stride=2, padding=1))
    assert a2.shape[2] == L2
    (a2.mean(2) * gvec.double()).sum().backward()
    gm = (gvec.double() / L2).float().to(cuda_dev)
    outs = {k: torch.full((W[k].numel() + 7,), SENT, device=cuda_dev) for k in W}
    assert lib.ertd_encoder_train_bwd(packed.data_ptr(), cond.data_ptr(), gm.data_ptr(), B, L,
                                      outs["0.weight"].data_ptr(), outs["0.bias"].data_ptr(),
                                      outs["2.weight"].data_ptr(), outs["2.bias"].data_ptr(),
                                      ws.data_ptr(), nws, st) == 0
    worst = 0.0
    for k in W:
        got = outs[k].cpu()
        nk = W[k].numel()
        assert bool((got[nk:] == SENT).all()), k
        got = got[:nk].view_as(W[k])
        ref = Wr[k].grad
        assert bool((got[ref == 0] == 0).all()), k
        if float(ref.norm()) == 0:
            continue
        e = _rel(got, ref)
        worst = max(worst, e)
        assert e < 1e-4, (k, e)
    record_error(f"encoder_train_bwd_L{L}", worst)


# ---------------------------------------------------------------------------------
# ertd_unet_update
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_kind", ["injected", "philox"])
@pytest.mark.parametrize("t", [0, 1, 5])
def test_unet_update(t, noise_kind, cuda_dev):
    """x <- c1[t] (x - c2[t] eps) + sigma[t] z for t > 0, no noise term at t = 0,
    against the float64 restatement; bound 2 fp32 ulp of the summed term
    magnitudes (as test_q_sample_one_ulp bounds q_sample).  Injected noise is
    (num_steps, B, P), read at row (num_steps - t) B + b; Philox noise is the
    stream ertdiff.philox_normal draws for the same seed, member offset and t."""
    B, P, num_steps = 5, 1000, 6                  # t = 5 = num_steps - 1
    seed, member_offset = 1234, 3
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    g = _gen(t)
    x, eps = torch.randn(B, P, generator=g), torch.randn(B, P, generator=g)
    betas, alphas, ab = ertdiff.get_diffusion_schedule(50)
    from ertdiff.schedule import step_tables
    tab = step_tables(betas, alphas, ab, num_steps)           # (3, num_steps): c1, c2, sigma
    noise = torch.randn(num_steps, B, P, generator=g)
    xd = torch.cat([x.reshape(-1), torch.full((7,), SENT)]).to(cuda_dev)
    epsd, tabd, nd = eps.to(cuda_dev), tab.to(cuda_dev), noise.to(cuda_dev)
    tdev = torch.tensor([t], dtype=torch.int32, device=cuda_dev)
    inj = noise_kind == "injected"
    assert lib.ertd_unet_update(xd.data_ptr(), epsd.data_ptr(), tabd[0].data_ptr(), tabd[1].data_ptr(),
                                tabd[2].data_ptr(), nd.data_ptr() if inj else None, num_steps,
                                tdev.data_ptr(), seed, member_offset, B, P, st) == 0
    if inj:
        z = noise[num_steps - t] if t > 0 else torch.zeros(B, P)
    else:
        z = ertdiff.philox_normal(B, P, t, 0, seed, member_offset, cuda_dev).cpu()
    c1, c2, sg = (float(tab[i, t]) for i in range(3))
    a, b = c1 * x.double(), c1 * c2 * eps.double()
    ref = a - b
    mag = a.abs() + b.abs()
    if t > 0:
        ref = ref + sg * z.double()
        mag = mag + (sg * z.double()).abs()
    got = xd.cpu()
    assert bool((got[B * P:] == SENT).all())
    got = got[:B * P].view(B, P).double()
    frac = float(((got - ref).abs() / (2 * EPS32 * mag)).max())
    record_error(f"unet_update_t{t}_{noise_kind}_frac_of_bound", frac)
    assert frac <= 1.0, frac
    if t == 0:
        # no noise term at all: independent of the noise source, bitwise
        x2 = x.reshape(-1).to(cuda_dev)
        assert lib.ertd_unet_update(x2.data_ptr(), epsd.data_ptr(), tabd[0].data_ptr(), tabd[1].data_ptr(),
                                    tabd[2].data_ptr(), None if inj else nd.data_ptr(), num_steps,
                                    tdev.data_ptr(), seed + 1, 0, B, P, st) == 0
        assert torch.equal(x2.cpu(), xd.cpu()[:B * P])
