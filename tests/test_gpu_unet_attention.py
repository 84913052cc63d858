"""The U-Net mid-block attention core alone (ertd_attention / ertdiff.unet.attention,
csrc/unet_ops.hip attention_kernel) against the float64 composition
softmax(q^T k / sqrt(C)) applied to v, built from the same fp32 qkv.

Beyond test_attention (C = 256, near-uniform softmax): C = 512 (a second pass
of the V.P^T channel loop and a 256-step Q.K reduction), a peaked softmax whose
logits overflow expf without the max subtraction, an exact one-hot routing that
pins the query / key index layout without a tolerance, batch invariance, the
train path's composition of the same operator (ertd_gemm_small,
ertd_softmax_rows, ertd_gemm_small with unet_train_forward's strides), and the
shape guards.

Gate: rel-L2 < 1e-5 (the project's fp32 operator gate).  torch's own fp32
composition on the CPU sits at 3.7e-6 (C = 256) / 3.5e-6 (C = 512) from float64
at s = 6 and at 3e-7 at s = 0.5, so the gate leaves about 2.7x over a plain fp32
evaluation."""
import ctypes
import math

import pytest
import torch

from ertdiff import _lib
from ertdiff.unet import attention, make_config
from oracle import ref_numpy as RN
from conftest import record_error

pytestmark = pytest.mark.gpu
GATE = 1e-5
N = 256


def _rel(a, b):
    return RN.rel_l2(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())


def _qkv(B, C, s, seed=16):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B, 3 * C, N), generator=g).float()
    qkv[:, :2 * C] *= s
    return qkv


def _ref64(qkv):
    """float64 composition; also returns P (B, N, N) for the regime figures."""
    C = qkv.shape[1] // 3
    q, k, v = (qkv[:, i * C:(i + 1) * C].double() for i in range(3))
    logits = torch.einsum("bci,bcj->bij", q, k) / math.sqrt(C)
    P = torch.softmax(logits, dim=-1)
    return torch.einsum("bij,bcj->bci", P, v), P, logits


_CACHE = {}


def _case(B, C, s):
    """(qkv, float64 reference, P, logits), computed once per case and shared."""
    key = (B, C, s)
    if key not in _CACHE:
        qkv = _qkv(B, C, s)
        _CACHE[key] = (qkv,) + _ref64(qkv)
    return _CACHE[key]


@pytest.mark.parametrize("s", [0.5, 6.0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [256, 512])
def test_attention_peaked_softmax(C, B, s, cuda_dev):
    qkv, ref, P, logits = _case(B, C, s)
    if s == 6.0:
        # the regime the case is for: expf(logit) alone overflows, rows are peaked
        assert float(logits.max()) > 100.0
        assert float(P.max(dim=-1).values.mean()) > 0.8
    out = attention(qkv.to(cuda_dev))
    assert bool(torch.isfinite(out).all())
    err = _rel(out, ref)
    record_error(f"attention_C{C}_B{B}_s{s}", err)
    assert err < GATE, err


def test_attention_one_hot_routing_exact(cuda_dev):
    """q = a I, k[c][j] = a [c == pi^-1(j)], a^2 / 16 = 200: query i's logits are
    200 at key pi(i) and 0 elsewhere, every off-target probability is
    exp(-200) = 0 in fp32, so out[b, :, i] == v[b, :, pi(i)] bit for bit."""
    B, C = 2, 256
    a = math.sqrt(200.0 * 16.0)
    idx = torch.arange(N)
    pi = (37 * idx + 11) % N                   # a permutation: gcd(37, 256) = 1
    assert torch.equal(torch.sort(pi).values, idx)
    q = a * torch.eye(C, N)
    k = torch.zeros(C, N)
    k[idx, pi] = a                             # k[c][pi(c)] = a  <=>  k[c][j] = a [c == pi^-1(j)]
    g = torch.Generator().manual_seed(17)
    v = torch.randn((B, C, N), generator=g).float()
    qkv = torch.cat([q.expand(B, C, N), k.expand(B, C, N), v], 1).contiguous()
    out = attention(qkv.to(cuda_dev)).cpu()
    assert torch.equal(out, v[:, :, pi])


@pytest.mark.parametrize("C", [256, 512])
def test_attention_batch_invariance(C, cuda_dev):
    qkv = _case(3, C, 6.0)[0].to(cuda_dev)
    full = attention(qkv)
    for b in range(3):
        assert torch.equal(full[b:b + 1], attention(qkv[b:b + 1].contiguous())), b


@pytest.mark.parametrize("s", [0.5, 6.0])
@pytest.mark.parametrize("C", [256, 512])
def test_attention_train_composition_same_spec(C, s, cuda_dev):
    """The train path's attention (unet_train_forward: S = q^T k by
    ertd_gemm_small, ertd_softmax_rows, O = v P^T by ertd_gemm_small, with its
    strides) and the inference kernel are two implementations of one spec: both
    within the gate of float64."""
    B = 3
    qkv, ref, _, _ = _case(B, C, s)
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    d = qkv.to(cuda_dev).view(B, 3, C, N)
    q, k, v = d[:, 0], d[:, 1], d[:, 2]
    S = torch.empty(B, N, N, device=cuda_dev)
    assert lib.ertd_gemm_small(q.data_ptr(), 1, N, 3 * C * N, k.data_ptr(), N, 1, 3 * C * N,
                               S.data_ptr(), N, 1, N * N, None, N, N, C, B, 1.0, 0, st) == 0
    P = torch.empty_like(S)
    assert lib.ertd_softmax_rows(S.data_ptr(), B * N, N, 1.0 / math.sqrt(C), P.data_ptr(), st) == 0
    O = torch.empty(B, C, N, device=cuda_dev)
    assert lib.ertd_gemm_small(v.data_ptr(), N, 1, 3 * C * N, P.data_ptr(), 1, N, N * N,
                               O.data_ptr(), N, 1, C * N, None, C, N, N, B, 1.0, 0, st) == 0
    e_train = _rel(O, ref)
    e_inf = _rel(attention(qkv.to(cuda_dev)), ref)
    record_error(f"attention_train_composition_C{C}_s{s}", e_train)
    assert e_train < GATE and e_inf < GATE, (e_train, e_inf)


def test_attention_guards(cuda_dev):
    lib, st = _lib.lib(), _lib.stream_of(cuda_dev)
    buf = torch.zeros(3 * 512 * 512, device=cuda_dev)
    out = torch.zeros(512 * 512, device=cuda_dev)
    for n in (64, 128, 512):
        assert lib.ertd_attention(buf.data_ptr(), 1, 256, n, out.data_ptr(), st) == _lib.ERTD_EINVAL, n
    for c in (128, 384):
        assert lib.ertd_attention(buf.data_ptr(), 1, c, 256, out.data_ptr(), st) == _lib.ERTD_EINVAL, c
    assert lib.ertd_attention(buf.data_ptr(), 1, 256, 256, out.data_ptr(), st) == 0
    # an attn config needs a 16x16 mid resolution (the kernel's N = 256)
    ok = make_config(image=64, ch=64, ch_mult=(1, 2, 4), attn=True)
    assert lib.ertd_unet_n_params(ctypes.byref(ok)) > 0
    for bad in (make_config(image=64, ch=128, ch_mult=(1, 2), attn=True),        # 32x32 mid
                make_config(image=128, ch=64, ch_mult=(1, 2, 4), attn=True)):    # 32x32 mid
        assert lib.ertd_unet_n_params(ctypes.byref(bad)) == _lib.ERTD_EINVAL
    # the same networks without attention are accepted
    assert lib.ertd_unet_n_params(ctypes.byref(make_config(image=64, ch=128, ch_mult=(1, 2)))) > 0
