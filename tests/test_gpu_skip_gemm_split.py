"""The 1x1 skip convs on bf16 MFMAs with three-way split operands
(unet_skip_gemm.hip, skip_gemm_split_kernel), through the public conv2d op
against F.conv2d in float64.

Yardstick: torch's CPU fp32 F.conv2d on the same inputs.  The kernel keeps six
of the nine cross products of (h + m + l)(h + m + l) -- every term above 2^-24
relative -- and accumulates in fp32, so its rel-L2 error has to stay within
2 x the fp32 conv's own (the factor is headroom for the MFMA's in-chunk
summation order; a two-plane hi/lo kernel lands at about 15 x).  The project's
absolute bound of 1e-5 holds as well.

Non-finite inputs: the planes of inf are (inf, nan, nan), so an output that
fp32 arithmetic gives as inf can come out as NaN; finite outputs are
unaffected (the tile's other rows and columns never see the value)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ertdiff.unet import conv2d
from oracle import ref_numpy as RN

pytestmark = pytest.mark.gpu


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _inputs(Ca, Cb, Cout, H, B, seed=0):
    x = _rand((B, Ca, H, H), 900 + seed)
    x2 = _rand((B, Cb, H, H), 901 + seed) if Cb else None
    w = _rand((Cout, Ca + Cb, 1, 1), 902 + seed, 1.0 / np.sqrt(Ca + Cb))
    b = _rand((Cout,), 903 + seed, 0.1)
    return x, x2, w, b


def _gpu(x, x2, w, b, dev, res=None):
    return conv2d(x.to(dev), w.to(dev), b.to(dev), x2=None if x2 is None else x2.to(dev),
                  res=None if res is None else res.to(dev)).cpu()


def _check(out, x, x2, w, b, res=None, mask=None):
    """rel-L2 of out and of torch's CPU fp32 conv against float64; asserts
    out <= 2 x fp32 and out < 1e-5 (over mask where given)."""
    xin = x if x2 is None else torch.cat([x, x2], 1)
    ref = F.conv2d(xin.double(), w.double(), b.double())
    f32 = F.conv2d(xin, w, b)
    if res is not None:
        ref = ref + res.double()
        f32 = f32 + res
    o, f, r = out.double().numpy(), f32.double().numpy(), ref.numpy()
    if mask is not None:
        o, f, r = o[mask], f[mask], r[mask]
    err, err32 = RN.rel_l2(o, r), RN.rel_l2(f, r)
    print(f"split rel-L2 {err:.3e}  fp32 cpu rel-L2 {err32:.3e}  ratio {err / err32:.2f}")
    assert err <= 2 * err32, (err, err32)
    assert err < 1e-5, err
    return ref


SHAPES = [  # (Ca, Cb, Cout, H, B)
    (32, 0, 64, 16, 1),        # one chunk, one 64 x 256 tile
    (64, 0, 128, 16, 2),       # 128 x 128 tiles
    (96, 32, 128, 16, 3),      # concat boundary inside a chunk, odd B
    (128, 64, 64, 64, 2),      # the Cout = 64 tile at 64 x 64, concat
    (256, 256, 256, 16, 2),    # K = 512
    (64, 64, 192, 32, 2),      # Cout not a multiple of 128: 64 x 256 tiles
]


@pytest.mark.parametrize("Ca,Cb,Cout,H,B", SHAPES)
def test_split_accuracy(Ca, Cb, Cout, H, B, cuda_dev):
    x, x2, w, b = _inputs(Ca, Cb, Cout, H, B)
    _check(_gpu(x, x2, w, b, cuda_dev), x, x2, w, b)


def test_split_planes_carry_weight(cuda_dev):
    """Inputs whose m and l planes are non-zero everywhere: channel c scaled by
    2^((c mod 9) - 4) (1 + 2^-9), weights by 1 + 2^-10."""
    Ca, Cb, Cout, H, B = 64, 0, 128, 16, 2
    x, x2, w, b = _inputs(Ca, Cb, Cout, H, B, seed=10)
    c = torch.arange(Ca)
    x = x * (torch.pow(2.0, (c % 9 - 4).float()) * (1 + 2.0 ** -9))[None, :, None, None]
    w = w * (1 + 2.0 ** -10)
    _check(_gpu(x, x2, w, b, cuda_dev), x, x2, w, b)


def test_split_batch_invariance_bitwise(cuda_dev):
    Ca, Cb, Cout, H = 128, 64, 128, 32
    x, x2, w, b = _inputs(Ca, Cb, Cout, H, 5, seed=20)
    o5 = _gpu(x, x2, w, b, cuda_dev)
    o1 = _gpu(x[:1].contiguous(), x2[:1].contiguous(), w, b, cuda_dev)
    assert torch.equal(o1[0], o5[0])


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_split_residual_and_bias(with_res, with_bias, cuda_dev):
    Ca, Cb, Cout, H, B = 64, 32, 128, 16, 2
    x, x2, w, b = _inputs(Ca, Cb, Cout, H, B, seed=30)
    if not with_bias:
        b = torch.zeros_like(b)
    res = _rand((B, Cout, H, H), 934) if with_res else None
    _check(_gpu(x, x2, w, b, cuda_dev, res=res), x, x2, w, b, res=res)


def test_split_nonfinite_stays_local(cuda_dev):
    Ca, Cb, Cout, H, B = 64, 0, 128, 16, 1
    x, x2, w, b = _inputs(Ca, Cb, Cout, H, B, seed=40)
    x[0, 5, 3, 7] = float("inf")
    x[0, 40, 11, 2] = float("nan")
    out = _gpu(x, x2, w, b, cuda_dev)
    ref = F.conv2d(x.double(), w.double(), b.double())
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(out), fin)
    assert int((~fin).sum()) == 2 * Cout
    _check(out, x, x2, w, b, mask=fin.numpy())
