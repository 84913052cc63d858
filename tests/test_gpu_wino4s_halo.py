"""The register-weight F(4x4) conv's producers (unet_conv_wino4s.hip) where a
lane activates only its tile's four own rows and takes the two halo rows of
its window from the lanes of the tiles above and below (16x16: whole-sample
items, 32x32: two tile rows per item and one extra row from memory); 64x64
(one tile row per item) keeps the six-row path.

Driven through ertd_conv2d (3x3, stride 1, GroupNorm + SiLU, fp32) against a
float64 convolution on the CPU, rel-L2 < 1e-5 as tests/test_gpu_unet_ops.py:
a wrong, stale or misplaced halo row is an O(1) error.

At 16x16 the route takes this kernel only where its items fill the CUs, so
besides the small-batch 16x16 shapes (which the route hands to another
Winograd kernel) each of them also runs at B = CUs / co groups, where the
route is asserted to be "f4s"."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ertdiff.unet import conv2d, conv2d_route
from oracle import ref_numpy as RN
from conftest import record_error

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _ref(x, w, b, gn, eb=None, res=None):
    """float64: conv3x3(silu(x * scale + shift)) + bias (+ emb) (+ residual)"""
    x, w, b, gn = x.double(), w.double(), b.double(), gn.double()
    y = F.conv2d(F.silu(x * gn[..., 0][:, :, None, None] + gn[..., 1][:, :, None, None]), w, b, padding=1)
    if eb is not None:
        y = y + eb.double()[:, :, None, None]
    if res is not None:
        y = y + res.double()
    return y


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _run(dev, x, w, b, gn, x2=None, eb=None, res=None):
    d = lambda v: None if v is None else v.to(dev)
    return conv2d(d(x), d(w), d(b), act="gn_silu", gn=d(gn), x2=d(x2), ebias=d(eb), res=d(res)).cpu()


def _is_f4s(dev, Ca, Cb, Cout, B, H, eb=False, res=False):
    r = conv2d_route(Ca, Cb, Cout, 3, B, H, act="gn_silu", ebias=eb, res=res, device=dev)
    return r.kernel == "f4s" and r.ksplit == 1


# (H, B, Ca, Cb, Cout, emb + residual); B = 0: CUs / co groups (16x16 items fill the CUs)
SHAPES = [
    (16, 3, 16, 0, 64, False),     # whole-sample items: every halo from a neighbour lane, top / bottom padding
    (16, 2, 56, 0, 128, False),    # 7 chunks: one turn of the 6-slot register-set rotation plus a tail; 2 co groups
    (32, 2, 16, 0, 64, False),     # two tile rows per item: (0,1), (6,7) hit the padding, (2,3), (4,5) read both extras
    (32, 1, 8, 48, 128, True),     # concat split between chunks, emb bias and residual
    (64, 1, 16, 0, 64, False),     # one tile row per item: nothing to share, the six-row path
    (16, 0, 16, 0, 64, False),     # the first two where the 16x16 route is this kernel
    (16, 0, 56, 0, 128, False),
]


@pytest.mark.parametrize("H,B,Ca,Cb,Cout,ebres", SHAPES)
def test_wino4s_halo_shapes(H, B, Ca, Cb, Cout, ebres, cuda_dev):
    full = B == 0
    if full:
        B = _cus(cuda_dev) // (Cout // 64)
    if full or H != 16:
        assert _is_f4s(cuda_dev, Ca, Cb, Cout, B, H, ebres, ebres)
    Cin = Ca + Cb
    seed = 1000 * H + 10 * Cin + Cout // 64
    x = _rand((B, Ca, H, H), seed)
    x2 = _rand((B, Cb, H, H), seed + 1) if Cb else None
    w = _rand((Cout, Cin, 3, 3), seed + 2, 1.0 / np.sqrt(9 * Cin))
    b = _rand((Cout,), seed + 3, 0.1)
    gn = torch.stack([_rand((B, Cin), seed + 4, 0.3) + 1.0, _rand((B, Cin), seed + 5, 0.2)], -1)
    eb = _rand((B, Cout), seed + 6) if ebres else None
    res = _rand((B, Cout, H, H), seed + 7) if ebres else None
    out = _run(cuda_dev, x, w, b, gn, x2, eb, res)
    ref = _ref(x if x2 is None else torch.cat([x, x2], 1), w, b, gn, eb, res)
    err = RN.rel_l2(out.double().numpy(), ref.numpy())
    record_error(f"wino4s_halo_{H}_{B}_{Ca}_{Cb}_{Cout}", err)
    print(f"rel-L2 {err:.3e}")
    assert err < TOL, err


@pytest.mark.parametrize("r", [0, 3, 4, 7, 8, -1])
@pytest.mark.parametrize("H", [16, 32])
def test_wino4s_halo_impulse_row(H, r, cuda_dev):
    """Input zero except image row r, GroupNorm scale 1 and shift 0 (SiLU keeps
    the zeros): the output is non-zero in rows r - 1 .. r + 1 only, so a halo
    row that lands in the wrong window row, or a padded row that is not zero,
    shows in full."""
    Cin, Cout = 16, 64
    B = _cus(cuda_dev) if H == 16 else 2
    assert _is_f4s(cuda_dev, Cin, 0, Cout, B, H)
    row = r % H
    x = torch.zeros(B, Cin, H, H)
    x[:, :, row, :] = _rand((B, Cin, H), 7 * H + row)
    w = _rand((Cout, Cin, 3, 3), 11, 1.0 / np.sqrt(9 * Cin))
    b = torch.zeros(Cout)
    gn = torch.stack([torch.ones(B, Cin), torch.zeros(B, Cin)], -1)
    out = _run(cuda_dev, x, w, b, gn)
    ref = _ref(x, w, b, gn)
    err = RN.rel_l2(out.double().numpy(), ref.numpy())
    print(f"rel-L2 {err:.3e}")
    assert err < TOL, err
    # nothing outside the three rows the impulse reaches (the transforms' rounding aside)
    far = torch.ones(H, dtype=torch.bool)
    far[max(row - 1, 0):row + 2] = False
    assert out[:, :, far, :].abs().max().item() < 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("H", [16, 32, 64])
def test_wino4s_halo_sample_alone_bitwise(H, cuda_dev):
    """Sample b run alone (B = 1) equals sample b of the B = 3 call bit for bit:
    the arithmetic per element does not depend on the item a tile sits in."""
    Cin, Cout, B = 16, 64, 3
    if H != 16:
        assert _is_f4s(cuda_dev, Cin, 0, Cout, B, H) and _is_f4s(cuda_dev, Cin, 0, Cout, 1, H)
    x = _rand((B, Cin, H, H), 40 + H)
    w = _rand((Cout, Cin, 3, 3), 41, 1.0 / np.sqrt(9 * Cin))
    b = _rand((Cout,), 42, 0.1)
    gn = torch.stack([_rand((B, Cin), 43, 0.3) + 1.0, _rand((B, Cin), 44, 0.2)], -1)
    out = _run(cuda_dev, x, w, b, gn)
    for s in range(B):
        one = _run(cuda_dev, x[s:s + 1], w, b, gn[s:s + 1])
        assert torch.equal(one[0], out[s]), s


def test_wino4s_halo_16_rolled_batch_bitwise(cuda_dev):
    """16x16 at B = CUs (whole-sample items on this kernel): the batch rolled
    by one sample puts every sample into another workgroup, with the same bits."""
    Cin, Cout, H = 16, 64, 16
    B = _cus(cuda_dev)
    assert _is_f4s(cuda_dev, Cin, 0, Cout, B, H)
    x = _rand((B, Cin, H, H), 50)
    w = _rand((Cout, Cin, 3, 3), 51, 1.0 / np.sqrt(9 * Cin))
    b = _rand((Cout,), 52, 0.1)
    gn = torch.stack([_rand((B, Cin), 53, 0.3) + 1.0, _rand((B, Cin), 54, 0.2)], -1)
    out = _run(cuda_dev, x, w, b, gn)
    rolled = _run(cuda_dev, x.roll(1, 0), w, b, gn.roll(1, 0))
    assert torch.equal(rolled.roll(-1, 0), out)
