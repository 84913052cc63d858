"""The persistent fp32 conv kernels where their work items do not divide the grid.

conv_wino4s_kernel (F4S, F4S_UP), conv_wino4_kernel (F4), conv_wino_kernel
(F2) and the skip GEMM launch one workgroup per CU (or a few) that walks
items bid, bid + G, ...  A workgroup carries state across its item boundaries
(the producers' prefetch of the next item's first chunk, the xi halves'
exchange buffer, the GroupNorm table indexed by the local item number, the
skip GEMM's chunk ring), and with items > G, items % G != 0 neighbouring
workgroups run different numbers of items: some have a next item, some do not.
The batch that produces this walk depends on the CU count, so every case asks
the library's route query (ertdiff.unet.conv2d_route) for the smallest such
B, and starts by asserting from the query that the call runs the kernel, the
K split and the ragged walk it is about.

Three checks per case:
  accuracy    rel-L2 of EVERY sample alone against float64 torch (GroupNorm,
              SiLU, conv, bias, ebias, residual in float64); the worst sample
              < 1e-5, the fp32 conv gate -- one bad item among hundreds is not
              diluted by the batch norm;
  placement   the same batch with its samples rolled by B // 2 + 1: B and so
              the route are unchanged, every sample moves to another item,
              round and workgroup, and its bits must not change (torch.equal);
  sentinel    the output is followed in its allocation by 4096 words
              0x7FC0DEAD: a workgroup that runs an item too many writes there.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ertdiff.unet import conv2d
from conftest import record_error
from dirty_state import check_sentinel, sentinel_empty
from ragged_route import Shape, assert_ragged, find_B, ragged_B, route

pytestmark = pytest.mark.gpu

_ragged_B = ragged_B
CONV_TOL = 1e-5   # the fp32 conv gate (test_gpu_unet_ops.py), here per sample


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _operands(sh: Shape, B: int, seed: int):
    """The Gaussian operands of test_gpu_unet_ops.py's conv tests, always with a bias."""
    Cin = sh.Ca + sh.Cb
    Ho = 2 * sh.H if sh.mode == "up" else sh.H
    o = {"x": _rand((B, sh.Ca, sh.H, sh.H), seed),
         "x2": _rand((B, sh.Cb, sh.H, sh.H), seed + 1) if sh.Cb else None,
         "w": _rand((sh.Cout, Cin, sh.ks, sh.ks), seed + 2, 1.0 / np.sqrt(Cin * sh.ks * sh.ks)),
         "b": _rand((sh.Cout,), seed + 3, 0.1), "gn": None,
         "ebias": _rand((B, sh.Cout), seed + 6) if sh.ebias else None,
         "res": _rand((B, sh.Cout, Ho, Ho), seed + 7) if sh.res else None}
    if sh.act != "none":
        o["gn"] = torch.stack([_rand((B, Cin), seed + 4, 0.3) + 1.0, _rand((B, Cin), seed + 5, 0.2)], -1)
    return o


def _ref64(sh: Shape, o):
    x = (o["x"] if o["x2"] is None else torch.cat([o["x"], o["x2"]], 1)).double()
    if sh.act != "none":
        gn = o["gn"].double()
        x = x * gn[..., 0][:, :, None, None] + gn[..., 1][:, :, None, None]
        if sh.act == "gn_silu":
            x = F.silu(x)
    if sh.mode == "up":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, o["w"].double(), o["b"].double(), padding=sh.ks // 2)
    if o["ebias"] is not None:
        y = y + o["ebias"].double()[:, :, None, None]
    if o["res"] is not None:
        y = y + o["res"].double()
    return y


def _per_sample_err(out, ref):
    d = (out.double() - ref).flatten(1).norm(dim=1)
    return d / ref.flatten(1).norm(dim=1)


BATCHED = ("x", "x2", "gn", "ebias", "res")


def _run(sh: Shape, o, dev, roll=0):
    """conv2d into a sentinel-tailed output; roll: every per-sample operand rolled along the batch."""
    d = {}
    for k, v in o.items():
        if v is not None and roll and k in BATCHED:
            v = torch.roll(v, roll, 0)
        d[k] = None if v is None else v.to(dev)
    B = o["x"].shape[0]
    Ho = 2 * sh.H if sh.mode == "up" else sh.H
    out = sentinel_empty((B, sh.Cout, Ho, Ho), device=dev, name="out")
    got = conv2d(d["x"], d["w"], d["b"], mode=sh.mode, act=sh.act, gn=d["gn"], x2=d["x2"], ebias=d["ebias"],
                 res=d["res"], out=out)
    assert got is out
    torch.cuda.synchronize(dev)
    check_sentinel(out)
    return out.cpu()


def _check(case: str, sh: Shape, B: int, r, dev, seed: int):
    o = _operands(sh, B, seed)
    out = _run(sh, o, dev)
    err = _per_sample_err(out, _ref64(sh, o))
    worst = float(err.max())
    record_error(f"conv_ragged_{case}_{r.kernel}_ks{r.ksplit}_B{B}_{r.items}x{r.grid}", worst)
    print(f"{case}: B={B} {r} worst per-sample rel-L2 {worst:.3e} (sample {int(err.argmax())})")
    assert worst < CONV_TOL, (worst, int(err.argmax()))
    # placement invariance: rolled by k, sample b sits at (b + k) % B -- another item, round and workgroup
    k = B // 2 + 1
    back = torch.roll(_run(sh, o, dev, roll=k), -k, 0)
    if not torch.equal(back, out):
        bad = (back != out).flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{case}: {len(bad)} of {B} samples change bits with their position in the batch "
                             f"(first: {bad[:8]}), max abs diff {float((back - out).abs().max()):.3e}")


GN = dict(act="gn_silu")
# case -> (shape, kernel, ksplit, min_rounds); B and the geometry in the comments: 256 CUs
RAGGED = {
    "a_f4s_xcd": (Shape(64, 0, 64, 64, ebias=True, res=True, **GN), "f4s", 1, 2),       # B 17: 272 items, nloc 2 / 1
    "b_f4s_3rounds": (Shape(64, 0, 64, 64, ebias=True, res=True, **GN), "f4s", 1, 3),   # B 33: 528 items
    "c_f4s_ncog2_concat": (Shape(32, 32, 128, 32, res=True, **GN), "f4s", 1, 2),        # B 33: 264 items
    "d_f4s_none": (Shape(64, 0, 64, 32, act="none"), "f4s", 1, 2),                      # B 65: 260 items
    "d_f4s_gn": (Shape(64, 0, 64, 32, act="gn"), "f4s", 1, 2),
    "e_f4s_16_unsplit": (Shape(64, 0, 256, 16, **GN), "f4s", 1, 2),                     # B 65: 260 items, ncog 4
    "f_f4s_16_ksplit": (Shape(64, 0, 256, 16, ebias=True, res=True, **GN), "f4s", 2, 2),   # B 33: 264 half-items
    "g_f4s_up": (Shape(64, 0, 64, 16, mode="up", res=True), "f4s_up", 1, 2),            # B 65: 260 items
    "h_f4_128": (Shape(16, 0, 64, 128, **GN), "f4", 1, 2),                              # B 9: 288 items
    "i_f4_128_ksplit": (Shape(16, 0, 64, 128, **GN), "f4", 2, 2),                       # B 5: 320 half-items
    "j_f4_16_two_samples": (Shape(12, 0, 256, 16, **GN), "f4", 1, 2),                   # B 130: 260 items
    "k_f2": (Shape(16, 8, 64, 16), "f2", 1, 2),                                         # expected: no B reaches it
    "k_f2_ksplit": (Shape(32, 0, 64, 16), "f2", 2, 2),
    "l_skip_split_64x256": (Shape(128, 64, 64, 64, ks=1), "skip_gemm_split", 1, 2),
    "m_skip_split_128x128": (Shape(256, 256, 256, 16, ks=1, res=True), "skip_gemm_split", 1, 2),
}


@pytest.mark.parametrize("case", list(RAGGED))
def test_conv2d_ragged(case, cuda_dev):
    sh, kernel, ksplit, min_rounds = RAGGED[case]
    B = _ragged_B(sh, kernel, ksplit, min_rounds, device=cuda_dev)
    r = route(sh, B, cuda_dev)
    assert_ragged(r, kernel, ksplit, min_rounds)
    if case.startswith("j_"):
        assert B % 2 == 0   # a 32-tile block holds two samples
    _check(case, sh, B, r, cuda_dev, seed=100 + 10 * list(RAGGED).index(case))


def test_conv2d_f4s_grid_not_multiple_of_8(cuda_dev):
    """The XCD remap bid = (blockIdx % 8) (G / 8) + blockIdx / 8 is a permutation
    only for G % 8 == 0 and is taken only then: a grid of fewer workgroups than
    CUs that is no multiple of 8 (64 -> 64 at 32x32, B = 3: 12 items) must take
    the plain order."""
    sh = Shape(64, 0, 64, 32, ebias=True, res=True, **GN)
    cus = torch.cuda.get_device_properties(cuda_dev).multi_processor_count
    B = find_B(sh, lambda r: r.kernel == "f4s" and r.ksplit == 1 and r.items < cus and r.items % 8 != 0 and
               r.items > 8, cuda_dev, b_min=2)
    if B is None:
        pytest.skip("no B <= 192 gives f4s a grid below the CU count that is no multiple of 8")
    r = route(sh, B, cuda_dev)
    assert r.kernel == "f4s" and r.ksplit == 1 and r.grid == r.items < cus and r.grid % 8 != 0, r
    _check("f4s_grid_mod8", sh, B, r, cuda_dev, seed=400)


def test_conv2d_f4_16x16_two_samples_exact(cuda_dev):
    """F4 at 16x16 (Cin % 8 == 4, even B, B / 2 * Cout / 64 >= CUs), where one
    32-tile block holds two samples (TS < 32: per-lane sample offsets, the
    GroupNorm row of sample cur_b + (t >= TS)), in the plain situation: items an
    exact multiple of the grid."""
    sh = RAGGED["j_f4_16_two_samples"][0]
    B = find_B(sh, lambda r: r.kernel == "f4" and r.ksplit == 1 and r.grid > 0 and r.items % r.grid == 0, cuda_dev)
    if B is None:
        pytest.skip("no B <= 192 runs f4 at 16x16 with items a multiple of the grid")
    r = route(sh, B, cuda_dev)
    assert r.kernel == "f4" and r.ksplit == 1 and B % 2 == 0 and r.items == B // 2 * (sh.Cout // 64), r
    assert r.items >= r.grid > 0 and r.items % r.grid == 0, r
    _check("j_f4_16_exact", sh, B, r, cuda_dev, seed=500)
