"""The Upsample conv on the F(4x4) register-weight kernel with its own point set
and the 11 dead Winograd products skipped (conv_wino4s_kernel, UP, XS = 2).

Every case asks the library's route query for its batch (the smallest B that
runs f4s_up; Cin >= 16, so the xi-split kernel) and asserts the route first.
Per case, for inputs N(0, 1) and 1e3 + N(0, 1) (border and padding errors show
against the large mean):
  accuracy   rel-L2 of the worst single sample against a float64 conv of the
             upsampled input: below the suite's 1e-5, and at most 2x what the
             parent commit's kernel (all 36 products, points {0, 1, -1, 1/2,
             -2, inf}) gives on the same inputs.  The parent's figures are in
             tests/golden/up25_parent.json, recorded from the parent build:
                                           parent N(0,1) / 1e3+N    this kernel
               w16 (16->64, 8->16, B 256)  7.16e-7 / 1.32e-7              1.18e-6 / 1.28e-7
               w32 (32->128, 16->32)       5.74e-7 / 1.40e-7              8.85e-7 / 1.37e-7
               w64 (16->64, 32->64)        6.33e-7 / 1.18e-7              1.01e-6 / 1.15e-7
               w64 ragged                  4.49e-7 / 1.21e-7              6.99e-7 / 1.18e-7
  placement  the batch rolled: every sample's bits unchanged;
  sentinel   4096 words behind the output untouched;
  dirty      outputs and the workspace (exactly the queried size) come from an
             allocator that fills them with 0xFF: same bits as the clean run.
The route offers no K split for an Upsample conv (wino_route: it never splits),
so there is no such case.

A layer that is not an Upsample conv (64 -> 64 at 16x16, GroupNorm + SiLU) must
be bit-identical to the parent: its SHA-256 per sample is in the same golden.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ertdiff.unet import conv2d
from dirty_state import check_sentinel, dirty_allocator, sentinel_empty
from ragged_route import Shape, find_B, ragged_B, route

pytestmark = pytest.mark.gpu

CONV_TOL = 1e-5
PARENT_FACTOR = 2.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "up25_parent.json")

# case -> (shape, ragged)
CASES = {
    "w16": (Shape(16, 0, 64, 8, mode="up"), False),
    "w32": (Shape(32, 0, 128, 16, mode="up", res=True), False),
    "w64": (Shape(16, 0, 64, 32, mode="up"), False),
    "w64_ragged": (Shape(16, 0, 64, 32, mode="up", res=True), True),
}
NONUP = Shape(64, 0, 64, 16, act="gn_silu", ebias=True, res=True)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def find_B_up(sh, dev, b_max=512):
    """The smallest B that routes sh to f4s_up (ragged_route.find_B stops at 192; 16x16 needs 256)."""
    for B in range(1, b_max + 1):
        try:
            if route(sh, B, dev).kernel == "f4s_up":
                return B
        except RuntimeError:   # a geometry the entry rejects at this B
            continue
    return None


def operands(sh, B, seed, offset):
    Cin = sh.Ca + sh.Cb
    Ho = 2 * sh.H if sh.mode == "up" else sh.H
    o = {"x": _rand((B, sh.Ca, sh.H, sh.H), seed) + offset,
         "w": _rand((sh.Cout, Cin, 3, 3), seed + 2, 1.0 / np.sqrt(Cin * 9)),
         "b": _rand((sh.Cout,), seed + 3, 0.1), "gn": None,
         "ebias": _rand((B, sh.Cout), seed + 6) if sh.ebias else None,
         "res": _rand((B, sh.Cout, Ho, Ho), seed + 7) if sh.res else None}
    if sh.act != "none":
        o["gn"] = torch.stack([_rand((B, Cin), seed + 4, 0.3) + 1.0, _rand((B, Cin), seed + 5, 0.2)], -1)
    return o


def ref64(sh, o):
    x = o["x"].double()
    if sh.mode == "up":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, o["w"].double(), o["b"].double(), padding=1)
    if o["res"] is not None:
        y = y + o["res"].double()
    return y


def run(sh, o, dev, roll=0):
    d = {}
    for k, v in o.items():
        if v is not None and roll and k in ("x", "gn", "ebias", "res"):
            v = torch.roll(v, roll, 0)
        d[k] = None if v is None else v.to(dev)
    B = o["x"].shape[0]
    Ho = 2 * sh.H if sh.mode == "up" else sh.H
    out = sentinel_empty((B, sh.Cout, Ho, Ho), device=dev, name="out")
    conv2d(d["x"], d["w"], d["b"], mode=sh.mode, act=sh.act, gn=d["gn"], ebias=d["ebias"], res=d["res"], out=out)
    torch.cuda.synchronize(dev)
    check_sentinel(out)
    return out.cpu()


def worst_err(out, ref):
    e = (out.double() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    return float(e.max())


def up_B(case, dev):
    sh, ragged = CASES[case]
    B = ragged_B(sh, "f4s_up", device=dev) if ragged else find_B_up(sh, dev)
    assert B is not None, f"{case}: no batch routes {tuple(sh)} to f4s_up"
    r = route(sh, B, dev)
    assert r.kernel == "f4s_up" and r.ksplit == 1 and sh.Ca >= 16, r
    if ragged:
        assert r.items > r.grid > 0 and r.items % r.grid != 0, r
    return B, r


def measure(case, dev):
    """{'B', 'n01', 'off1e3'}: the case's batch and worst per-sample rel-L2 for both inputs."""
    sh, _ = CASES[case]
    B, _ = up_B(case, dev)
    res = {"B": B}
    for key, offset in (("n01", 0.0), ("off1e3", 1e3)):
        o = operands(sh, B, 700 + 10 * list(CASES).index(case), offset)
        res[key] = worst_err(run(sh, o, dev), ref64(sh, o))
    return res


def nonup_hashes(dev, B):
    o = operands(NONUP, B, 900, 0.0)
    out = run(NONUP, o, dev)
    return [hashlib.sha256(out[b].numpy().tobytes()).hexdigest() for b in range(B)]


def nonup_B(dev):
    return find_B(NONUP, lambda r: r.kernel == "f4s", dev, b_min=1)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_up25_accuracy_against_parent(case, golden, cuda_dev):
    got = measure(case, cuda_dev)
    par = golden["cases"][case]
    print(f"{case}: B={got['B']} N(0,1) {got['n01']:.3e} (parent {par['n01']:.3e}), "
          f"1e3+N(0,1) {got['off1e3']:.3e} (parent {par['off1e3']:.3e})")
    for key in ("n01", "off1e3"):
        assert got[key] < CONV_TOL, (key, got[key])
        assert got[key] <= PARENT_FACTOR * par[key], (key, got[key], par[key])


@pytest.mark.parametrize("case", list(CASES))
def test_up25_placement_and_dirty_memory(case, cuda_dev):
    sh, _ = CASES[case]
    B, _ = up_B(case, cuda_dev)
    for offset in (0.0, 1e3):
        o = operands(sh, B, 800 + 10 * list(CASES).index(case), offset)
        out = run(sh, o, cuda_dev)
        assert torch.isfinite(out).all()
        k = B // 2 + 1
        back = torch.roll(run(sh, o, cuda_dev, roll=k), -k, 0)
        assert torch.equal(back, out), f"{case}: bits change with the sample's position in the batch"
        with dirty_allocator():
            dirty = run(sh, o, cuda_dev)
        assert torch.equal(dirty, out), f"{case}: bits change on 0xFF-filled output / workspace memory"


def test_non_upsample_layer_is_bit_identical_to_parent(golden, cuda_dev):
    B = golden["nonup"]["B"]
    r = route(NONUP, B, cuda_dev)
    assert r.kernel == "f4s", r
    got = nonup_hashes(cuda_dev, B)
    assert got == golden["nonup"]["sha256"]
