"""Batches at which a persistent conv kernel's work items do not divide its grid.

The fp32 Winograd convs and the skip GEMM are persistent: workgroup g of G
runs items g, g + G, ...; with items > G and items % G != 0 neighbouring
workgroups run different numbers of items.  Which batch produces that walk
depends on the device's CU count and on the dispatch, so the tests ask the
library (ertdiff.unet.conv2d_route, the dispatch's own functions) instead of
restating its rules.  Importing needs no GPU."""
from __future__ import annotations

import collections

import pytest

B_MAX = 192

# the geometry of one ertdiff.unet.conv2d call (H: the input size)
Shape = collections.namedtuple("Shape", "Ca Cb Cout H ks mode act ebias res", defaults=(3, "same", "none", False, False))


def route(shape: Shape, B: int, device=None):
    from ertdiff.unet import conv2d_route
    return conv2d_route(shape.Ca, shape.Cb, shape.Cout, shape.ks, B, shape.H, mode=shape.mode, act=shape.act,
                        ebias=shape.ebias, res=shape.res, device=device)


def rounds(r) -> int:
    return -(-r.items // r.grid) if r.grid else 0


def is_ragged(r, want_kernel, want_ksplit, min_rounds=2) -> bool:
    return (r.kernel == want_kernel and r.ksplit == want_ksplit and r.items > r.grid > 0 and
            r.items % r.grid != 0 and rounds(r) >= min_rounds)


def find_B(shape: Shape, pred, device=None, b_min: int = 1):
    """The smallest b_min <= B <= B_MAX whose route satisfies pred, or None."""
    for B in range(b_min, B_MAX + 1):
        try:
            r = route(shape, B, device)
        except RuntimeError:   # a geometry the entry rejects at this B
            continue
        if pred(r):
            return B
    return None


def ragged_B(shape: Shape, want_kernel: str, want_ksplit: int = 1, min_rounds: int = 2, device=None) -> int:
    """The smallest B <= 192 at which `shape` runs want_kernel with want_ksplit,
    items > grid, items % grid != 0 and at least min_rounds rounds; skips the
    calling test, naming the route, when no batch reaches it."""
    B = find_B(shape, lambda r: is_ragged(r, want_kernel, want_ksplit, min_rounds), device)
    if B is None:
        pytest.skip(f"no B <= {B_MAX} runs {want_kernel} (ksplit {want_ksplit}, >= {min_rounds} rounds) raggedly "
                    f"for {tuple(shape)} on this device: the route is unreachable with ragged items")
    return B


def assert_ragged(r, want_kernel, want_ksplit=1, min_rounds=2):
    """The precondition every ragged test states first, from the query."""
    assert r.kernel == want_kernel and r.ksplit == want_ksplit, r
    assert r.items > r.grid > 0 and r.items % r.grid != 0 and rounds(r) >= min_rounds, r
