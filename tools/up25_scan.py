#!/usr/bin/env python3
"""Scan of F(4x4,3x3) point sets {0, 1, p, t, -t, inf} for the Upsample conv (CPU, NumPy).

For each (t, p): is the B^T row of p exactly 0 on x2-replicated windows, and
the rel-L2 of an fp32 emulation (transform, accumulation over Cin channels and
output transform in float32, U rounded once from float64) against a float64
conv, on random data -- all 36 products for the project's points, the 25 live
ones for the vanishing-row sets.  The committed choice is ertdiff.wino_up.UP_POINTS.

    python tools/up25_scan.py [--cin 128] [--tiles 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "ert-conditional-diffusion-model_amd", "ertdiff"))
import wino_up as W   # noqa: E402  (no torch needed)


def emulate(points, dead, cin, tiles, rng):
    AT, G, BT = W.cook_toom(points)
    f = np.float32
    src = rng.standard_normal((tiles, cin, 4, 4)).astype(f)
    d = W.up_window(src)
    g = rng.standard_normal((cin, 3, 3)) / np.sqrt(9 * cin)
    U = np.einsum("ia,cab,jb->cij", G, g, G).astype(f)
    BTf, ATf = BT.astype(f), AT.astype(f)
    V = np.einsum("ia,tcab,jb->tcij", BTf, d, BTf, optimize=False).astype(f)
    # the dead row is 0 on the replication pattern (a, b, b, c, c, d) for every input: exact in the
    # matrix; the kernel's operation order (wino_up.bt6u_f32) keeps it an exact 0.0 in fp32 as well
    rep = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    zero_row = dead is not None and bool(np.all(BT[dead] @ rep == 0))
    live = np.ones((6, 6), dtype=f)
    if dead is not None:
        live[dead] = 0
        live[:, dead] = 0
    M = np.zeros((tiles, 6, 6), dtype=f)
    for c in range(cin):
        M = (M + U[c] * V[:, c] * live).astype(f)
    Y = np.einsum("ri,tij,xj->trx", ATf, M, ATf).astype(f)
    ref = np.array([[[(d[t, :, r:r + 3, x:x + 3].astype(np.float64) * g).sum() for x in range(4)]
                     for r in range(4)] for t in range(tiles)])
    return zero_row, np.linalg.norm(Y - ref) / np.linalg.norm(ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cin", type=int, default=128)
    ap.add_argument("--tiles", type=int, default=64)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    z, e = emulate(W.PROJECT_POINTS, None, a.cin, a.tiles, rng)
    print(f"project points {W.PROJECT_POINTS} + inf, 36 products: rel-L2 {e:.2e}")
    for t in (0.5, 2.0, 0.25, 4.0, 1.5):
        for p in (-1.0,):
            pts = (0.0, 1.0, t, -t, p)
            z, e = emulate(pts, 4, a.cin, a.tiles, np.random.default_rng(0))
            print(f"t = {t:<5} p = {p:<5} dead row exactly 0: {z}   25 products: rel-L2 {e:.2e}")


if __name__ == "__main__":
    main()
