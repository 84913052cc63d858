"""The Upsample conv's Winograd F(4x4,3x3) point set and its Cook-Toom matrices.

An Upsample conv is a 3x3 conv of a nearest-x2 image: a 6-wide window of it is
(a, b, b, c, c, d).  The B^T row of a finite non-zero point p is the coefficient
vector of x * prod(x - q) over the other three finite non-zero points q; for
q = {1, t, -t} that is [0, t^2, -t^2, -1, 1, 0], which is 0 on every such
window.  With the points below (t = 1/2, p = -1) row 4 and column 4 of
V = B^T d B vanish for every tile: 11 of the 36 Winograd-domain products are
products with exact zeros, and csrc/unet_conv_wino4s.hip skips them.

The kernel's bt6u / at6u and the pack's GD_UP are these matrices; NumPy only.
"""
from __future__ import annotations

import numpy as np

# index order of the kernel: xi = 6 * row + column; index 5 is the point at infinity
UP_POINTS = (0.0, 1.0, 0.5, -0.5, -1.0)
UP_DEAD = 4                      # the index of p = -1: the vanishing row / column
PROJECT_POINTS = (0.0, 1.0, -1.0, 0.5, -2.0)   # every other F(4x4) layer


def cook_toom(points, row0_scale=None):
    """(AT 4x6, G 6x3, BT 6x6) in float64 for F(4,3) on 5 finite points + infinity:
    y = AT [(G g) * (BT d)].  BT rows are the monic M_i(x) = prod_{j != i}(x - a_j)
    (row 5: prod_j (x - a_j)), G rows a_i^k / M_i(a_i); row 0 of BT is scaled to a
    constant term of 1 (G row 0 = [1, 0, 0]) as the kernels write it."""
    a = np.asarray(points, dtype=np.float64)
    n = len(a)
    AT = np.zeros((4, n + 1))
    G = np.zeros((n + 1, 3))
    BT = np.zeros((n + 1, n + 1))
    for i in range(n):
        others = np.delete(a, i)
        m = np.poly(others)[::-1]            # ascending coefficients, degree n - 1
        N = np.prod(a[i] - others)
        s = 1.0
        if i == 0:
            s = (1.0 / m[0]) if row0_scale is None else row0_scale
        BT[i, :n] = m * s
        G[i] = a[i] ** np.arange(3) / (N * s)
        AT[:, i] = a[i] ** np.arange(4)
    BT[n] = np.poly(a)[::-1]
    G[n] = [0.0, 0.0, 1.0]
    AT[3, n] = 1.0
    return AT, G, BT


# the tables as written in the kernel (bt6u, at6u) and the pack (GD_UP)
BT_UP = np.array([[1, 0, -5, 0, 4, 0],
                  [0, -.25, -.25, 1, 1, 0],
                  [0, -.5, -1, .5, 1, 0],
                  [0, .5, -1, -.5, 1, 0],
                  [0, .25, -.25, -1, 1, 0],
                  [0, .25, 0, -1.25, 0, 1]], dtype=np.float64)
AT_UP = np.array([[1, 1, 1, 1, 1, 0],
                  [0, 1, .5, -.5, -1, 0],
                  [0, 1, .25, .25, 1, 0],
                  [0, 1, .125, -.125, -1, 1]], dtype=np.float64)
G_UP = np.array([[1, 0, 0],
                 [2 / 3, 2 / 3, 2 / 3],
                 [-8 / 3, -4 / 3, -2 / 3],
                 [-8 / 3, 4 / 3, -2 / 3],
                 [2 / 3, -2 / 3, 2 / 3],
                 [0, 0, 1]], dtype=np.float64)

_f = np.float32


def _fma(a, b, c):
    """fp32 fused multiply-add of float32 arrays (exact product in float64, one rounding)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(_f) \
        if np.isscalar(b) else (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_f)


def bt6u_f32(d):
    """The kernel's bt6u on float32 d[6, ...] (same operation order; row 4 computed)."""
    d = [np.asarray(x, dtype=_f) for x in d]
    c, e = d[4] - d[2], d[3] - d[1]
    return [_fma(d[4], 4.0, _fma(d[2], -5.0, d[0])),
            _fma(d[1] + d[2], -0.25, d[3] + d[4]),
            _fma(e, 0.5, c),
            _fma(e, -0.5, c),
            _fma(d[1] - d[2], 0.25, d[4] - d[3]),
            _fma(d[3], -1.25, _fma(d[1], 0.25, d[5]))]


def at6u_f32(m, dead=True):
    """The kernel's at6u on float32 m[6, ...]; dead=False adds m[4]'s column of A^T as well
    (the 36-product form)."""
    m = [np.asarray(x, dtype=_f) for x in m]
    s, d = m[2] + m[3], m[2] - m[3]
    y = [(m[0] + m[1]) + s, _fma(d, 0.5, m[1]), _fma(s, 0.25, m[1]), _fma(d, 0.125, m[1] + m[5])]
    if not dead:
        y = [y[0] + m[4], y[1] - m[4], y[2] + m[4], y[3] - m[4]]
    return y


def input_transform_f32(win):
    """V = B^T d B of float32 windows win[6, 6, ...] as the producers compute it: rows first."""
    rows = bt6u_f32([win[i] for i in range(6)])                  # [6 rows][6 cols, ...]
    V = [bt6u_f32([r[j] for j in range(6)]) for r in rows]        # V[i][j]
    return V


def conv_tile_f32(wins, U, live_only):
    """One 4x4 output tile in the fp32 emulation: wins (Cin, 6, 6) float32 windows, U
    (Cin, 6, 6) float32 transformed weights; fp32 accumulation over Cin in order.  live_only:
    the 25 products (dead row / column skipped); else all 36."""
    Cin = wins.shape[0]
    M = np.zeros((6, 6), dtype=_f)
    for c in range(Cin):
        V = input_transform_f32(wins[c])
        for i in range(6):
            for j in range(6):
                if live_only and (i == UP_DEAD or j == UP_DEAD):
                    continue
                M[i, j] = _fma(np.asarray(U[c, i, j], _f), np.asarray(V[i][j], _f), M[i, j])
    P = [at6u_f32([M[i, j] for j in range(6)], dead=live_only) for i in range(6)]   # P[i][x]
    Y = np.zeros((4, 4), dtype=_f)
    for x in range(4):
        col = at6u_f32([P[i][x] for i in range(6)], dead=live_only)
        for r in range(4):
            Y[r, x] = col[r]
    return Y


def up_window(src4):
    """The 6x6 window (.., 6, 6) of the nearest-x2 image over a (.., 4, 4) source patch."""
    m = [0, 1, 1, 2, 2, 3]
    return np.asarray(src4)[..., m, :][..., :, m]
