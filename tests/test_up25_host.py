"""The Upsample conv's vanishing-row Winograd transforms, on the host (NumPy).

The matrices are derived from the committed points (ertdiff.wino_up.UP_POINTS)
by Cook-Toom and must equal the tables the kernel and the pack are written
from.  Then: the algorithm is a 3x3 conv of the x2-replicated patch (float64);
row 4 and column 4 of V are exactly 0.0 in fp32 for every finite input -- also
with a zeroed border row / column and with a large common offset; and skipping
the 11 dead products changes no bit of the fp32 emulation's output.
"""
import numpy as np
import pytest

from ertdiff import wino_up as W


def test_tables_are_cook_toom_of_the_points():
    AT, G, BT = W.cook_toom(W.UP_POINTS)
    assert np.array_equal(BT, W.BT_UP)
    assert np.array_equal(AT, W.AT_UP)
    assert np.allclose(G, W.G_UP, rtol=0, atol=1e-15)
    # the dead row: 0 on every (a, b, b, c, c, d), and it does not touch positions 0 and 5
    assert BT[W.UP_DEAD].tolist() == [0, .25, -.25, -1, 1, 0]
    # the project's points have no such row
    _, _, BTp = W.cook_toom(W.PROJECT_POINTS)
    e = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    assert (np.abs(BTp @ e).sum(1) > 0).all()
    assert np.flatnonzero(np.abs(BT @ e).sum(1) == 0).tolist() == [W.UP_DEAD]


def test_float64_algorithm_is_the_conv_of_the_replicated_patch():
    rng = np.random.default_rng(0)
    AT, G, BT = W.cook_toom(W.UP_POINTS)
    for _ in range(20):
        src = rng.standard_normal((4, 4))
        g = rng.standard_normal((3, 3))
        d = W.up_window(src)
        y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
        ref = np.array([[(d[r:r + 3, x:x + 3] * g).sum() for x in range(4)] for r in range(4)])
        assert np.abs(y - ref).max() < 1e-12
        # ... and with the dead row and column of the product dropped
        live = np.ones((6, 6)); live[W.UP_DEAD] = 0; live[:, W.UP_DEAD] = 0
        y25 = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T) * live) @ AT.T
        assert np.abs(y25 - ref).max() < 1e-12
        assert int(live.sum()) == 25


def _windows(rng, n, offset):
    src = (offset + rng.standard_normal((n, 4, 4))).astype(np.float32)
    return W.up_window(src)          # (n, 6, 6)


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("border", ["none", "row0", "row5", "col0", "col5", "corner"])
def test_dead_row_and_column_are_exact_zeros_in_fp32(offset, border):
    rng = np.random.default_rng(1)
    win = _windows(rng, 4096, offset).copy()
    if border in ("row0", "corner"):
        win[:, 0, :] = 0
    if border == "row5":
        win[:, 5, :] = 0
    if border in ("col0",):
        win[:, :, 0] = 0
    if border in ("col5", "corner"):
        win[:, :, 5] = 0
    V = W.input_transform_f32(np.moveaxis(win, 0, -1))     # V[i][j]: (n,)
    for k in range(6):
        assert np.all(V[W.UP_DEAD][k] == 0.0) and np.all(V[k][W.UP_DEAD] == 0.0)
    # (the live ones are not: the check above is not vacuous)
    assert all(np.any(V[i][j] != 0) for i in range(6) for j in range(6) if i != W.UP_DEAD and j != W.UP_DEAD)


@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_25_products_equal_36_bit_for_bit(offset):
    rng = np.random.default_rng(2)
    Cin = 16
    _, G, _ = W.cook_toom(W.UP_POINTS)
    for _ in range(6):
        wins = _windows(rng, Cin, offset)
        g = (rng.standard_normal((Cin, 3, 3)) / np.sqrt(9 * Cin))
        U = np.einsum("ia,cab,jb->cij", G, g, G).astype(np.float32)
        y25 = W.conv_tile_f32(wins, U, live_only=True)
        y36 = W.conv_tile_f32(wins, U, live_only=False)
        assert y25.tobytes() == y36.tobytes()
        ref = np.array([[(wins[:, r:r + 3, x:x + 3].astype(np.float64) * g).sum() for x in range(4)]
                        for r in range(4)])
        assert np.linalg.norm(y25 - ref) / np.linalg.norm(ref) < 1e-5
