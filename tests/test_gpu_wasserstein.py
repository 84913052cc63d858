"""Device row sort and Wasserstein-1 distance (csrc/rowsort.hip, ertdiff.stats)
against numpy and the scipy / sklearn fixture (tests/golden/wasserstein_kat.npz).

The sort is bitwise: np.array_equal against np.sort(x, axis=1).  The distance
is compared with the numpy restatement of scipy's _cdf_distance
(make_wasserstein_golden.wasserstein_numpy) at rtol 1e-12, the project's
float64 gate: the device's terms are scipy's bit for bit and non-negative, so
the two sums differ only in their order of addition, by at most (longest
chain + tree depth) * 2^-53 relative -- under 3e-13 for the device's chains
(at most 88 additions on any path) and for numpy's pairwise sum alike.  The
measured errors are recorded.  Row lengths are built from the kernel's tile T
(ertd_rows_sort_tile): one short tile, a full tile, one key more, several
runs with an odd one copied through, and the reference's 65,702."""
import numpy as np
import pytest
import torch

import ertdiff
from ertdiff import _lib
from conftest import load_golden, record_error
import make_wasserstein_golden as G

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
CODE = {"f32": 0, "f64": 1}
# (a, b): M = a * T + b
MS = [(0, 1), (0, 2), (0, 63), (0, 64), (0, 65), (0, 1000), (1, -1), (1, 0), (1, 1), (2, 0), (2, 1),
      (3, 0), (5, 7), (0, 65702)]
M_IDS = ["1", "2", "63", "64", "65", "1000", "T-1", "T", "T+1", "2T", "2T+1", "3T", "5T+7", "65702"]


@pytest.fixture(scope="module")
def kat():
    return load_golden("wasserstein_kat.npz")


@pytest.fixture(scope="module")
def tile(cuda_dev):
    lib = _lib.lib()
    t = {k: lib.ertd_rows_sort_tile(c) for k, c in CODE.items()}
    assert t["f32"] >= 1024 and t["f64"] >= 1024
    return t


def _inputs(n, M, dtype, seed):
    """name -> (n, M) rows: random, already sorted, reversed, and drawn from 5
    distinct values (long equal runs across tile and merge-chunk boundaries)."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, M)) * 10.0 ** rng.integers(-2, 3, size=(n, 1))).astype(dtype)
    s = np.sort(x, axis=1)
    five = rng.choice(np.array([-1.5, 0.0, 0.25, 3.0, 1e3]), size=(n, M)).astype(dtype)
    return {"random": x, "sorted": s, "reversed": s[:, ::-1].copy(), "five": five}


def _sorted_equal(x, dev, **kw):
    got = ertdiff.sort_rows(torch.from_numpy(x).to(dev))
    assert got.dtype == torch.from_numpy(x).dtype and tuple(got.shape) == x.shape
    return np.array_equal(got.cpu().numpy(), np.sort(x, axis=-1), **kw)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("m", MS, ids=M_IDS)
def test_sort_bitwise(m, dt, tile, cuda_dev):
    M = m[0] * tile[dt] + m[1]
    for name, x in _inputs(3, M, NP[dt], 17 * M + 1).items():
        assert _sorted_equal(x, cuda_dev), name


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(300, 1000), (1, (5, 7))], ids=["300x1000", "1x(5T+7)"])
def test_sort_many_rows_and_one_row(shape, dt, tile, cuda_dev):
    n, M = shape
    if isinstance(M, tuple):
        M = M[0] * tile[dt] + M[1]
    for name, x in _inputs(n, M, NP[dt], 5).items():
        assert _sorted_equal(x, cuda_dev), name


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_sort_strided_view_one_dim_and_numpy(dt, tile, cuda_dev):
    M = 2 * tile[dt] + 1
    big = _inputs(3, M + 13, NP[dt], 9)["random"]
    view = torch.from_numpy(big).to(cuda_dev)[:, 5:5 + M]          # ld = M + 13 > M
    assert not view.is_contiguous()
    got = ertdiff.sort_rows(view)
    assert np.array_equal(got.cpu().numpy(), np.sort(big[:, 5:5 + M], axis=1))
    one = ertdiff.sort_rows(big[0])                                 # numpy in, (M,) out
    assert tuple(one.shape) == (M + 13,) and np.array_equal(one.cpu().numpy(), np.sort(big[0]))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_sort_puts_nans_last(dt, tile, cuda_dev):
    T = tile[dt]
    M = 2 * T + 1
    x = _inputs(3, M, NP[dt], 21)["random"]
    x[1, [3, T + 5, 2 * T]] = np.nan                                # one per tile
    assert _sorted_equal(x, cuda_dev, equal_nan=True)
    got = ertdiff.sort_rows(torch.from_numpy(x).to(cuda_dev)).cpu().numpy()
    assert np.isnan(got[1, -3:]).all() and not np.isnan(got[1, :-3]).any()


def _check_distance(u, v, dev, name):
    got = ertdiff.wasserstein(torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev))
    assert got.dtype == torch.float64 and tuple(got.shape) == (u.shape[0],)
    want = np.array([G.wasserstein_numpy(r, v) for r in u])
    g = got.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want != 0, np.abs(g - want) / np.abs(want), np.abs(g))
    print(f"{name}: max rel err {rel.max():.3e}")
    record_error(f"wasserstein {name}", rel.max())
    np.testing.assert_allclose(g, want, rtol=1e-12, atol=0, err_msg=name)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("m", MS, ids=M_IDS)
def test_distance_equal_sizes(m, dt, tile, cuda_dev):
    M = m[0] * tile[dt] + m[1]
    ins = _inputs(4, M, NP[dt], 31 * M + 3)
    for kind in ("random", "five"):
        x = ins[kind]
        _check_distance(x[:3], x[3] + NP[dt](0.25 if kind == "random" else 0.0), cuda_dev,
                        f"{dt} M={M} {kind}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("sizes", [(0, 1500, 0, 1201), (1, 1, 0, 7), (0, 7, 2, 1)],
                         ids=["1500-1201", "T+1-7", "7-2T+1"])
def test_distance_unequal_sizes(sizes, dt, tile, cuda_dev):
    Nu = sizes[0] * tile[dt] + sizes[1]
    Nv = sizes[2] * tile[dt] + sizes[3]
    for kind in ("random", "five"):
        u = _inputs(3, Nu, NP[dt], 41)[kind]
        v = _inputs(1, Nv, NP[dt], 43)[kind][0]
        _check_distance(u, v, cuda_dev, f"{dt} {Nu}x{Nv} {kind}")


def test_distance_exact_cases(tile, cuda_dev):
    x = _inputs(3, tile["f64"] + 1, np.float64, 51)["random"]
    xd = torch.from_numpy(x).to(cuda_dev)
    d = ertdiff.wasserstein(xd, xd[0]).cpu().numpy()
    assert d[0] == 0.0 and not np.signbit(d[0]) and (d[1:] > 0).all()
    u, v = np.array([[1.25], [-3.0], [7.5]]), np.array([0.1])
    got = ertdiff.wasserstein(u, v).cpu().numpy()
    assert np.array_equal(got, np.abs(u[:, 0] - v[0]))


def test_distance_nan(tile, cuda_dev):
    M = tile["f64"] + 1
    x = _inputs(3, M, np.float64, 61)["random"]
    v = _inputs(1, M, np.float64, 62)["random"][0]
    clean = ertdiff.wasserstein(x, v).cpu().numpy()
    xn = x.copy()
    xn[1, 17] = np.nan
    got = ertdiff.wasserstein(xn, v).cpu().numpy()
    assert np.isnan(got[1]) and np.array_equal(got[[0, 2]], clean[[0, 2]])
    vn = v.copy()
    vn[M // 2] = np.nan
    assert np.isnan(ertdiff.wasserstein(x, vn).cpu().numpy()).all()


@pytest.mark.parametrize("name", ["a", "b", "c_f64", "c_f32"])
def test_fixture(name, kat, cuda_dev):
    u, v = G.cases()[name]
    got = ertdiff.wasserstein(u, v).cpu().numpy()
    want = kat["w1_" + name]
    rel = np.abs(got - want) / np.abs(want)
    print(f"fixture {name}: max rel err {rel.max():.3e}")
    record_error(f"wasserstein fixture {name}", rel.max())
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    one = ertdiff.wasserstein_distance(u[0].reshape(-1), v.reshape(-1))
    assert isinstance(one, float)
    assert one == ertdiff.wasserstein(u[0].reshape(-1)[None], v.reshape(-1))[0].item() == got[0]
    if "mse_" + name in kat.files:
        m = ertdiff.mse(u, v)
        assert m.dtype == torch.float64 and tuple(m.shape) == (u.shape[0],)
        mrel = np.abs(m.cpu().numpy() - kat["mse_" + name]) / kat["mse_" + name]
        record_error(f"mse fixture {name}", mrel.max())
        np.testing.assert_allclose(m.cpu().numpy(), kat["mse_" + name], rtol=1e-12, atol=0)


def test_deterministic(cuda_dev):
    x = torch.from_numpy(_inputs(3, 65702, np.float64, 71)["random"]).to(cuda_dev)
    v = torch.from_numpy(_inputs(1, 65702, np.float64, 72)["random"][0]).to(cuda_dev)
    assert torch.equal(ertdiff.sort_rows(x), ertdiff.sort_rows(x))
    a, b = ertdiff.wasserstein(x, v), ertdiff.wasserstein(x, v)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_c_abi_errors(tile, cuda_dev):
    lib = _lib.lib()
    T = tile["f64"]
    M = T + 1
    x = torch.zeros(2, M, dtype=torch.float64, device=cuda_dev)
    out = torch.full((2, M), -7.0, dtype=torch.float64, device=cuda_dev)
    need = lib.ertd_rows_sort_ws_bytes(1, 2, M)
    assert need >= 2 * M * 8
    ws = torch.empty(need, dtype=torch.uint8, device=cuda_dev)
    args = (x.data_ptr(), 1, 2)
    tail = (out.data_ptr(), ws.data_ptr())
    assert lib.ertd_rows_sort(*args, 0, 0, *tail, need, None) == _lib.ERTD_EINVAL           # M = 0
    assert lib.ertd_rows_sort(*args, M, M - 1, *tail, need, None) == _lib.ERTD_EINVAL       # ld < M
    assert lib.ertd_rows_sort(None, 1, 1, 2 ** 24 + 1, 2 ** 24 + 1, None, None, 0, None) == _lib.ERTD_EINVAL
    assert lib.ertd_rows_sort(x.data_ptr(), 1, 0, M, M, *tail, need, None) == _lib.ERTD_EINVAL   # n = 0
    assert lib.ertd_rows_sort(x.data_ptr(), 2, 2, M, M, *tail, need, None) == _lib.ERTD_EINVAL   # dtype
    assert lib.ertd_rows_sort(*args, M, M, *tail, need - 1, None) == _lib.ERTD_ENOSPC
    assert lib.ertd_rows_sort_tile(2) == 0 and lib.ertd_rows_sort_ws_bytes(1, 2, 0) == 0
    assert lib.ertd_rows_sort_ws_bytes(1, 2, T) == 0                                         # one tile: no merge

    v = torch.zeros(M, dtype=torch.float64, device=cuda_dev)
    d = torch.full((2,), -7.0, dtype=torch.float64, device=cuda_dev)
    wneed = lib.ertd_wasserstein_ws_bytes(1, 2, M, M)
    assert wneed > 0
    wws = torch.empty(wneed, dtype=torch.uint8, device=cuda_dev)
    w = lib.ertd_wasserstein
    assert w(x.data_ptr(), 1, 2, 0, 0, v.data_ptr(), M, d.data_ptr(), wws.data_ptr(), wneed, None) == _lib.ERTD_EINVAL
    assert w(x.data_ptr(), 1, 2, M, M, v.data_ptr(), 0, d.data_ptr(), wws.data_ptr(), wneed, None) == _lib.ERTD_EINVAL
    assert w(x.data_ptr(), 1, 2, M, M - 1, v.data_ptr(), M, d.data_ptr(), wws.data_ptr(), wneed, None) == _lib.ERTD_EINVAL
    assert w(None, 1, 1, 2 ** 24 + 1, 2 ** 24 + 1, None, 5, None, None, 0, None) == _lib.ERTD_EINVAL
    assert w(x.data_ptr(), 1, 2, M, M, v.data_ptr(), M, d.data_ptr(), wws.data_ptr(), wneed - 1, None) == _lib.ERTD_ENOSPC
    torch.cuda.synchronize(cuda_dev)
    assert bool((out == -7.0).all()) and bool((d == -7.0).all())                             # nothing was launched


def test_python_guards(cuda_dev):
    u = torch.zeros(2, 5, dtype=torch.float64, device=cuda_dev)
    with pytest.raises(ValueError, match="dtype"):
        ertdiff.wasserstein(u, torch.zeros(5, dtype=torch.float32, device=cuda_dev))
    with pytest.raises(ValueError, match="empty"):
        ertdiff.wasserstein(u, torch.zeros(0, dtype=torch.float64, device=cuda_dev))
    with pytest.raises(ValueError, match="empty"):
        ertdiff.wasserstein(u[:0], u[0])
    with pytest.raises(ValueError, match="empty"):
        ertdiff.sort_rows(u[:, :0])
    with pytest.raises(ValueError, match="empty"):
        ertdiff.mse(u[:0], u[0])
    with pytest.raises(ValueError, match="dtype"):
        ertdiff.mse(u, torch.zeros(5, dtype=torch.float32, device=cuda_dev))
    with pytest.raises(ValueError):
        ertdiff.sort_rows(torch.zeros(2, 3, 4, device=cuda_dev))
    with pytest.raises(ValueError, match="float32 or float64"):
        ertdiff.sort_rows(np.zeros((2, 3), dtype=np.int32))
