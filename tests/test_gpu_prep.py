"""Data preparation on the device (csrc/dataprep.hip, ertdiff/prep.py) against
the sklearn / reference fixture tests/golden/dataprep_kat.npz and, at shapes
the fixture does not store, the numpy restatement of the contract
(tests/golden/dataprep_ref.py; test_prep_host.py shows it reproduces the
fixture).  Every comparison is an equality of bits: dtype, shape, values and
NaN positions."""
import os

import numpy as np
import pytest
import torch

import ertdiff
from conftest import GOLDEN
import dataprep_ref as ref

pytestmark = pytest.mark.gpu

FITTED = ("scale_", "min_", "data_min_", "data_max_", "data_range_")
KEYS = {"scale_": "scale", "min_": "min", "data_min_": "data_min", "data_max_": "data_max",
        "data_range_": "data_range"}


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "dataprep_kat.npz"), allow_pickle=False)


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check_fitted(scaler, want, what):
    for k in FITTED:
        got = getattr(scaler, k)
        assert isinstance(got, np.ndarray) and same(got, want[k]), f"{what}: {k}"


def fixture_vectors(kat, prefix):
    return {k: kat[f"{prefix}_{KEYS[k]}"] for k in FITTED}


def scaler_from(vec, feature_range=(0, 1), n=1):
    class Fitted:
        pass
    f = Fitted()
    f.feature_range, f.n_samples_seen_ = feature_range, n
    for k in FITTED:
        setattr(f, k, vec[k])
    return ertdiff.DeviceMinMaxScaler.from_sklearn(f)


@pytest.mark.parametrize("pieces", [None, (1, 7, 29)])
def test_fit_matches_fixture(kat, cuda_dev, pieces):
    """F = 742 (even: 16-byte loads) and F = 29 (odd: 8-byte loads), whole and
    through partial_fit over row pieces."""
    N = kat["ert_sim"].shape[0]
    for prefix, X, fr in (("ert", kat["ert_sim"].reshape(N, -1), (0, 1)),
                          ("par", kat["sim_param"].reshape(N, -1), (0.0, 1.0))):
        s = ertdiff.DeviceMinMaxScaler(fr, device=cuda_dev)
        if pieces is None:
            assert s.fit(X) is s
        else:
            r = 0
            for k in pieces:
                s.partial_fit(torch.from_numpy(X[r:r + k]).to(cuda_dev))
                r += k
        check_fitted(s, fixture_vectors(kat, prefix), prefix)
        assert s.n_samples_seen_ == N and s.n_features_in_ == X.shape[1]
        assert s.scale_ is s.scale_          # one host copy


def test_fit_many_slabs_strided_rows_and_refit(cuda_dev):
    """More rows than slabs, a slab boundary inside the 4-row unrolled loop,
    a row pitch wider than F, NaNs in the first, a middle and the last slab,
    and fit() after fit() forgetting the first data.  The views cover both
    load widths: even F on an even pitch from an aligned start (16-byte
    loads), odd F, and even F from a start that is only 8-byte aligned."""
    n, F = 1531, 38
    X = ref.lognormal((n, F + 4), 93)
    X[0, 1] = X[n - 1, 2] = X[700, 3] = np.nan
    X[:, 4] = np.nan
    d = torch.from_numpy(X).to(cuda_dev)
    s = ertdiff.DeviceMinMaxScaler((-1, 2), device=cuda_dev)
    s.fit(torch.from_numpy(ref.lognormal((5, F), 94) * 1e9).to(cuda_dev))
    for c0, c1 in ((0, F), (2, F + 2), (1, F), (1, F + 1)):
        view = d[:, c0:c1]
        assert view.stride(0) == F + 4
        s.fit(view)
        check_fitted(s, ref.fit(X[:, c0:c1], (-1, 2)), f"columns {c0}:{c1}")
        assert s.n_samples_seen_ == n and s.n_features_in_ == c1 - c0


def test_partial_fit_propagates_a_piece_that_is_all_nan(cuda_dev):
    """np.minimum / np.maximum between pieces propagate a NaN, as sklearn's partial_fit does."""
    X = ref.lognormal((6, 4), 95)
    X[3:, 1] = np.nan
    s = ertdiff.DeviceMinMaxScaler(device=cuda_dev)
    s.partial_fit(X[:3]).partial_fit(X[3:])
    want = ref.fit(X, (0, 1), pieces=(3, 3))
    assert np.isnan(want["data_min_"][1]) and not np.isnan(ref.fit(X)["data_min_"][1])
    check_fitted(s, want, "pieces (3, 3)")


def test_transform_cond_matches_fixture(kat, cuda_dev):
    s = scaler_from(fixture_vectors(kat, "ert"))
    cond = s.transform_cond(torch.from_numpy(kat["ert_sim"]).to(cuda_dev))
    assert same(cond, kat["cond"])
    N = kat["ert_sim"].shape[0]
    assert same(s.transform_cond(kat["ert_sim"].reshape(N, -1)), kat["cond"])      # 2-D numpy input
    fitted = ertdiff.DeviceMinMaxScaler(device=cuda_dev).fit(kat["ert_sim"].reshape(N, -1))
    assert same(fitted.transform_cond(kat["ert_sim"], L=kat["ert_sim"].shape[1]), kat["cond"])


@pytest.mark.parametrize("L", [1, 3, 4, 255, 256, 257, 4693])
def test_transform_cond_and_inverse_shapes(cuda_dev, L):
    """Tile edges (the tile is 256 positions), odd output row alignment and the real L."""
    n = 3
    ert = ref.lognormal((n, L, ref.C), 100 + L)
    ert[1, L // 2, 5] = np.nan
    f = ref.fit(ert.reshape(n, -1), (-1, 2))
    s = ertdiff.DeviceMinMaxScaler((-1, 2), device=cuda_dev).fit(ert.reshape(n, -1))
    check_fitted(s, f, f"L={L}")
    cond = s.transform_cond(torch.from_numpy(ert).to(cuda_dev))
    want = ref.cond_build(ert, f["scale_"], f["min_"])
    assert same(cond, want)
    if L in (1, 257, 4693):
        assert same(s.inverse_cond(cond), ref.cond_inverse(want, f["scale_"], f["min_"]))


def test_transform_cond_single_row_gives_fr0(cuda_dev):
    """n = 1: every range is 0, every scale 1, and min_ = fr0 - x, so x + min_ rounds back to fr0
    or next to it; the restatement decides the bits."""
    ert = ref.lognormal((1, 300, ref.C), 96)
    s = ertdiff.DeviceMinMaxScaler((0, 1), device=cuda_dev).fit(ert.reshape(1, -1))
    assert np.array_equal(s.scale_, np.ones(300 * ref.C)) and np.array_equal(s.data_range_, np.zeros(300 * ref.C))
    cond = s.transform_cond(ert)
    assert same(cond, ref.cond_build(ert, s.scale_, s.min_))
    assert same(cond, np.zeros((1, ref.C, 300), np.float32))


def test_transform_cond_into_a_row_slice(kat, cuda_dev):
    s = scaler_from(fixture_vectors(kat, "ert"))
    N, L, C = kat["ert_sim"].shape
    buf = torch.full((N + 5, C, L), -7.0, dtype=torch.float32, device=cuda_dev)
    r0, r1 = 11, 24
    got = s.transform_cond(torch.from_numpy(kat["ert_sim"][r0:r1]).to(cuda_dev), out=buf[2 + r0:2 + r1])
    assert got.data_ptr() == buf[2 + r0].data_ptr()
    b = buf.cpu().numpy()
    assert same(b[2 + r0:2 + r1], kat["cond"][r0:r1])
    assert (b[:2 + r0] == -7.0).all() and (b[2 + r1:] == -7.0).all()
    with pytest.raises(RuntimeError, match="ertdiff: out must be"):
        s.transform_cond(kat["ert_sim"][r0:r1], out=buf[:3])


def test_inverse_cond_matches_fixture(kat, cuda_dev):
    s = scaler_from(fixture_vectors(kat, "ert"))
    assert same(s.inverse_cond(torch.from_numpy(kat["cond"]).to(cuda_dev)), kat["cond_inv"])
    assert same(s.inverse_cond(kat["cond"]), kat["cond_inv"])                     # host input


def test_plain_transform_and_inverse_f64(kat, cuda_dev):
    """F = 29 from the fixture (whole-data and held-out-rows scalers), F = 742
    from the restatement; out-of-place, in place, and into a wider buffer."""
    N, h = kat["sim_param"].shape[0], int(kat["held_rows"])
    par = kat["sim_param"].reshape(N, -1)
    s = ertdiff.DeviceMinMaxScaler((0.0, 1.0), device=cuda_dev)
    y = s.fit_transform(par)
    assert y.dtype == torch.float64 and same(y, kat["par_scaled"])
    assert same(s.inverse_transform(y), kat["par_inv"])
    held = ertdiff.DeviceMinMaxScaler((-1, 2), device=cuda_dev).fit(par[:h])
    check_fitted(held, fixture_vectors(kat, "held_par"), "held_par")
    d = torch.from_numpy(par).to(cuda_dev)
    assert held.transform(d, out=d) is d and same(d, kat["held_par_scaled"])       # in place
    assert held.inverse_transform(d, out=d) is d and same(d, kat["held_par_inv"])
    # F = 742, strided destination
    ert2d = kat["ert_sim"].reshape(N, -1)
    he = ertdiff.DeviceMinMaxScaler((-1, 2), device=cuda_dev).fit(ert2d[:h])
    check_fitted(he, fixture_vectors(kat, "held_ert"), "held_ert")
    wide = torch.full((N, ert2d.shape[1] + 6), -7.0, dtype=torch.float64, device=cuda_dev)
    he.transform(ert2d, out=wide[:, 3:-3])
    want = ref.transform(ert2d, he.scale_, he.min_)
    w = wide.cpu().numpy()
    assert same(w[:, 3:-3], want) and (w[:, :3] == -7.0).all() and (w[:, -3:] == -7.0).all()
    assert same(he.inverse_transform(torch.from_numpy(want).to(cuda_dev)), ref.inverse_f64(want, he.scale_, he.min_))


def test_plain_inverse_f32_rounds_twice(kat, cuda_dev):
    s = scaler_from(fixture_vectors(kat, "ert"))
    N = kat["cond"].shape[0]
    x = np.ascontiguousarray(kat["cond"].swapaxes(1, 2)).reshape(N, -1)
    got = s.inverse_transform(x)
    assert got.dtype == torch.float32 and same(got.reshape(kat["cond_inv"].shape), kat["cond_inv"])


def test_device_scaler_rejects_float32_and_wrong_width(kat, cuda_dev):
    s = scaler_from(fixture_vectors(kat, "par"))
    with pytest.raises(RuntimeError, match="ertdiff: X must be float64.*float32"):
        s.transform(torch.zeros(2, 29, device=cuda_dev))
    with pytest.raises(RuntimeError, match="ertdiff: X has 30 features"):
        s.transform(torch.zeros(2, 30, dtype=torch.float64, device=cuda_dev))
    with pytest.raises(RuntimeError, match="ertdiff: X has 28 columns"):
        s.transform_cond(torch.zeros(2, 28, dtype=torch.float64, device=cuda_dev), L=3)


@pytest.fixture(scope="module")
def prepared(kat, cuda_dev):
    return ertdiff.prepare_dataset(kat["sim_param"], kat["ert_sim"], cuda_dev)


def test_prepare_dataset_matches_fixture(kat, prepared, cuda_dev):
    ds, ps, es = prepared
    assert isinstance(ds, ertdiff.DeviceDataset) and ds.device == cuda_dev and len(ds) == 37
    assert same(ds.cond, kat["cond"])
    # DeviceDataset.from_dataset(DiffusionDataset(sklearn-scaled arrays)) with the scaled arrays of
    # the fixture, built on this host: x0 ends in the host's logarithm (dataprep_ref.ulp_distance)
    N, L, C = kat["ert_sim"].shape
    ert_scaled = ref.transform(kat["ert_sim"].reshape(N, -1), kat["ert_scale"], kat["ert_min"])
    want = ertdiff.DeviceDataset.from_dataset(
        ertdiff.DiffusionDataset(kat["par_scaled"].reshape(N, -1, 1), ert_scaled.reshape(N, L, C)), cuda_dev)
    assert same(ds.x0, want.x0) and same(ds.cond, want.cond)
    d = ref.ulp_distance(host(ds.x0), kat["x0"])
    print("x0 vs fixture, ulp:", d)
    assert d <= ref.X0_ULPS
    check_fitted(ps, fixture_vectors(kat, "par"), "param_scaler")
    check_fitted(es, fixture_vectors(kat, "ert"), "ert_scaler")
    assert ps.feature_range == (0.0, 1.0) and es.feature_range == (0, 1)
    # (N, P) parameters and host tensors are accepted as well
    ds2, _, _ = ertdiff.prepare_dataset(torch.from_numpy(kat["sim_param"].reshape(37, -1)),
                                        torch.from_numpy(kat["ert_sim"]), cuda_dev)
    assert same(ds2.x0, ds.x0) and same(ds2.cond, kat["cond"])


@pytest.mark.parametrize("chunk", [5, 37, 100])
def test_prepare_dataset_chunked_gives_the_same_bits(kat, prepared, cuda_dev, chunk):
    ds, ps, es = prepared
    dc, pc, ec = ertdiff.prepare_dataset(kat["sim_param"], kat["ert_sim"], cuda_dev, chunk_rows=chunk)
    assert torch.equal(dc.x0.view(torch.int32), ds.x0.view(torch.int32))
    assert torch.equal(dc.cond.view(torch.int32), ds.cond.view(torch.int32))
    for k in FITTED:
        assert same(getattr(ec, k), getattr(es, k)) and same(getattr(pc, k), getattr(ps, k))
    assert ec.n_samples_seen_ == 37


def test_param_scaler_feeds_postprocess(kat, prepared, postproc_chain_kat, cuda_dev):
    _, ps, _ = prepared
    limits = postproc_chain_kat["limits"]
    u = torch.from_numpy(postproc_chain_kat["u"]).to(cuda_dev)
    a_out, a_valid = ertdiff.postprocess(u, ps, limits)
    b_out, b_valid = ertdiff.postprocess(u, (ps.min_, ps.scale_), limits)
    assert same(a_out, b_out) and torch.equal(a_valid, b_valid)
