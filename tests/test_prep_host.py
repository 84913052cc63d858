"""Data preparation, host side (ertdiff/prep.py, csrc/dataprep.hip's C entry
points): the fixture tests/golden/dataprep_kat.npz holds what sklearn's
MinMaxScaler and the reference's DiffusionDataset compute for a small case
(make_dataprep_golden.py); the numpy restatement of the arithmetic contract
(tests/golden/dataprep_ref.py) must reproduce it bit for bit, and so must
sklearn where it is installed.  No GPU needed."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import random_split

import ertdiff
from ertdiff import _lib
from conftest import GOLDEN
import dataprep_ref as ref

FITTED = ("scale_", "min_", "data_min_", "data_max_", "data_range_")
KEYS = {"scale_": "scale", "min_": "min", "data_min_": "data_min", "data_max_": "data_max",
        "data_range_": "data_range"}


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "dataprep_kat.npz"), allow_pickle=False)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check_fitted(got, kat, prefix):
    for k in FITTED:
        assert same(got[k], kat[f"{prefix}_{KEYS[k]}"]), f"{prefix} {k}"


def test_fixture_has_the_planted_columns(kat):
    N = kat["ert_sim"].shape[0]
    ert2d = kat["ert_sim"].reshape(N, -1)
    const, tiny, one_nan, all_nan = kat["ert_cols"]
    eps = np.finfo(np.float64).eps
    assert kat["ert_data_range"][const] == 0.0 and kat["ert_scale"][const] == 1.0
    assert kat["ert_data_range"][tiny] == 8 * eps and kat["ert_scale"][tiny] == 1.0
    assert np.isnan(ert2d[:, one_nan]).sum() == 1 and np.isfinite(kat["ert_scale"][one_nan])
    assert np.isnan(ert2d[:, all_nan]).all() and np.isnan(kat["ert_scale"][all_nan])
    assert np.isnan(kat["ert_min"][all_nan]) and np.isnan(kat["ert_data_min"][all_nan])
    # six decades in an ordinary column
    assert kat["ert_data_max"][0] / kat["ert_data_min"][0] > 1e3
    assert kat["cond"].dtype == np.float32 and kat["x0"].dtype == np.float32


@pytest.mark.parametrize("pieces", [None, (1, 7, 29), (37,)])
def test_restatement_fit_reproduces_fixture(kat, pieces):
    N = kat["ert_sim"].shape[0]
    check_fitted(ref.fit(kat["ert_sim"].reshape(N, -1), (0, 1), pieces), kat, "ert")
    check_fitted(ref.fit(kat["sim_param"].reshape(N, -1), (0.0, 1.0), pieces), kat, "par")


def test_restatement_held_out_scaler_reproduces_fixture(kat):
    N, h = kat["ert_sim"].shape[0], int(kat["held_rows"])
    par = kat["sim_param"].reshape(N, -1)
    f = ref.fit(par[:h], (-1, 2))
    check_fitted(f, kat, "held_par")
    check_fitted(ref.fit(kat["ert_sim"].reshape(N, -1)[:h], (-1, 2)), kat, "held_ert")
    y = ref.transform(par, f["scale_"], f["min_"])
    assert same(y, kat["held_par_scaled"])
    assert same(ref.inverse_f64(y, f["scale_"], f["min_"]), kat["held_par_inv"])


def test_restatement_transforms_reproduce_fixture(kat):
    N = kat["ert_sim"].shape[0]
    par = kat["sim_param"].reshape(N, -1)
    y = ref.transform(par, kat["par_scale"], kat["par_min"])
    assert same(y, kat["par_scaled"])
    assert same(ref.inverse_f64(y, kat["par_scale"], kat["par_min"]), kat["par_inv"])
    assert same(ref.cond_build(kat["ert_sim"], kat["ert_scale"], kat["ert_min"]), kat["cond"])
    assert same(ref.cond_inverse(kat["cond"], kat["ert_scale"], kat["ert_min"]), kat["cond_inv"])
    # DiffusionDataset.params from the scaled parameters: ends in this host's logarithm
    x0 = ertdiff.transform_to_unconstrained(torch.from_numpy(y).float(), 0.0, 1.0).numpy()
    d = ref.ulp_distance(x0, kat["x0"])
    print("x0 vs fixture, ulp:", d)
    assert d <= ref.X0_ULPS


def test_single_rounding_inverse_is_not_the_contract(kat):
    """The float32 inverse rounds twice; rounding once gives other bits somewhere."""
    x = np.ascontiguousarray(kat["cond"].swapaxes(1, 2)).reshape(kat["cond"].shape[0], -1)
    once = ((x.astype(np.float64) - kat["ert_min"]) / kat["ert_scale"]).astype(np.float32)
    assert not same(once.reshape(kat["cond_inv"].shape), kat["cond_inv"])


def test_sklearn_reproduces_fixture(kat):
    pytest.importorskip("sklearn")
    import warnings
    from sklearn.preprocessing import MinMaxScaler
    warnings.filterwarnings("ignore", "All-NaN slice encountered")
    N = kat["ert_sim"].shape[0]
    ert2d, par = kat["ert_sim"].reshape(N, -1), kat["sim_param"].reshape(N, -1)
    es, ps = MinMaxScaler(feature_range=(0, 1)), MinMaxScaler(feature_range=(0.0, 1.0))
    ert_scaled, par_scaled = es.fit_transform(ert2d), ps.fit_transform(par)
    check_fitted({k: getattr(es, k) for k in FITTED}, kat, "ert")
    check_fitted({k: getattr(ps, k) for k in FITTED}, kat, "par")
    assert same(par_scaled, kat["par_scaled"])
    ds = ertdiff.DiffusionDataset(par_scaled.reshape(N, -1, 1), ert_scaled.reshape(kat["ert_sim"].shape))
    assert ref.ulp_distance(ds.params.numpy(), kat["x0"]) <= ref.X0_ULPS
    assert same(ds.conditions.contiguous().numpy(), kat["cond"])
    inv = es.inverse_transform(kat["cond"].swapaxes(1, 2).reshape(N, -1))
    assert same(inv.reshape(kat["cond_inv"].shape), kat["cond_inv"])
    # partial_fit over the row pieces the GPU test uses
    pf = MinMaxScaler(feature_range=(0, 1))
    r = 0
    for k in (1, 7, 29):
        pf.partial_fit(ert2d[r:r + k])
        r += k
    check_fitted({k: getattr(pf, k) for k in FITTED}, kat, "ert")


def test_sklearn_round_trip_of_the_scaler_object(kat):
    pytest.importorskip("sklearn")
    from sklearn.preprocessing import MinMaxScaler
    N, h = kat["sim_param"].shape[0], int(kat["held_rows"])
    par = kat["sim_param"].reshape(N, -1)
    sk = MinMaxScaler(feature_range=(-1, 2)).fit(par[:h])
    ours = ertdiff.DeviceMinMaxScaler.from_sklearn(sk)
    assert ours.feature_range == (-1, 2) and ours.n_samples_seen_ == h and ours.n_features_in_ == par.shape[1]
    for k in FITTED:
        assert isinstance(getattr(ours, k), np.ndarray) and same(getattr(ours, k), getattr(sk, k))
    back = ours.to_sklearn()
    assert same(back.transform(par), kat["held_par_scaled"])


def test_from_sklearn_takes_any_fitted_object(kat):
    class Fitted:
        feature_range = (0, 1)
        n_samples_seen_ = 37
    for k in FITTED:
        setattr(Fitted, k, kat[f"par_{KEYS[k]}"])
    s = ertdiff.DeviceMinMaxScaler.from_sklearn(Fitted())
    assert same(s.min_, kat["par_min"]) and same(s.scale_, kat["par_scale"])
    with pytest.raises(AttributeError):
        ertdiff.DeviceMinMaxScaler().scale_


@pytest.mark.filterwarnings("ignore:Length of split at index")
@pytest.mark.parametrize("n", [1, 9, 10, 5076])
def test_split_indices_equal_random_split(n):
    sizes = [int(0.8 * n), int(0.1 * n)]
    sizes.append(n - sum(sizes))
    want = random_split(range(n), sizes, generator=torch.Generator().manual_seed(1234 + n))
    got = ertdiff.split_indices(n, generator=torch.Generator().manual_seed(1234 + n))
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and g.tolist() == list(w.indices)
    # the default generator, as random_split's default
    torch.manual_seed(77)
    want = random_split(range(n), sizes)
    torch.manual_seed(77)
    got = ertdiff.split_indices(n)
    assert [g.tolist() for g in got] == [list(w.indices) for w in want]


def test_new_entries_reject_null_and_bad_sizes():
    lib = _lib.load()
    E = _lib.ERTD_EINVAL
    one = 8          # a non-null address that is never dereferenced: every call below is rejected first
    assert lib.ertd_minmax_ws_bytes(0, 5) == 0 and lib.ertd_minmax_ws_bytes(5, 0) == 0
    assert lib.ertd_minmax_ws_bytes(5076, 65702) >= 2 * 65702 * 8
    assert lib.ertd_minmax_ws_bytes(3, 29) == 2 * 3 * 29 * 8
    assert lib.ertd_minmax_partial_fit(None, 4, 4, 4, None, None, 0, None, 0, None) == E
    assert lib.ertd_minmax_partial_fit(one, 0, 4, 4, one, one, 0, one, 1 << 20, None) == E
    assert lib.ertd_minmax_partial_fit(one, 4, 4, 3, one, one, 0, one, 1 << 20, None) == E
    assert lib.ertd_minmax_partial_fit(one, 4, 4, 4, one, one, 0, one, 8, None) == _lib.ERTD_ENOSPC
    assert lib.ertd_minmax_finalize(None, None, 4, 0.0, 1.0, None, None, None, None) == E
    assert lib.ertd_minmax_finalize(one, one, 0, 0.0, 1.0, one, one, one, None) == E
    assert lib.ertd_minmax_transform(None, 4, 4, 4, None, None, None, 4, None) == E
    assert lib.ertd_minmax_transform(one, 4, 4, 4, one, one, one, 3, None) == E
    assert lib.ertd_minmax_inverse(None, 1, 4, 4, 4, None, None, None, 4, None) == E
    assert lib.ertd_minmax_inverse(one, 7, 4, 4, 4, one, one, one, 4, None) == E
    assert lib.ertd_minmax_cond(None, 4, 4, 14, None, None, None, None) == E
    assert lib.ertd_minmax_cond(one, 4, 0, 14, one, one, one, None) == E
    assert lib.ertd_minmax_cond(one, 4, 4, 17, one, one, one, None) == E
    assert lib.ertd_minmax_cond_inverse(None, 4, 4, 14, None, None, None, None) == E
    assert lib.ertd_minmax_cond_inverse(one, -1, 4, 14, one, one, one, None) == E


def test_prepare_dataset_rejects_bad_input(kat):
    par, ert = kat["sim_param"], kat["ert_sim"]
    with pytest.raises(RuntimeError, match="ertdiff: ert_sim must be float64.*float32"):
        ertdiff.prepare_dataset(par, ert.astype(np.float32), "cuda")
    with pytest.raises(RuntimeError, match="ertdiff: sim_param must be float64"):
        ertdiff.prepare_dataset(par.astype(np.float32), ert, "cuda")
    with pytest.raises(RuntimeError, match="ertdiff: sim_param has 36 rows, ert_sim has 37"):
        ertdiff.prepare_dataset(par[:36], ert, "cuda")
    with pytest.raises(RuntimeError, match=r"ertdiff: ert_sim must be \(N, L, 14\)"):
        ertdiff.prepare_dataset(par, ert[:, :, :13], "cuda")
    with pytest.raises(RuntimeError, match="ertdiff: ert_sim must be"):
        ertdiff.prepare_dataset(par, ert.reshape(37, -1), "cuda")
    with pytest.raises(RuntimeError, match="ertdiff: sim_param must be"):
        ertdiff.prepare_dataset(np.zeros((37, 29, 2)), ert, "cuda")
    with pytest.raises(RuntimeError, match="ertdiff: sim_param must be a numpy array"):
        ertdiff.prepare_dataset(par.tolist(), ert, "cuda")
    with pytest.raises(RuntimeError, match="ertdiff: chunk_rows"):
        ertdiff.prepare_dataset(par, ert, "cuda", chunk_rows=0)


def test_scaler_rejects_bad_input(kat):
    s = ertdiff.DeviceMinMaxScaler()
    with pytest.raises(RuntimeError, match="ertdiff: X must be float64.*float32"):
        s.fit(kat["sim_param"].reshape(37, -1).astype(np.float32))
    with pytest.raises(RuntimeError, match="ertdiff: X must be a numpy array or a torch tensor"):
        s.fit([[1.0, 2.0]])
    with pytest.raises(RuntimeError, match="ertdiff: X must have 2 dimensions"):
        s.fit(kat["sim_param"])
    with pytest.raises(RuntimeError, match="ertdiff: feature_range"):
        ertdiff.DeviceMinMaxScaler((1, 1))
