"""Host side of the Wasserstein distance (CPU only): the fixture
tests/golden/wasserstein_kat.npz is scipy's and sklearn's, the numpy restatement
the GPU tests compare against (make_wasserstein_golden.wasserstein_numpy)
reproduces it, and the guards of the drop-in fire before any device work."""
import numpy as np
import pytest

import ertdiff
from conftest import load_golden
import make_wasserstein_golden as G


@pytest.fixture(scope="module")
def kat():
    return load_golden("wasserstein_kat.npz")


@pytest.fixture(scope="module")
def cases():
    return G.cases()


def test_fixture_is_small_and_complete(kat, cases):
    assert set(kat.files) == {"w1_a", "w1_b", "w1_c_f64", "w1_c_f32", "mse_a", "mse_c_f64"}
    for name, (u, _) in cases.items():
        assert kat["w1_" + name].shape == (u.shape[0],) and kat["w1_" + name].dtype == np.float64
    assert cases["c_f64"][0].shape == (3, 4693, 14) and cases["c_f32"][0].dtype == np.float32
    assert cases["b"][0].shape == (4, 1500) and cases["b"][1].shape == (1201,)
    assert np.array_equal(cases["b"][0] * 4, np.round(cases["b"][0] * 4))      # multiples of 0.25


def test_numpy_restatement_matches_fixture(kat, cases):
    for name, (u, v) in cases.items():
        got = np.array([G.wasserstein_numpy(r, v) for r in u])
        np.testing.assert_allclose(got, kat["w1_" + name], rtol=1e-12, atol=0, err_msg=name)


def test_scipy_matches_fixture(kat, cases):
    stats = pytest.importorskip("scipy.stats")
    for name, (u, v) in cases.items():
        got = np.array([stats.wasserstein_distance(r.flatten(), v.flatten()) for r in u])
        np.testing.assert_allclose(got, kat["w1_" + name], rtol=1e-12, atol=0, err_msg=name)


def test_mse_fixture_is_the_mean_square(kat, cases):
    for name in ("a", "c_f64"):
        u, v = cases[name]
        want = ((u.reshape(u.shape[0], -1) - v.reshape(-1)) ** 2).mean(axis=1)
        np.testing.assert_allclose(kat["mse_" + name], want, rtol=1e-12, atol=0)


def test_weights_are_rejected_before_any_device_work():
    u, v = np.arange(5.0), np.arange(4.0)
    w = np.ones(5)
    with pytest.raises(ValueError, match="weighted"):
        ertdiff.wasserstein_distance(u, v, u_weights=w)
    with pytest.raises(ValueError, match="weighted"):
        ertdiff.wasserstein_distance(u, v, None, np.ones(4))
