"""Host side of ertdiff.stats (CPU only): the reference's calibration scores
against the golden fixture (tests/golden/make_stats_golden.py), the
counts -> coverage arithmetic, the percentile formula the kernel implements,
and the input guards that fire before any launch."""
import numpy as np
import pytest
import torch

import ertdiff
from ertdiff import _lib, stats
from conftest import load_golden


@pytest.fixture(scope="module")
def stats_kat():
    return load_golden("stats_kat.npz")


def test_scores_match_reference(stats_kat):
    k = stats_kat
    prob = k["prob_array"]
    assert np.array_equal(prob, np.linspace(0.01, 0.99, 30))
    assert tuple(ertdiff.uncertainty_metrics(k["avg_proportion"], prob)) == tuple(k["scores"])
    for curve, want in zip(k["avg_proportion_per_param"], k["param_scores"]):
        a_p = ertdiff.avg_prop_indicator_function(curve, prob)
        acc = ertdiff.accuracy_score(a_p, prob)
        got = (acc, ertdiff.preccision_score(acc, curve, prob, a_p),
               ertdiff.goodness_score(a_p, curve, prob))
        assert got == tuple(want)
    # the parameter whose truths lie outside every interval: no accuracy, and
    # preccision_score's 0.0 branch
    outside = np.flatnonzero(~k["avg_proportion_per_param"].any(axis=1))
    assert outside.size >= 1 and (k["param_scores"][outside, :2] == 0).all()
    assert ertdiff.preccision_score(0, k["avg_proportion"], prob, np.ones(30, int)) == 0.0


def test_coverage_from_counts_is_the_indicator_mean():
    rng = np.random.default_rng(0)
    K, N, P = 30, 37, 29
    ind = rng.random((K, N, P)) < np.linspace(0.05, 0.95, K)[:, None, None]
    counts = ind.sum(axis=1)
    cols = np.full(P, N)
    avg, per_param = ertdiff.coverage_from_counts(counts, cols)
    assert avg.shape == (K,) and per_param.shape == (P, K)
    for k in range(K):
        assert avg[k] == np.mean(ind[k].astype(int))
        for p in range(P):
            assert per_param[p, k] == np.mean(ind[k, :, p].astype(int))
    # shards of the test set add
    a, b = ind[:, :20].sum(axis=1), ind[:, 20:].sum(axis=1)
    avg2, _ = ertdiff.coverage_from_counts(a + b, np.full(P, 20) + np.full(P, 17))
    assert np.array_equal(avg, avg2)
    with pytest.raises(ValueError):
        ertdiff.coverage_from_counts(counts, cols[:-1])


def _quantile_restated(x, q):
    """The kernel's formula (include/ertdiff.h), per column, in numpy."""
    s = np.sort(x, axis=0)
    m = s.shape[0]
    out = np.empty((len(q),) + s.shape[1:], np.float64)
    for k, qk in enumerate(q):
        vi = (m - 1) * qk
        lo = int(np.floor(vi))
        hi = min(lo + 1, m - 1)
        t = vi - lo
        d = (s[hi] - s[lo]).astype(np.float64)      # subtraction in the input's dtype
        out[k] = s[lo].astype(np.float64) + d * t if t < 0.5 else s[hi].astype(np.float64) - d * (1 - t)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_percentile_formula_is_numpys(dtype):
    prob = np.linspace(0.01, 0.99, 30)
    q_low, q_upp = ertdiff.interval_fractions(prob)
    percents = np.concatenate([(1 - prob) / 2 * 100, (1 + prob) / 2 * 100, [0, 25, 50, 75, 100]])
    q = np.concatenate([q_low, q_upp, np.true_divide([0, 25, 50, 75, 100], 100.0)])
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 7, 50, 64, 65, 257):
        x = (rng.normal(size=(n, 11)) * 10.0 ** rng.integers(-3, 5, 11)).astype(dtype)
        assert np.array_equal(_quantile_restated(x, q), np.percentile(x, percents, axis=0))


def test_guards_fire_before_any_launch():
    g = torch.zeros(5, 4, 3)
    t = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="gfx950"):
        ertdiff.ensemble_percentile(g, [50])
    with pytest.raises(RuntimeError, match="gfx950"):
        ertdiff.ensemble_summary(g)
    with pytest.raises(RuntimeError, match="gfx950"):
        ertdiff.coverage_curve(g, t)
    with pytest.raises(RuntimeError, match="gfx950"):
        ertdiff.wsse(g, t)
    with pytest.raises(ValueError, match="true must be"):
        ertdiff.coverage_curve(g, torch.zeros(3, 4))
    with pytest.raises(ValueError, match="share a dtype"):
        ertdiff.coverage_curve(g, t.double())
    with pytest.raises(ValueError, match="valid must be"):
        ertdiff.coverage_curve(g, t, valid=torch.ones(5, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="observations must be"):
        ertdiff.wsse(g, torch.zeros(4, 2))
    with pytest.raises(ValueError, match="float32 or float64"):
        ertdiff.ensemble_percentile(torch.zeros(5, 4, dtype=torch.int32), [50])
    with pytest.raises(ValueError, match="float32 or float64"):
        ertdiff.ensemble_percentile(np.zeros((5, 4), np.float16), [50])
    with pytest.raises(ValueError, match=r"1\.\.16384"):
        ertdiff.ensemble_percentile(torch.zeros(stats.MAX_N + 1, 2), [50])
    with pytest.raises(ValueError, match=r"\(n, \*cells\)"):
        ertdiff.ensemble_percentile(torch.zeros(5), [50])
    with pytest.raises(ValueError, match="range"):
        ertdiff.ensemble_percentile(g, [101])
    with pytest.raises(ValueError, match="valid must be"):
        ertdiff.ensemble_percentile(g, [50], valid=torch.ones(5, 3, dtype=torch.bool))


def test_library_rejects_bad_arguments_on_the_host():
    """ERTD_EINVAL comes back before anything is launched (the pointers are
    never dereferenced on the host)."""
    lib = _lib.load()
    p = 4096
    E = _lib.ERTD_EINVAL
    assert lib.ertd_ens_percentile(None, 0, 50, 8, 8, None, 1, p, 1, p, None, None) == E
    assert lib.ertd_ens_percentile(p, 0, stats.MAX_N + 1, 8, 8, None, 1, p, 1, p, None, None) == E
    assert lib.ertd_ens_percentile(p, 0, 0, 8, 8, None, 1, p, 1, p, None, None) == E
    assert lib.ertd_ens_percentile(p, 2, 50, 8, 8, None, 1, p, 1, p, None, None) == E      # dtype
    assert lib.ertd_ens_percentile(p, 0, 50, 8, 7, None, 1, p, 1, p, None, None) == E      # ld < cells
    assert lib.ertd_ens_percentile(p, 0, 50, 8, 8, p, 3, p, 1, p, None, None) == E         # 8 % 3
    assert lib.ertd_ens_moments(p, 1, 0, 8, 8, None, 1, p, p, None) == E
    assert lib.ertd_coverage(p, p, 0, stats.MAX_N + 1, 4, 3, None, p, p, 30, p, p, None) == E
    assert lib.ertd_coverage(p, p, 0, 50, 4, 200, None, p, p, 30, p, p, None) == E         # (K+1) P
    assert lib.ertd_wsse(p, None, 1, 4, 6, 8, 0.1, 0.01, p, None) == E
