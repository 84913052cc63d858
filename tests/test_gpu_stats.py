"""Device ensemble statistics (csrc/ensstats.hip, ertdiff.stats) against numpy
and the reference fixture (tests/golden/stats_kat.npz).

Percentiles and coverage are bitwise: np.array_equal on float64 against
np.percentile(x, p, axis=0), exact equality of the coverage curve and its
scores.  Moments and WSSE are float64 sums in another order than numpy's:
rtol 1e-12, the project's float64 gate (tests/test_gpu_kde.py), on data whose
cell means are not cancellation-dominated; the measured errors are recorded."""
import numpy as np
import pytest
import torch

import ertdiff
from ertdiff import _lib
from conftest import load_golden, record_error
import make_stats_golden as G

pytestmark = pytest.mark.gpu

PROB = np.linspace(0.01, 0.99, 30)
# the 60 calibration levels as the reference forms them, plus the summary's
PERCENTS = np.concatenate([(1 - PROB) / 2 * 100, (1 + PROB) / 2 * 100, [0, 25, 50, 75, 100]])

NS = (1, 2, 3, 50, 63, 64, 65, 100, 257, 1000, 4097, 16384)
CELLS = (1, 29, 63, 64, 65, 518)
# plus the edges of the in-register regime (columns of up to 256 samples, 64 per register)
SHAPES = sorted({(n, 65) for n in NS} | {(n, c) for n in (50, 257) for c in CELLS}
                | {(128, 65), (129, 65), (256, 65)})


@pytest.fixture(scope="module")
def stats_kat():
    return load_golden("stats_kat.npz")


def _ensemble(n, cells, dtype, seed):
    """Columns with scales 1e-3 ... 1e4 and offsets; one constant column, one
    with heavily duplicated values."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** (np.arange(cells) % 8 - 3)
    x = (rng.normal(size=(n, cells)) + rng.uniform(-2, 2, cells)) * scale
    if cells > 1:
        x[:, 1] = 2.5 * scale[1]
    if cells > 2:
        x[:, 2] = np.round(x[:, 2] / scale[2]) * scale[2]
    return x.astype(dtype)


def _offset_ensemble(n, cells, dtype, seed):
    """Column scales 1e-3 ... 1e4 with offsets of 3 to 5 scales, so that
    |mean| >= 0.1 mean|x|: moments are not cancellation-dominated."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** (np.arange(cells) % 8 - 3)
    return ((rng.normal(size=(n, cells)) + rng.uniform(3, 5, cells)) * scale).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,cells", SHAPES)
def test_percentiles_bitwise(n, cells, dtype, cuda_dev):
    x = _ensemble(n, cells, dtype, 1000 * n + cells)
    got = ertdiff.ensemble_percentile(torch.from_numpy(x).to(cuda_dev), PERCENTS)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(PERCENTS), cells)
    assert np.array_equal(got.cpu().numpy(), np.percentile(x, PERCENTS, axis=0))


@pytest.mark.parametrize("n", [50, 257])
def test_strided_view(n, cuda_dev):
    big = torch.from_numpy(_offset_ensemble(n, 80, np.float32, 7)).to(cuda_dev)
    view = big[:, 3:68]                       # ld = 80 > cells = 65
    assert not view.is_contiguous()
    vn = view.cpu().numpy()
    got = ertdiff.ensemble_percentile(view, PERCENTS)
    assert np.array_equal(got.cpu().numpy(), np.percentile(vn, PERCENTS, axis=0))
    mean, var = ertdiff.ensemble_moments(view)
    np.testing.assert_allclose(mean.cpu().numpy(), vn.astype(np.float64).mean(0), rtol=1e-12)
    np.testing.assert_allclose(var.cpu().numpy(), vn.astype(np.float64).var(0), rtol=1e-12)


def test_too_many_samples_is_an_error(cuda_dev):
    x = torch.zeros(16385, 2, device=cuda_dev)
    q = torch.tensor([0.5], dtype=torch.float64, device=cuda_dev)
    out = torch.empty(1, 2, dtype=torch.float64, device=cuda_dev)
    rc = _lib.lib().ertd_ens_percentile(x.data_ptr(), 0, 16385, 2, 2, None, 1, q.data_ptr(), 1,
                                        out.data_ptr(), None, None)
    assert rc == _lib.ERTD_EINVAL
    with pytest.raises(ValueError):
        ertdiff.ensemble_percentile(x, [50])


@pytest.mark.parametrize("n", [50, 4097])
def test_nan_poisons_its_column_only(n, cuda_dev):
    x = _ensemble(n, 65, np.float64, 3)
    x[n // 3, 7] = np.nan
    got = ertdiff.ensemble_percentile(torch.from_numpy(x).to(cuda_dev), PERCENTS).cpu().numpy()
    assert np.isnan(got[:, 7]).all()
    keep = np.arange(65) != 7
    assert np.array_equal(got[:, keep], np.percentile(x[:, keep], PERCENTS, axis=0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_masked_percentiles(dtype, cuda_dev):
    n, N, P = 23, 9, 5
    x = _offset_ensemble(n, N * P, dtype, 11).reshape(n, N, P)
    valid = np.random.default_rng(12).random((n, N)) < 0.7
    valid[:, 4] = False                       # a test sample with no valid realisation
    valid[:, 6] = True
    valid[1:, 2] = False                      # ... and one with a single realisation
    valid[0, 2] = True
    got, n_eff = ertdiff.ensemble_percentile(torch.from_numpy(x).to(cuda_dev), PERCENTS,
                                             valid=torch.from_numpy(valid).to(cuda_dev),
                                             return_n_eff=True)
    got, n_eff = got.cpu().numpy(), n_eff.cpu().numpy()
    assert got.shape == (len(PERCENTS), N, P)
    for i in range(N):
        for p in range(P):
            kept = x[valid[:, i], i, p]
            assert n_eff[i, p] == kept.size
            if kept.size == 0:
                assert np.isnan(got[:, i, p]).all()
            else:
                assert np.array_equal(got[:, i, p], np.percentile(kept, PERCENTS))
    mean, var = ertdiff.ensemble_moments(torch.from_numpy(x).to(cuda_dev),
                                         valid=torch.from_numpy(valid).to(cuda_dev))
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    assert np.isnan(mean[4]).all() and np.isnan(var[4]).all()
    for i in (0, 2, 6):
        kept = x[valid[:, i], i].astype(np.float64)
        np.testing.assert_allclose(mean[i], kept.mean(0), rtol=1e-12)
        np.testing.assert_allclose(var[i], kept.var(0), rtol=1e-12, atol=0)


# ---- coverage ------------------------------------------------------------------

def _numpy_counts(gen, true, prob=PROB, valid=None):
    """The reference's loop, per column so that a mask can drop realisations."""
    S, N, P = gen.shape
    counts = np.zeros((len(prob), P), np.int64)
    cols = np.zeros(P, np.int64)
    for i in range(N):
        kept = gen[:, i] if valid is None else gen[valid[:, i], i]
        if kept.shape[0] == 0:
            continue
        cols += 1
        for k, pr in enumerate(prob):
            low = np.percentile(kept, (1 - pr) / 2 * 100, axis=0)
            upp = np.percentile(kept, (1 + pr) / 2 * 100, axis=0)
            counts[k] += (low < true[i]) & (true[i] <= upp)
    return counts, cols


def test_coverage_matches_reference_fixture(stats_kat, cuda_dev):
    gen, true = G.calibration_inputs()
    avg, per_param, counts, cols = ertdiff.coverage_curve(torch.from_numpy(gen).to(cuda_dev),
                                                          torch.from_numpy(true).to(cuda_dev))
    assert np.array_equal(cols, np.full(29, 37))
    assert np.array_equal(avg, stats_kat["avg_proportion"])
    assert np.array_equal(per_param, stats_kat["avg_proportion_per_param"])
    assert tuple(ertdiff.uncertainty_metrics(avg, PROB)) == tuple(stats_kat["scores"])
    got = ertdiff.parameter_uncertainty_metrics(gen, true, device=cuda_dev)
    assert np.array_equal(got, stats_kat["param_scores"])


def test_coverage_strict_and_inclusive_edges(cuda_dev):
    """Truths placed exactly on numpy's lower and upper bounds: the lower
    comparison is strict, the upper inclusive."""
    rng = np.random.default_rng(21)
    S, N, P = 7, 5, 3
    gen = rng.normal(size=(S, N, P)) * [1e-3, 1.0, 1e4]
    true = rng.normal(size=(N, P)) * [1e-3, 1.0, 1e4] * 0.5
    for j, (i, p, k) in enumerate([(0, 0, 3), (1, 1, 10), (2, 2, 17), (3, 0, 25), (4, 1, 29), (0, 2, 0)]):
        pc = ((1 - PROB[k]) if j % 2 == 0 else (1 + PROB[k])) / 2 * 100
        true[i, p] = np.percentile(gen[:, i, p], pc)
    want, wcols = _numpy_counts(gen, true)
    # both edges are in play: moving a truth on the lower bound up one ulp adds a hit
    bumped = true.copy()
    bumped[0, 0] = np.nextafter(true[0, 0], np.inf)
    assert _numpy_counts(gen, bumped)[0][3, 0] == want[3, 0] + 1
    _, _, counts, cols = ertdiff.coverage_curve(torch.from_numpy(gen).to(cuda_dev),
                                                torch.from_numpy(true).to(cuda_dev))
    assert np.array_equal(counts, want) and np.array_equal(cols, wcols)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_coverage_masked_and_halves(dtype, cuda_dev):
    rng = np.random.default_rng(22)
    S, N, P = 50, 37, 29
    gen, true = G.calibration_inputs()
    gen, true = gen.astype(dtype), true.astype(dtype)
    valid = rng.random((S, N)) < 0.8
    valid[:, 5] = False
    want, wcols = _numpy_counts(gen, true, valid=valid)
    g, t = torch.from_numpy(gen).to(cuda_dev), torch.from_numpy(true).to(cuda_dev)
    avg, per_param, counts, cols = ertdiff.coverage_curve(g, t, valid=torch.from_numpy(valid).to(cuda_dev))
    assert np.array_equal(counts, want) and np.array_equal(cols, wcols)
    assert cols[0] == N - 1
    assert np.array_equal(avg, want.sum(1) / wcols.sum())
    assert np.array_equal(per_param, (want / wcols).T)
    # two halves of the test set add up to the whole (a sharded evaluation)
    whole = ertdiff.coverage_counts(g, t)
    a = ertdiff.coverage_counts(g[:, :18], t[:18])
    b = ertdiff.coverage_counts(g[:, 18:], t[18:])
    assert np.array_equal(a[0] + b[0], whole[0]) and np.array_equal(a[1] + b[1], whole[1])


# ---- moments and WSSE ------------------------------------------------------------

def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


def test_summary_and_wsse_match_reference_fixture(stats_kat, cuda_dev):
    sim, obs = G.simulation_inputs()
    k = stats_kat
    s = ertdiff.ensemble_summary(sim, device=cuda_dev)
    assert tuple(s["mean"].shape) == (6, 8) and tuple(s["percentiles"].shape) == (3, 6, 8)
    for name, key in (("mean", "sim_mean"), ("std", "sim_std"), ("var", "sim_var")):
        err = _rel(s[name].cpu().numpy(), k[key])
        record_error(f"stats.summary.{name}.fixture", err)
        assert err <= 1e-12
    pct = s["percentiles"].cpu().numpy()
    for j, key in enumerate(("sim_p25", "sim_p50", "sim_p75")):
        assert np.array_equal(pct[j], k[key])
    cv = k["sim_std"] / (np.abs(k["sim_mean"]) + 1e-8)
    np.testing.assert_allclose(s["cv"].cpu().numpy(), cv, rtol=1e-12)
    w = ertdiff.wsse(sim, obs, float(k["wsse_A"]), float(k["wsse_B"]), device=cuda_dev)
    assert tuple(w.shape) == (40, 8)
    err = _rel(w.cpu().numpy(), k["wsse_sim"])
    record_error("stats.wsse.fixture", err)
    assert err <= 1e-12
    one, wse = ertdiff.WSSE_metric(0.1, 0.01, sim[3][:, 2], obs[:, 2], device=cuda_dev)
    assert abs(one - k["wsse_sim"][3, 2]) <= 1e-12 * k["wsse_sim"][3, 2]
    sd = 0.1 * np.abs(obs[:, 2]) + 0.01
    np.testing.assert_allclose(wse.cpu().numpy(), (sim[3][:, 2] - obs[:, 2]) ** 2 / sd ** 2, rtol=1e-14)


def test_summary_shape_and_numpy_input(cuda_dev):
    sim, _ = G.simulation_inputs()
    s = ertdiff.ensemble_summary(sim, device=cuda_dev)               # numpy (40, 6, 8)
    flat = ertdiff.ensemble_summary(torch.from_numpy(sim.reshape(40, 48)).to(cuda_dev))
    assert set(s) == {"mean", "std", "var", "percentiles", "cv"}
    for key in ("mean", "std", "var", "cv"):
        assert tuple(s[key].shape) == (6, 8) and torch.equal(s[key].reshape(-1), flat[key])
    assert torch.equal(s["percentiles"].reshape(3, -1), flat["percentiles"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,cells", [(1, 65), (50, 29), (50, 518), (257, 65), (1000, 65), (16384, 65)])
def test_moments_vs_numpy(n, cells, dtype, cuda_dev):
    """Offsets of 3 to 5 column scales: |mean| >= 0.1 mean|x| by construction
    (asserted), so rtol 1e-12 is a statement about the summation alone."""
    x = _offset_ensemble(n, cells, dtype, n + cells)
    x64 = x.astype(np.float64)
    assert (np.abs(x64.mean(0)) >= 0.1 * np.abs(x64).mean(0)).all()
    mean, var = ertdiff.ensemble_moments(torch.from_numpy(x).to(cuda_dev))
    em = _rel(mean.cpu().numpy(), x64.mean(0))
    record_error(f"stats.moments.mean.n{n}.c{cells}.{np.dtype(dtype).name}", em)
    assert em <= 1e-12
    if n > 1:
        ev = _rel(var.cpu().numpy(), x64.var(0))
        record_error(f"stats.moments.var.n{n}.c{cells}.{np.dtype(dtype).name}", ev)
        assert ev <= 1e-12
    else:
        assert (var.cpu().numpy() == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,M,E", [(3, 1, 1), (5, 37, 14), (4, 300, 7), (2, 5, 300)])
def test_wsse_vs_numpy(n, M, E, dtype, cuda_dev):
    rng = np.random.default_rng(M + E)
    obs = (rng.uniform(-20, 20, (M, E))).astype(dtype)
    sim = (obs * (1 + 0.1 * rng.normal(size=(n, M, E)))).astype(dtype)
    w = ertdiff.wsse(torch.from_numpy(sim).to(cuda_dev), torch.from_numpy(obs).to(cuda_dev))
    s64, o64 = sim.astype(np.float64), obs.astype(np.float64)
    want = ((s64 - o64) ** 2 / (0.1 * np.abs(o64) + 0.01) ** 2).mean(axis=1)
    err = _rel(w.cpu().numpy(), want)
    record_error(f"stats.wsse.M{M}.E{E}.{np.dtype(dtype).name}", err)
    assert err <= 1e-12


# ---- the reference's shapes ------------------------------------------------------

def test_full_size_coverage(cuda_dev):
    """(50, 509, 29) float32: the test-set evaluation.  256 sampled columns'
    bounds bitwise against numpy, the counts against numpy's indicator."""
    g = torch.Generator(device=cuda_dev).manual_seed(5)
    S, N, P = 50, 509, 29
    scale = 10.0 ** (torch.arange(P, device=cuda_dev) % 8 - 3).float()
    centre = torch.randn(N, P, generator=g, device=cuda_dev) + 4.0
    gen = (centre + 0.3 * torch.randn(S, N, P, generator=g, device=cuda_dev)) * scale
    true = (centre + 0.3 * torch.randn(N, P, generator=g, device=cuda_dev)) * scale
    avg, per_param, counts, cols = ertdiff.coverage_curve(gen, true)
    gn, tn = gen.cpu().numpy(), true.cpu().numpy()
    low = np.percentile(gn, (1 - PROB) / 2 * 100, axis=0)
    upp = np.percentile(gn, (1 + PROB) / 2 * 100, axis=0)
    assert np.array_equal(counts, ((low < tn) & (tn <= upp)).sum(axis=1))
    assert np.array_equal(cols, np.full(P, N))
    assert np.array_equal(avg, ((low < tn) & (tn <= upp)).mean(axis=(1, 2)))
    assert 0.3 < avg[15] < 0.7                # a calibrated ensemble: the curve is not trivial
    pick = np.random.default_rng(3).choice(N * P, 256, replace=False)
    pct = ertdiff.ensemble_percentile(gen, PERCENTS).cpu().numpy().reshape(len(PERCENTS), -1)
    assert np.array_equal(pct[:, pick], np.percentile(gn.reshape(S, -1)[:, pick], PERCENTS, axis=0))


def test_full_size_summary(cuda_dev):
    """(100, 4693, 14) float64: the simulated ensemble.  256 sampled cells."""
    g = torch.Generator(device=cuda_dev).manual_seed(7)
    n, cells = 100, 4693 * 14
    loc = torch.rand(cells, generator=g, device=cuda_dev, dtype=torch.float64) * 40 + 2
    sc = torch.rand(cells, generator=g, device=cuda_dev, dtype=torch.float64) * 2 + 0.05
    x = (loc + sc * torch.randn(n, cells, generator=g, device=cuda_dev, dtype=torch.float64))
    s = ertdiff.ensemble_summary(x.reshape(n, 4693, 14))
    assert tuple(s["mean"].shape) == (4693, 14) and tuple(s["percentiles"].shape) == (3, 4693, 14)
    assert all(torch.isfinite(v).all() for v in s.values())
    pick = np.random.default_rng(3).choice(cells, 256, replace=False)
    xc = x.cpu().numpy()[:, pick]
    assert np.array_equal(s["percentiles"].cpu().numpy().reshape(3, -1)[:, pick],
                          np.percentile(xc, [25, 50, 75], axis=0))
    np.testing.assert_allclose(s["mean"].cpu().numpy().reshape(-1)[pick], xc.mean(0), rtol=1e-12)
    np.testing.assert_allclose(s["var"].cpu().numpy().reshape(-1)[pick], xc.var(0), rtol=1e-12)
    obs = (loc * 1.01).reshape(4693, 14)
    w = ertdiff.wsse(x.reshape(n, 4693, 14), obs).cpu().numpy()
    o = obs.cpu().numpy()
    want = ((x.cpu().numpy().reshape(n, 4693, 14)[:8] - o) ** 2 / (0.1 * np.abs(o) + 0.01) ** 2).mean(axis=1)
    np.testing.assert_allclose(w[:8], want, rtol=1e-12)
