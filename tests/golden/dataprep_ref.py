"""numpy restatement of the data-preparation contract (csrc/dataprep.hip,
include/ertdiff.h), shared by the host and the GPU tests.

Test infrastructure only.  Each function spells out one float64 operation
per line, so numpy rounds after every operation exactly as the contract
says; test_prep_host.py checks that this reproduces the sklearn / reference
fixture bit for bit, which lets the GPU tests use it at shapes the fixture
does not store.
"""
from __future__ import annotations

import warnings

import numpy as np

from synth import synth_normal

C = 14


def col_minmax(X):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # all-NaN column
        return np.nanmin(X, axis=0), np.nanmax(X, axis=0)


def finalize(data_min, data_max, feature_range=(0, 1)):
    """-> scale_, min_, data_range_"""
    fr0, fr1 = feature_range
    rng = data_max - data_min
    safe = rng.copy()
    safe[safe < 10 * np.finfo(np.float64).eps] = 1.0
    scale = (fr1 - fr0) / safe
    mn = fr0 - data_min * scale
    return scale, mn, rng


def fit(X, feature_range=(0, 1), pieces=None):
    """dict of the five fitted vectors; pieces: row counts fed to partial_fit in turn."""
    if pieces is None:
        dmin, dmax = col_minmax(X)
    else:
        assert sum(pieces) == X.shape[0]
        r, dmin, dmax = 0, None, None
        for k in pieces:
            pmin, pmax = col_minmax(X[r:r + k])
            dmin = pmin if dmin is None else np.minimum(dmin, pmin)
            dmax = pmax if dmax is None else np.maximum(dmax, pmax)
            r += k
    scale, mn, rng = finalize(dmin, dmax, feature_range)
    return {"scale_": scale, "min_": mn, "data_min_": dmin, "data_max_": dmax, "data_range_": rng}


def transform(X, scale, mn):
    t = X * scale
    return t + mn


def inverse_f64(X, scale, mn):
    t = X - mn
    return t / scale


def inverse_f32(X, scale, mn):
    assert X.dtype == np.float32
    t = (X.astype(np.float64) - mn).astype(np.float32)
    return (t.astype(np.float64) / scale).astype(np.float32)


def cond_build(ert, scale, mn):
    """ert (n, L, C) float64 -> (n, C, L) float32"""
    n, L, _ = ert.shape
    y = transform(ert.reshape(n, -1), scale, mn).reshape(n, L, C)
    return np.ascontiguousarray(np.transpose(y, (0, 2, 1)).astype(np.float32))


def cond_inverse(cond, scale, mn):
    """cond (n, C, L) float32 -> (n, L, C) float32"""
    n, _, L = cond.shape
    x = np.ascontiguousarray(cond.swapaxes(1, 2)).reshape(n, -1)
    return inverse_f32(x, scale, mn).reshape(n, L, C)


def ulp_distance(a, b):
    """Largest |a - b| in units of the float32 spacing at the larger magnitude;
    NaNs must sit at the same places.

    For x0 only.  x0 ends in torch.log on the host, and torch's CPU logarithm
    is not the same code on every machine (it is picked by the CPU's vector
    instruction set), so a fixture written on one host is not a bitwise
    reference on another.  Each variant is accurate to 1 ulp, so two of them
    lie within 2 ulp of each other: X0_ULPS.  Everything before the logarithm
    is IEEE arithmetic and is compared bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    a, b = a[ok], b[ok]
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return float(np.max(d / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64), initial=0.0))


X0_ULPS = 2.0


def lognormal(shape, seed):
    """exp(2.3 z): six decades between -3 and +3 sigma, full float64 mantissas."""
    return np.exp(2.3 * synth_normal(shape, seed).astype(np.float64))
