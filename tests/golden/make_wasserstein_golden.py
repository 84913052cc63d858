"""Generate tests/golden/wasserstein_kat.npz: scipy's Wasserstein-1 distance and
sklearn's mean squared error of synthetic simulated ERT images against an
observation, as the reference computes them (ERT_Conditional_Diffusion.py:860,
:898-899 with the `wasserstein_distance` imported at :13; :927-930, :940-941).

Needs scipy and scikit-learn, the reference's own dependencies; the GPU tests
need neither.  The inputs are pure functions of tests/golden/synth.py seeds
(the case_* functions below, which the tests import), so the file holds
expected outputs only: a few kilobytes.  Usage:

    python tests/golden/make_wasserstein_golden.py
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from synth import synth_normal, synth_uniform  # noqa: E402

REF_CELLS = (4693, 14)             # one simulated ERT image of the reference


def _images(n, cells, seed):
    """sim (n, *cells) and obs cells, float64: positive apparent-resistivity-
    like levels, 10 % ensemble spread, 5 % observation noise."""
    level = 1.0 + 19.0 * synth_uniform(cells, seed).astype(np.float64)
    sim = level * (1.0 + 0.1 * synth_normal((n,) + tuple(cells), seed + 1).astype(np.float64))
    obs = level * (1.0 + 0.05 * synth_normal(cells, seed + 2).astype(np.float64))
    return sim, obs


def case_a():
    """sim (6, 37, 14) against obs (37, 14), float64."""
    return _images(6, (37, 14), 301)


def case_b():
    """u (4, 1500) against v (1201,), float64 multiples of 0.25: heavy ties,
    unequal sizes."""
    u = np.round(8.0 * synth_normal((4, 1500), 311).astype(np.float64)) * 0.25
    v = np.round(8.0 * synth_normal((1201,), 312).astype(np.float64) + 1.0) * 0.25
    return u, v


def case_c(dtype=np.float64):
    """The reference shape: sim (3, 4693, 14) against obs (4693, 14)."""
    sim, obs = _images(3, REF_CELLS, 321)
    return sim.astype(dtype), obs.astype(dtype)


def wasserstein_numpy(u, v):
    """scipy.stats._cdf_distance(p = 1, no weights) restated in numpy: both
    samples flattened and cast to float64, the merged sequence sorted, each
    empirical CDF evaluated at all but its last value, |difference| times the
    gaps, summed by np.sum."""
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    u_sorted, v_sorted = np.sort(u), np.sort(v)
    all_values = np.concatenate((u, v))
    all_values.sort(kind="mergesort")
    deltas = np.diff(all_values)
    u_cdf = u_sorted.searchsorted(all_values[:-1], "right") / u.size
    v_cdf = v_sorted.searchsorted(all_values[:-1], "right") / v.size
    return np.sum(np.multiply(np.abs(u_cdf - v_cdf), deltas))


def cases():
    """name -> (u (n, ...), v) of every fixture case."""
    return {"a": case_a(), "b": case_b(), "c_f64": case_c(np.float64), "c_f32": case_c(np.float32)}


def main():
    from scipy.stats import wasserstein_distance
    from sklearn.metrics import mean_squared_error

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    res = {}
    for name, (u, v) in cases().items():
        res["w1_" + name] = np.array([wasserstein_distance(r.flatten(), v.flatten()) for r in u],
                                     dtype=np.float64)
        # sklearn averages float32 inputs in float32: only its float64 results
        # are float64 references
        if u[0].size == v.size and u.dtype == np.float64:
            res["mse_" + name] = np.array([mean_squared_error(v.flatten(), r.flatten()) for r in u],
                                          dtype=np.float64)
        assert np.all(res["w1_" + name] > 0)
    out = os.path.join(args.out, "wasserstein_kat.npz")
    np.savez_compressed(out, **res)
    print("wasserstein_kat.npz", os.path.getsize(out))


if __name__ == "__main__":
    main()
