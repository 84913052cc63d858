"""Ensemble percentiles, coverage calibration, moments and WSSE on the device.

The reference evaluates its results on the host from arrays the device
produced: the uncertainty calibration of `Uncertainty_params` (S, N, 29)
(ERT_Conditional_Diffusion.py:1089-1137, per parameter :1187-1276: 60
np.percentile calls over the realisation axis, the coverage indicator, the
averaged coverage curve and the accuracy / precision / goodness scores), the
per-cell statistics of the simulated ensemble (:867-876) and the WSSE of every
realisation and survey (:767-787).  Here the order statistics, the indicator
counts, the moments and the WSSE come from float64 kernels (csrc/ensstats.hip)
that read the arrays where they are; percentiles and coverage carry numpy's
bits.  Only the three scores of a 30-point curve are host numpy.  The
Wasserstein-1 distance of each simulated image to the observation (:860,
:898-899, scipy.stats.wasserstein_distance) and the sort of long rows behind
it come from csrc/rowsort.hip; the per-realisation MSE (:927-949) is a WSSE
with unit weights.

    ensemble_percentile(x, percents, valid=None)    -> (len(percents), *cells) float64
    ensemble_summary(sim_data, percentiles=(25, 50, 75)) -> dict mean/std/var/percentiles/cv
    coverage_curve(generated, true, prob_array=None, valid=None)
                                 -> avg_proportion (K,), per parameter (P, K), counts, cols
    parameter_uncertainty_metrics(generated, true)  -> (P, 3) accuracy, precision, goodness
    wsse(sim_data, observations, A=0.1, B=0.01)     -> (n, E) float64
    mse(sim_data, observations)                     -> (n,) float64
    sort_rows(x)                                    -> x's shape and dtype, rows ascending
    wasserstein(sim_data, observations)             -> (n,) float64
    wasserstein_distance(u_values, v_values)        -> float (scipy's name and signature)
    avg_prop_indicator_function, accuracy_score, preccision_score, goodness_score,
    uncertainty_metrics, WSSE_metric                 (the reference's names and spellings)
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_N = 16384                      # one workgroup sorts a whole column in LDS
_DTYPES = {torch.float32: 0, torch.float64: 1}     # ERTD_F32 / ERTD_F64
_trapezoid = getattr(np, "trapezoid", None) or np.trapz


# ---- host side: the scores of a coverage curve (reference :1089-1115) ---------

def avg_prop_indicator_function(avg_proportion, prob_array):
    """a(p): 1 where the observed coverage reaches the nominal level, else 0."""
    avg_proportion = np.asarray(avg_proportion)
    prob_array = np.asarray(prob_array)
    return np.array([1 if avg_proportion[i] >= prob_array[i] else 0
                     for i in range(prob_array.shape[0])])


def accuracy_score(a_p, prob_array):
    return _trapezoid(a_p, prob_array)


def preccision_score(Accuracy_unc, avg_proportion, prob_array, a_p):
    """Precision is defined only where there is accuracy: 0.0 otherwise."""
    if Accuracy_unc == 0:
        return 0.0
    return 1 - 2 * _trapezoid(a_p * (avg_proportion - prob_array), prob_array)


def goodness_score(a_p, avg_proportion, prob_array):
    return 1 - _trapezoid((3 * a_p - 2) * (avg_proportion - prob_array), prob_array)


def uncertainty_metrics(avg_proportion, prob_array) -> Tuple[float, float, float]:
    """(accuracy, precision, goodness) of one coverage curve."""
    avg_proportion = np.asarray(avg_proportion, dtype=np.float64)
    prob_array = np.asarray(prob_array, dtype=np.float64)
    a_p = avg_prop_indicator_function(avg_proportion, prob_array)
    acc = accuracy_score(a_p, prob_array)
    return (acc, preccision_score(acc, avg_proportion, prob_array, a_p),
            goodness_score(a_p, avg_proportion, prob_array))


def interval_fractions(prob_array) -> Tuple[np.ndarray, np.ndarray]:
    """The central interval of each level p as the float64 fractions
    np.percentile forms from the reference's arguments (:1124-1127):
    percent = ((1 -/+ p) / 2) * 100, then q = percent / 100."""
    p = np.asarray(prob_array, dtype=np.float64).reshape(-1)
    q_low = np.true_divide(((1 - p) / 2) * 100, 100.0)
    q_upp = np.true_divide(((1 + p) / 2) * 100, 100.0)
    return q_low, q_upp


def coverage_from_counts(counts, cols) -> Tuple[np.ndarray, np.ndarray]:
    """avg_proportion (K,) and per parameter (P, K) from indicator counts
    (K, P) and column counts (P): the reference's np.mean(indicator_matrix).
    Counts of disjoint slices of the test set add before this call."""
    counts = np.asarray(counts, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    if counts.ndim != 2 or cols.shape != (counts.shape[1],):
        raise ValueError(f"counts must be (K, P) and cols (P,), got {counts.shape} and {cols.shape}")
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.true_divide(counts.sum(axis=1), cols.sum())
        per_param = np.true_divide(counts.T, cols[:, None])
    return avg, per_param


# ---- device side ---------------------------------------------------------------

def _check_dtype(dtype, name: str) -> None:
    if dtype not in _DTYPES:
        raise ValueError(f"ertdiff: {name} must be float32 or float64, got {dtype}")


def _as_tensor(x, device, name: str) -> torch.Tensor:
    """numpy arrays go to `device` (default cuda:0) in their own dtype."""
    if isinstance(x, np.ndarray):
        _check_dtype({np.dtype(np.float32): torch.float32,
                      np.dtype(np.float64): torch.float64}.get(x.dtype, x.dtype), name)
        dev = torch.device(device) if device is not None else torch.device("cuda", 0)
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"ertdiff: {name} must be a numpy array or a tensor")
    _check_dtype(x.dtype, name)
    return x if device is None else x.to(device)


_q_cache: Dict[tuple, torch.Tensor] = {}


def _fractions_on(dev: torch.device, q: np.ndarray) -> torch.Tensor:
    """q as a float64 device tensor; the few level sets a program uses are kept
    (a host-to-device copy per call would cost more than the kernels)."""
    key = (str(dev), q.tobytes())
    t = _q_cache.get(key)
    if t is None:
        if len(_q_cache) >= 32:
            _q_cache.clear()
        t = _q_cache[key] = torch.from_numpy(q).to(dev)
    return t


def _check_n(n: int) -> None:
    if not 1 <= n <= MAX_N:
        raise ValueError(f"ertdiff: the ensemble axis must hold 1..{MAX_N} samples, got {n}")


def _rows(t: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """(tensor, cells, ld) of an (n, *cells) ensemble: a 2-D view whose rows
    are contiguous is read in place through its row pitch."""
    n = t.shape[0]
    cells = int(np.prod(t.shape[1:]))
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= cells:
        return t, cells, int(t.stride(0))
    return t.contiguous(), cells, cells


def _mask(valid, t: torch.Tensor, name: str) -> Tuple[Optional[torch.Tensor], int]:
    """valid (n, *cells[:-1]) -> contiguous uint8 on t's device, rows_per_valid."""
    if valid is None:
        return None, 1
    want = tuple(t.shape[:-1])
    if t.dim() < 2 or tuple(valid.shape) != want:
        raise ValueError(f"ertdiff: valid must be {want} for {name} {tuple(t.shape)}, "
                         f"got {tuple(valid.shape)}")
    if isinstance(valid, np.ndarray):
        valid = torch.from_numpy(np.ascontiguousarray(valid))
    if valid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"ertdiff: valid must be bool or uint8, got {valid.dtype}")
    v = valid.to(t.device).contiguous()
    return (v.view(torch.uint8) if v.dtype == torch.bool else v), int(t.shape[-1])


def _prepare(x, valid, device, name: str):
    t = _as_tensor(x, device, name)
    if t.dim() < 2:
        raise ValueError(f"ertdiff: {name} must be (n, *cells), got {tuple(t.shape)}")
    _check_n(t.shape[0])
    if t.numel() == 0:
        raise ValueError(f"ertdiff: {name} is empty")
    v, rpv = _mask(valid, t, name)
    dev = _lib.require_device(t, v)
    return t, v, rpv, dev


def ensemble_percentile(x, percents, valid=None, device=None, return_n_eff: bool = False):
    """np.percentile(x, percents, axis=0), bit for bit, on the device.

    x: (n, *cells) float32 or float64, a device tensor or a numpy array (moved
    to `device`).  percents: numpy's 0..100 scale.  valid (n, *cells[:-1]),
    bool/uint8: the realisations to use per leading cell index (postprocess's
    mask); a column with none yields NaN.  Returns (len(percents), *cells)
    float64 on the device, and the per-column sample count with return_n_eff."""
    q = np.true_divide(np.asarray(percents, dtype=np.float64).reshape(-1), 100.0)
    if q.size < 1 or not np.all((q >= 0) & (q <= 1)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    t, v, rpv, dev = _prepare(x, valid, device, "x")
    cell_shape = tuple(t.shape[1:])
    t, cells, ld = _rows(t)
    qd = _fractions_on(dev, q)
    out = torch.empty((q.size,) + cell_shape, dtype=torch.float64, device=dev)
    n_eff = torch.empty(cell_shape, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ertd_ens_percentile(
            t.data_ptr(), _DTYPES[t.dtype], t.shape[0], cells, ld, _lib.ptr(v), rpv, qd.data_ptr(),
            q.size, out.data_ptr(), n_eff.data_ptr(), _lib.stream_of(dev)), "ens_percentile")
    return (out, n_eff) if return_n_eff else out


def ensemble_moments(x, valid=None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-cell mean and population variance (np.mean / np.var over axis 0),
    two passes accumulated in float64 whatever the input dtype."""
    t, v, rpv, dev = _prepare(x, valid, device, "x")
    cell_shape = tuple(t.shape[1:])
    t, cells, ld = _rows(t)
    mean = torch.empty(cell_shape, dtype=torch.float64, device=dev)
    var = torch.empty(cell_shape, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ertd_ens_moments(
            t.data_ptr(), _DTYPES[t.dtype], t.shape[0], cells, ld, _lib.ptr(v), rpv,
            mean.data_ptr(), var.data_ptr(), _lib.stream_of(dev)), "ens_moments")
    return mean, var


def ensemble_summary(sim_data, percentiles=(25, 50, 75), device=None) -> Dict[str, torch.Tensor]:
    """The reference's ensemble statistics (:867-876) of sim_data (n, *cells):
    mean, std, var, percentiles (len(percentiles), *cells) and the coefficient
    of variation std / (|mean| + 1e-8), all float64 on the device."""
    t = _as_tensor(sim_data, device, "sim_data")
    mean, var = ensemble_moments(t)
    std = torch.sqrt(var)
    return {"mean": mean, "std": std, "var": var,
            "percentiles": ensemble_percentile(t, percentiles),
            "cv": std / (mean.abs() + 1e-8)}


def coverage_counts(generated, true, prob_array=None, valid=None, device=None):
    """The indicator counts of the calibration loop (:1121-1132) as numpy
    int64: counts (K, P) and cols (P).  See coverage_curve."""
    if prob_array is None:
        prob_array = np.linspace(0.01, 0.99, 30)
    q_low, q_upp = interval_fractions(prob_array)
    if q_low.size < 1 or not np.all((q_low >= 0) & (q_upp <= 1)):
        raise ValueError("prob_array must hold levels in [0, 1]")
    g = _as_tensor(generated, device, "generated")
    if g.dim() == 2:                       # one parameter: (S, N)
        g = g.unsqueeze(-1)
        true = true.reshape(tuple(true.shape) + (1,))
    if g.dim() != 3:
        raise ValueError(f"ertdiff: generated must be (S, N, P), got {tuple(g.shape)}")
    if tuple(true.shape) != tuple(g.shape[1:]):
        raise ValueError(f"ertdiff: true must be {tuple(g.shape[1:])} for generated "
                         f"{tuple(g.shape)}, got {tuple(true.shape)}")
    _check_n(g.shape[0])
    S, N, P = g.shape
    K = q_low.size
    if N < 1 or P < 1 or (K + 1) * P > 4096:
        raise ValueError(f"ertdiff: coverage needs N, P >= 1 and (K + 1) * P <= 4096, got {N}, {P}, {K}")
    tr = _as_tensor(true, g.device if isinstance(true, np.ndarray) else None, "true")
    if tr.dtype != g.dtype:
        raise ValueError(f"ertdiff: generated ({g.dtype}) and true ({tr.dtype}) must share a dtype")
    v, _ = _mask(valid, g, "generated")
    dev = _lib.require_device(g, tr, v)
    g, tr = g.contiguous(), tr.contiguous()
    ql, qu = _fractions_on(dev, q_low), _fractions_on(dev, q_upp)
    counts = torch.empty((K, P), dtype=torch.int32, device=dev)
    cols = torch.empty((P,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ertd_coverage(
            g.data_ptr(), tr.data_ptr(), _DTYPES[g.dtype], S, N, P, _lib.ptr(v), ql.data_ptr(),
            qu.data_ptr(), K, counts.data_ptr(), cols.data_ptr(), _lib.stream_of(dev)), "coverage")
    return counts.cpu().numpy().astype(np.int64), cols.cpu().numpy().astype(np.int64)


def coverage_curve(generated, true, prob_array=None, valid=None, device=None):
    """The reference's calibration loop (:1121-1132) in one launch.

    generated (S, N, P) and true (N, P), same dtype; prob_array: the interval
    levels (default np.linspace(0.01, 0.99, 30)); valid (S, N): the
    realisations to use per test sample.  Returns (avg_proportion (K,),
    avg_proportion_per_param (P, K), counts (K, P), cols (P,)) as numpy:
    avg_proportion[k] = counts[k].sum() / cols.sum(), per parameter
    counts[k, p] / cols[p] -- without a mask the reference's
    np.mean(indicator_matrix), exactly.  A sharded evaluation adds the counts
    and cols of its shards and calls coverage_from_counts."""
    counts, cols = coverage_counts(generated, true, prob_array, valid, device)
    avg, per_param = coverage_from_counts(counts, cols)
    return avg, per_param, counts, cols


def parameter_uncertainty_metrics(generated, true, prob_array=None, valid=None, device=None):
    """(P, 3) accuracy, precision, goodness per parameter: the columns of the
    reference's Parameter_uncertainty_metrics.csv (:1187-1276)."""
    if prob_array is None:
        prob_array = np.linspace(0.01, 0.99, 30)
    prob_array = np.asarray(prob_array, dtype=np.float64)
    _, per_param, _, _ = coverage_curve(generated, true, prob_array, valid, device)
    return np.array([uncertainty_metrics(row, prob_array) for row in per_param], dtype=np.float64)


def wsse(sim_data, observations, A: float = 0.1, B: float = 0.01, device=None) -> torch.Tensor:
    """WSSE of every realisation and survey (:775-784): sim_data (n, M, E),
    observations (M, E), same dtype; out[s, e] = mean_m (sim - obs)^2 /
    (A |obs| + B)^2 as (n, E) float64 on the device."""
    s = _as_tensor(sim_data, device, "sim_data")
    if s.dim() != 3:
        raise ValueError(f"ertdiff: sim_data must be (n, M, E), got {tuple(s.shape)}")
    if tuple(observations.shape) != tuple(s.shape[1:]):
        raise ValueError(f"ertdiff: observations must be {tuple(s.shape[1:])}, "
                         f"got {tuple(observations.shape)}")
    if s.numel() == 0:
        raise ValueError("ertdiff: sim_data is empty")
    o = _as_tensor(observations, s.device if isinstance(observations, np.ndarray) else None,
                   "observations")
    if o.dtype != s.dtype:
        raise ValueError(f"ertdiff: sim_data ({s.dtype}) and observations ({o.dtype}) must share a dtype")
    dev = _lib.require_device(s, o)
    s, o = s.contiguous(), o.contiguous()
    n, M, E = s.shape
    out = torch.empty((n, E), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ertd_wsse(s.data_ptr(), o.data_ptr(), _DTYPES[s.dtype], n, M, E,
                                        float(A), float(B), out.data_ptr(), _lib.stream_of(dev)),
                   "wsse")
    return out


def WSSE_metric(A, B, predictions, observations, device=None):
    """The reference's WSSE_metric (:767-773) for one realisation and one
    survey, without the print: (WSSE float, WSE (M,) float64 tensor)."""
    p = _as_tensor(predictions, device, "predictions").reshape(1, -1, 1)
    o = _as_tensor(observations, p.device if isinstance(observations, np.ndarray) else None,
                   "observations").reshape(-1, 1)
    value = wsse(p, o, A, B)
    o64, p64 = o.reshape(-1).to(torch.float64), p.reshape(-1).to(torch.float64)
    sd = A * o64.abs() + B
    return float(value.item()), (p64 - o64) ** 2 / sd ** 2


def mse(sim_data, observations, device=None) -> torch.Tensor:
    """sklearn's mean_squared_error of every flattened realisation against the
    flattened observation (:927-930, :940-941): sim_data (n, *cells),
    observations of the same number of values, same dtype; (n,) float64 on the
    device.  It is the WSSE with the weight (0 |o| + 1)^2, exactly 1."""
    n = int(sim_data.shape[0]) if len(sim_data.shape) else 0
    if n < 1 or int(np.prod(sim_data.shape)) == 0:
        raise ValueError("ertdiff: sim_data is empty")
    return wsse(sim_data.reshape(n, -1, 1), observations.reshape(-1, 1), A=0.0, B=1.0,
                device=device)[:, 0]


# ---- row sort and Wasserstein-1 distance (csrc/rowsort.hip) ---------------------

MAX_ROW = 1 << 24                  # keys per row


def _row_view(t: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """(tensor, M, ld) of n rows of M values: a 2-D view whose rows are
    contiguous is read in place through its row pitch (as _rows does for
    columns); anything else is flattened per row into a contiguous copy."""
    n = t.shape[0]
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t, int(t.shape[1]), int(t.stride(0))
    t = t.reshape(n, -1).contiguous()
    return t, int(t.shape[1]), int(t.shape[1])


def _check_rows(n: int, M: int, name: str) -> None:
    if n < 1 or M < 1:
        raise ValueError(f"ertdiff: {name} is empty")
    if M > MAX_ROW:
        raise ValueError(f"ertdiff: {name} holds {M} values per row, more than {MAX_ROW}")


def sort_rows(x, device=None) -> torch.Tensor:
    """np.sort(x, axis=-1) of x (n, M) or (M,), float32 or float64, on the
    device: every row ascending, NaNs last, bit for bit.  Returns a sorted copy
    in the input's shape and dtype.  Rows of any length up to 2^24 (many
    workgroups sort one row); a 2-D view with contiguous rows is read in place."""
    t = _as_tensor(x, device, "x")
    if t.dim() not in (1, 2):
        raise ValueError(f"ertdiff: x must be (n, M) or (M,), got {tuple(t.shape)}")
    shape = tuple(t.shape)
    t2 = t.unsqueeze(0) if t.dim() == 1 else t
    _check_rows(t2.shape[0], t2.shape[1], "x")
    dev = _lib.require_device(t2)
    t2, M, ld = _row_view(t2)
    n, dt = t2.shape[0], _DTYPES[t2.dtype]
    out = torch.empty((n, M), dtype=t2.dtype, device=dev)
    with torch.cuda.device(dev):
        lib = _lib.lib()
        need = lib.ertd_rows_sort_ws_bytes(dt, n, M)
        ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
        _lib.check(lib.ertd_rows_sort(t2.data_ptr(), dt, n, M, ld, out.data_ptr(), _lib.ptr(ws), need,
                                      _lib.stream_of(dev)), "rows_sort")
    return out.reshape(shape)


def wasserstein(sim_data, observations, device=None) -> torch.Tensor:
    """scipy.stats.wasserstein_distance(sim_data[s].flatten(),
    observations.flatten()) for every realisation s (:860, :898-899).

    sim_data (n, *cells) and observations of any shape, same dtype (float32 or
    float64), device tensors or numpy arrays; the two sides may hold different
    numbers of values.  Returns (n,) float64 on the device: scipy's terms bit
    for bit, added in a fixed order.  A NaN in a realisation makes its
    distance NaN, a NaN in the observation every distance."""
    u = _as_tensor(sim_data, device, "sim_data")
    if u.dim() < 2:
        raise ValueError(f"ertdiff: sim_data must be (n, *cells), got {tuple(u.shape)}")
    v = _as_tensor(observations, u.device if isinstance(observations, np.ndarray) else None,
                   "observations")
    if v.dtype != u.dtype:
        raise ValueError(f"ertdiff: sim_data ({u.dtype}) and observations ({v.dtype}) must share a dtype")
    _check_rows(u.shape[0], int(np.prod(u.shape[1:])), "sim_data")
    _check_rows(1, v.numel(), "observations")
    dev = _lib.require_device(u, v)
    u, Mu, ld = _row_view(u)
    v = v.reshape(-1).contiguous()
    n, Mv, dt = u.shape[0], v.numel(), _DTYPES[u.dtype]
    out = torch.empty((n,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        lib = _lib.lib()
        need = lib.ertd_wasserstein_ws_bytes(dt, n, Mu, Mv)
        if not need:
            raise ValueError(f"ertdiff: wasserstein cannot take {n} rows of {Mu} against {Mv} values")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.check(lib.ertd_wasserstein(u.data_ptr(), dt, n, Mu, ld, v.data_ptr(), Mv, out.data_ptr(),
                                        ws.data_ptr(), need, _lib.stream_of(dev)), "wasserstein")
    return out


def wasserstein_distance(u_values, v_values, u_weights=None, v_weights=None) -> float:
    """The reference's import (:13), scipy's name and signature, for two
    one-dimensional samples.  Weighted distributions are not on the device."""
    if u_weights is not None or v_weights is not None:
        raise ValueError("ertdiff: weighted distributions are not on the device; "
                         "wasserstein_distance takes u_weights = v_weights = None")
    if not isinstance(u_values, (np.ndarray, torch.Tensor)):
        u_values = np.asarray(u_values, dtype=np.float64)
    if not isinstance(v_values, (np.ndarray, torch.Tensor)):
        v_values = np.asarray(v_values, dtype=np.float64)
    return float(wasserstein(u_values.reshape(1, -1), v_values.reshape(-1))[0].item())
