"""Generate tests/golden/dataprep_kat.npz: the reference's scaling cell
(ERT_Conditional_Diffusion.py:230-269) and its inverse (:417-419) on a small
synthetic case, computed by sklearn's MinMaxScaler and the reference's own
DiffusionDataset.

Runs only where the reference checkout and sklearn are present.  The
DiffusionDataset class is taken from the reference at generation time the way
make_golden.py does it (the definitions before the data-loading cell, executed
in a fresh namespace); only numbers are written.

    python tests/golden/make_dataprep_golden.py --ref REFERENCE_CHECKOUT

Case: N = 37 samples, L = 53 positions x 14 surveys (F = 742), P = 29
parameters.  Values are log-normal, exp(2.3 z): +-3 sigma spans six decades
in every column.  They are rounded to float32 and stored as float64 so the
file compresses; the scalers' vectors carry full float64 mantissas, so every
product and sum still rounds.  Planted columns, in both arrays:
  CONST   one value throughout            -> range 0, scale_ 1
  TINY    1 + k * eps, k = i % 9           -> range 8 ulp < 10 eps, scale_ 1
  ONE_NAN one NaN at row NAN_ROW          -> skipped by nanmin / nanmax
  ALL_NAN NaN throughout                  -> every fitted value NaN
NAN_ROW is 20, so the one NaN is never a whole row piece on its own when the
rows are fed to partial_fit in pieces of 1, 7 and 29 (np.minimum would then
propagate it, in sklearn as here).
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402
from synth import synth_normal  # noqa: E402

N, L, C, P = 37, 53, 14, 29
NAN_ROW = 20
HELD_ROWS = 10
# planted columns: (CONST, TINY, ONE_NAN, ALL_NAN) as flat feature indices
ERT_COLS = (5, 100, 300, L * C - 1)
PAR_COLS = (3, 7, 11, P - 1)


def raw_table(shape, seed, cols):
    z = synth_normal(shape, seed).astype(np.float64)
    x = np.exp(2.3 * z).astype(np.float32).astype(np.float64)
    const, tiny, one_nan, all_nan = cols
    x[:, const] = 3.25
    x[:, tiny] = 1.0 + (np.arange(shape[0]) % 9) * np.finfo(np.float64).eps
    x[NAN_ROW, one_nan] = np.nan
    x[:, all_nan] = np.nan
    return x


def fitted(prefix, sc):
    return {f"{prefix}_scale": sc.scale_, f"{prefix}_min": sc.min_, f"{prefix}_data_min": sc.data_min_,
            f"{prefix}_data_max": sc.data_max_, f"{prefix}_data_range": sc.data_range_}


def main():
    from sklearn.preprocessing import MinMaxScaler
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of pnnl/ERT-Conditional-Diffusion-Model")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref = load_reference(args.ref)
    warnings.filterwarnings("ignore", "All-NaN slice encountered")

    ert2d = raw_table((N, L * C), 91, ERT_COLS)
    par2d = raw_table((N, P), 92, PAR_COLS)
    ert_sim = ert2d.reshape(N, L, C)
    sim_param = par2d.reshape(N, P, 1)
    res = {"ert_sim": ert_sim, "sim_param": sim_param, "ert_cols": np.array(ERT_COLS),
           "par_cols": np.array(PAR_COLS), "nan_row": np.array(NAN_ROW), "held_rows": np.array(HELD_ROWS)}

    # :230-269 as written
    a, b = 0.0, 1.0
    param_scaler = MinMaxScaler(feature_range=(a, b))
    sim_param_scaled = param_scaler.fit_transform(sim_param.reshape(N, -1)).reshape(sim_param.shape)
    ert_scaler = MinMaxScaler(feature_range=(0, 1))
    ert_sim_scaled = ert_scaler.fit_transform(ert_sim.reshape(N, -1)).reshape(ert_sim.shape)
    dataset = ref["DiffusionDataset"](sim_param_scaled, ert_sim_scaled)
    x0 = dataset.params.numpy().copy()
    cond = dataset.conditions.contiguous().numpy().copy()
    assert x0.dtype == np.float32 and cond.dtype == np.float32 and cond.shape == (N, C, L)
    res.update(fitted("par", param_scaler))
    res.update(fitted("ert", ert_scaler))
    res.update(par_scaled=sim_param_scaled.reshape(N, P), x0=x0, cond=cond)

    # :417-419 as written, on the float32 conditions
    ert_sim_test = cond.swapaxes(1, 2)
    inv = ert_scaler.inverse_transform(ert_sim_test.reshape(N, -1)).reshape(ert_sim_test.shape)
    assert inv.dtype == np.float32
    res["cond_inv"] = inv
    # the parameter scaler backwards in float64
    res["par_inv"] = param_scaler.inverse_transform(sim_param_scaled.reshape(N, P))

    # a scaler fitted on the first rows only, feature_range (-1, 2), applied to all rows
    held_par = MinMaxScaler(feature_range=(-1, 2)).fit(par2d[:HELD_ROWS])
    held_ert = MinMaxScaler(feature_range=(-1, 2)).fit(ert2d[:HELD_ROWS])
    res.update(fitted("held_par", held_par))
    res.update(fitted("held_ert", held_ert))
    res["held_par_scaled"] = held_par.transform(par2d)
    res["held_par_inv"] = held_par.inverse_transform(res["held_par_scaled"])

    path = os.path.join(args.out, "dataprep_kat.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
