"""Generate tests/golden/stats_kat.npz: the reference's uncertainty calibration,
ensemble statistics and WSSE on synthetic inputs.

Like make_golden.py this runs ONLY where the reference checkout is available.
It parses ERT_Conditional_Diffusion.py and executes, in a namespace that
supplies the inputs, just

  * the function definitions WSSE_metric (:767-773) and
    avg_prop_indicator_function / accuracy_score / preccision_score /
    goodness_score (:1089-1115),
  * the module-level calibration statements :1121-1137 and the per-parameter
    loop :1187-1214 (a for statement whose body also plots: `plt` is a no-op
    stand-in, and the stand-in for `print` records each parameter's curve),
  * the ensemble statistics :867-872 and the WSSE loop :775-784.

Only numbers are written.  The inputs are pure functions of tests/golden/synth.py
seeds (calibration_inputs, simulation_inputs below, which the tests import), so
the file holds expected outputs only.  Usage:

    python tests/golden/make_stats_golden.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import ast
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from synth import synth_normal, synth_uniform  # noqa: E402

S_CAL, N_CAL, P_CAL = 50, 37, 29
OVER_DISPERSED = 5        # parameter whose ensemble is 3x too wide
OUTSIDE = 11              # parameter whose truths lie outside every interval
_DECADES = (1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0, 1e3, 1e4)


def calibration_inputs():
    """generated (50, 37, 29) and true (37, 29), float32, physical-unit-like:
    parameter p has its own scale (1e-3 ... 1e4) and offset; per test sample the
    ensemble and the truth scatter about a common centre, with a spread ratio
    that varies over the parameters (0.6 ... 1.6: under- to over-confident)."""
    p = np.arange(P_CAL)
    scale = np.array([_DECADES[i % 8] * (1.0 + 0.125 * (i // 8)) for i in p])
    offset = scale * (3.0 + 0.25 * (p % 5))
    ratio = 0.6 + 0.25 * (p % 5)               # ensemble spread / truth spread
    ratio[OVER_DISPERSED] = 3.0
    centre = offset + scale * synth_normal((N_CAL, P_CAL), 91).astype(np.float64)
    true = centre + 0.2 * scale * synth_normal((N_CAL, P_CAL), 92).astype(np.float64)
    true[:, OUTSIDE] = centre[:, OUTSIDE] + 50.0 * scale[OUTSIDE]
    gen = centre + 0.2 * scale * ratio * synth_normal((S_CAL, N_CAL, P_CAL), 93).astype(np.float64)
    return gen.astype(np.float32), true.astype(np.float32)


def simulation_inputs():
    """sim_data (40, 6, 8) float64 and an observation (6, 8): positive
    apparent-resistivity-like values, 10 % ensemble spread."""
    level = 1.0 + 19.0 * synth_uniform((6, 8), 94).astype(np.float64)
    sim = level * (1.0 + 0.1 * synth_normal((40, 6, 8), 95).astype(np.float64))
    obs = level * (1.0 + 0.05 * synth_normal((6, 8), 96).astype(np.float64))
    return sim, obs


class _NoOp:
    """Stand-in for matplotlib.pyplot: every attribute is a callable returning it."""

    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


def _load(ref_dir):
    path = os.path.join(ref_dir, "ERT_Conditional_Diffusion.py")
    with open(path) as f:
        return ast.parse(f.read(), filename=path), path


def _run(tree, path, ns, keep):
    body = [n for n in tree.body if keep(n)]
    assert body, "no reference statements selected"
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore", DeprecationWarning)
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def _between(lo, hi):
    return lambda n: lo <= n.lineno <= hi


def gen_calibration(tree, path):
    gen, true = calibration_inputs()
    curves = []
    ns = {"np": np, "plt": _NoOp(), "generated_params_np": gen, "true_params_np": true,
          "names": [f"p{i}" for i in range(P_CAL)]}
    ns["print"] = lambda *a, **k: curves.append(ns["avg_proportion"].copy())
    _run(tree, path, ns, lambda n: isinstance(n, ast.FunctionDef) and 1089 <= n.lineno <= 1115)
    _run(tree, path, ns, _between(1121, 1137))
    res = {"prob_array": ns["prob_array"], "avg_proportion": ns["avg_proportion"].copy(),
           "scores": np.array([ns["Accuracy_unc"], ns["Precision_unc"], ns["Goodness_metric"]],
                              dtype=np.float64)}
    _run(tree, path, ns, _between(1187, 1214))
    per_param = np.array(curves)
    assert per_param.shape == (P_CAL, len(ns["prob_array"]))
    res["avg_proportion_per_param"] = per_param
    res["param_scores"] = np.stack([np.asarray(ns["param_accuracy"], np.float64),
                                    np.asarray(ns["param_precision"], np.float64),
                                    np.asarray(ns["param_goodness"], np.float64)], axis=1)
    # the indicator must really be exercised, and the two special parameters behave
    nontrivial = sum(1 for c in per_param if not (np.all(c == 0) or np.all(c == 1)))
    assert nontrivial >= 25, f"coverage curve trivial for {P_CAL - nontrivial} parameters"
    assert res["param_scores"][OUTSIDE, 0] == 0 and res["param_scores"][OUTSIDE, 1] == 0.0
    assert np.all(per_param[OVER_DISPERSED] >= ns["prob_array"])
    return res


def gen_simulation(tree, path):
    sim, obs = simulation_inputs()
    ns = {"np": np, "plt": _NoOp(), "sim_data": sim, "conditional_ert_sample": obs,
          "ert_surveys": sim.shape[2]}
    _run(tree, path, ns, lambda n: isinstance(n, ast.FunctionDef) and n.lineno == 767)
    _run(tree, path, ns, _between(775, 784))
    _run(tree, path, ns, _between(867, 872))
    assert ns["WSSE_sim"].shape == (sim.shape[0], sim.shape[2])
    return {"sim_mean": ns["ensemble_mean"], "sim_std": ns["ensemble_std"],
            "sim_var": ns["ensemble_variance"], "sim_p25": ns["P25"], "sim_p50": ns["P50"],
            "sim_p75": ns["P75"], "wsse_sim": ns["WSSE_sim"],
            "wsse_A": np.array(ns["A_sd"]), "wsse_B": np.array(ns["B_sd"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    tree, path = _load(args.ref)
    res = gen_calibration(tree, path)
    res.update(gen_simulation(tree, path))
    out = os.path.join(args.out, "stats_kat.npz")
    np.savez_compressed(out, **res)
    print("stats_kat.npz", os.path.getsize(out))


if __name__ == "__main__":
    main()
