"""Time the few-step solver samplers beside the ancestral ones, in one run on
one box:

  * U2, B = 64, fp32, L = 4693: UNetSolverPlan at K = 50 (ddim and dpmpp_2m),
    ms per step and per chain, against UNetSamplerPlan per step (the same 50
    steps of its T = 1000 plan) and per whole T = 1000 chain;
  * the reference model, B = 64, L = 4693: ertd_sample_solver at K = 50 against
    the hoisted T = 500 chain.  The per-step time of each persistent kernel is
    the difference of a whole chain and a one-step call over the step count
    (both calls run the same encoder, prep and launches; the time table's
    extra rows, one small workgroup each, are part of the difference).

    python tools/solver_probe.py [--out profiles/solver_probe.json] [--windows 12]

Times are HIP events around one call per window after a warm call; each row
reports min / median / max over the windows.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ert-conditional-diffusion-model_amd"))
import ertdiff  # noqa: E402
from ertdiff import solver as S  # noqa: E402

B, L, K = 64, 4693, 50


def windows_ms(fn, windows, scale=1.0):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * scale)
    return {"min": float(np.min(out)), "median": float(np.median(out)), "max": float(np.max(out)),
            "windows": len(out)}


def per(row, n):
    return {k: (v / n if k != "windows" else v) for k, v in row.items()}


def alternating_ms(fns, windows):
    """One window of each callable in turn, `windows` rounds, the order rotated
    by one every round: the rows share whatever drift (clocks, other tenants)
    the run sees, and no row always runs after the same neighbour."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    keys = list(fns)
    for r in range(windows):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[k]()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1))
    out["sampler_all"] = out["sampler"] + out["sampler_repeat"]
    return {k: {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v)),
                "windows": len(v)} for k, v in out.items()}


def unet_rows(dev, windows, long_windows):
    T = 1000
    m = ertdiff.ConditionalUNet.from_config("U2", seed=0).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    cond = torch.rand(B, 14, L, generator=g).to(dev)
    betas, alphas, ab = ertdiff.get_diffusion_schedule(T)
    anc = ertdiff.UNetSamplerPlan(m, cond, T, betas, alphas, ab, B=B, seed=3)
    x_T = ertdiff.philox_normal(B, m.param_dim, T, 1, 3, 0, dev)
    plans = {s: ertdiff.UNetSolverPlan(m, cond, T, ab, steps=K, solver=s, B=B, seed=3)
             for s in ("ddim", "dpmpp_2m")}

    def anc_steps(n=None):
        anc.x.copy_(x_T)
        anc.launch(n_steps=n)

    def solver_chain(plan):
        def run():
            plan.x.copy_(x_T)
            plan.launch()
        return run

    # the ancestral plan takes two places in the rotation: the gap between its
    # own two rows is what the run cannot resolve between any two plans
    fns = {"sampler": lambda: anc_steps(K)}
    for i, (s, plan) in enumerate(plans.items()):
        assert plan.K == K
        fns[s] = solver_chain(plan)
        if i == 0:
            fns["sampler_repeat"] = lambda: anc_steps(K)
    rows = alternating_ms(fns, windows)
    out = {"shape": {"config": "U2", "B": B, "L": L, "precision": "fp32", "K": K, "T": T},
           "windows": "one window of each row in turn, order rotated every round (head graph + 50 "
                      "steps each); UNetSamplerPlan runs twice per round (per_step_ms / "
                      "per_step_ms_repeat, both together in per_step_ms_all)"}
    out["sampler_plan"] = {"per_step_ms": per(rows["sampler"], K),
                           "per_step_ms_repeat": per(rows["sampler_repeat"], K),
                           "per_step_ms_all": per(rows["sampler_all"], K),
                           "chain_T1000_ms": windows_ms(anc_steps, long_windows)}
    sp = out["sampler_plan"]
    sp["chain_T1000_per_step_ms"] = per(sp["chain_T1000_ms"], T)
    for s in plans:
        r = {"chain_ms": rows[s], "per_step_ms": per(rows[s], K)}
        med = r["per_step_ms"]["median"]
        r["per_step_median_within_sampler_spread"] = bool(
            sp["per_step_ms_all"]["min"] <= med <= sp["per_step_ms_all"]["max"])
        r["per_step_median_vs_sampler_median"] = med / sp["per_step_ms_all"]["median"]
        r["chain_speedup_vs_T1000"] = sp["chain_T1000_ms"]["median"] / r["chain_ms"]["median"]
        out[f"solver_plan_{s}"] = r
        plans[s].close()
    anc.close()
    return out


def reference_rows(dev, windows):
    T, P = 500, 29
    torch.manual_seed(2)
    m = ertdiff.ConditionalDiffusionModel(P, 128).to(dev).eval()
    g = torch.Generator().manual_seed(4)
    cond = torch.rand(B, 14, L, generator=g).to(dev)
    betas, alphas, ab = ertdiff.get_diffusion_schedule(T)
    x_T = ertdiff.philox_normal(B, P, T, 1, 5, 0, dev)
    out = {"shape": {"B": B, "L": L, "P": P, "K": K, "T": T, "precision": "fp32"}}

    def hoisted(n_run):
        plan = ertdiff.SamplerPlan(m, cond, T, betas, alphas, ab, mode="hoisted", n_run=n_run, seed=5)

        def run():
            plan.x.copy_(x_T)
            plan.enqueue_direct()
        row = windows_ms(run, windows, 1e3)
        plan.close()
        return row

    whole, one = hoisted(T), hoisted(1)
    out["hoisted_T500"] = {"chain_us": whole, "one_step_call_us": one,
                           "kernel_us_per_step": (whole["median"] - one["median"]) / (T - 1),
                           "kernel_us_per_step_spread": [(whole["min"] - one["median"]) / (T - 1),
                                                         (whole["max"] - one["median"]) / (T - 1)]}
    # eta = 1 draws a Philox z every step, as the ancestral kernel does; the
    # eta = 0 rows (s_k = 0) draw none
    for name, solver, eta in (("ddim", "ddim", 0.0), ("ddim_eta1", "ddim", 1.0),
                              ("dpmpp_2m", "dpmpp_2m", 0.0)):
        tab = S._Tables(T, ab, K, None, solver, eta, 1.0, dev)
        d_prev = torch.zeros_like(x_T)
        x = torch.empty_like(x_T)

        def seg(n_run):
            def run():
                x.copy_(x_T)
                S.reference_solver_segment(m, cond, 14 * L, tab, x, d_prev, 0, n_run, seed=5)
            return windows_ms(run, windows, 1e3)

        whole, one = seg(K), seg(1)
        out[f"solver_{name}_K50"] = {
            "chain_us": whole, "one_step_call_us": one,
            "kernel_us_per_step": (whole["median"] - one["median"]) / (K - 1),
            "kernel_us_per_step_spread": [(whole["min"] - one["median"]) / (K - 1),
                                          (whole["max"] - one["median"]) / (K - 1)],
            "chain_speedup_vs_T500": out["hoisted_T500"]["chain_us"]["median"] / whole["median"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_probe.json"))
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--long-windows", type=int, default=3, help="windows of the T = 1000 chain")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev),
           "unet": unet_rows(dev, a.windows, a.long_windows),
           "reference": reference_rows(dev, a.windows)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
