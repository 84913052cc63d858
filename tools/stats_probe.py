"""Time the ensemble-statistics kernels (csrc/ensstats.hip) and the row sort /
Wasserstein distance (csrc/rowsort.hip) at the reference's shapes, beside two
baselines measured in the same run on the same box:

  * the reference's numpy / scipy formulation on the host, and
  * a torch.sort + gather composition of the same percentiles on the same GPU
    (torch.sort of the same rows; torch.sort + torch.searchsorted for the
    distance).

    python tools/stats_probe.py [--out profiles/stats_probe.json] [--repeats 9] [--inner 20]

Device times are HIP events around `inner` back-to-back calls after a warm
call; each of `repeats` windows gives one per-call time, reported as
min / median / max.  `api` rows time the public function (coverage_curve
returns host counts, so it ends in a copy and a synchronise; its torch
counterpart does the same) and include the host's share of a call; `device`
rows call the C entry points on preallocated buffers: the kernels alone.  Achieved input
bandwidth = input bytes / median device time, against the HBM figures of the
MI355X (8.0 TB/s specified, 6.29 TB/s measured for a float4 copy).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ert-conditional-diffusion-model_amd"))
import ertdiff  # noqa: E402
from ertdiff import _lib, stats  # noqa: E402

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29
PROB = np.linspace(0.01, 0.99, 30)


def device_time(fn, repeats, inner):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner * 1e3)
    return spread(out)


def host_time(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return spread(out)


def spread(us):
    return {"min_us": float(np.min(us)), "median_us": float(np.median(us)), "max_us": float(np.max(us)),
            "windows": len(us)}


def lerp_rows(srt, q):
    """numpy's linear percentile from a column-sorted (n, cells) tensor: the
    row indices and weights are the same for every column."""
    n = srt.shape[0]
    vi = (n - 1) * torch.as_tensor(q, dtype=torch.float64, device=srt.device)
    lo = vi.floor().long().clamp(0, n - 1)
    hi = (lo + 1).clamp(max=n - 1)
    t = (vi - lo).unsqueeze(1)
    a, b = srt.index_select(0, lo), srt.index_select(0, hi)
    d = (b - a).double()
    return torch.where(t < 0.5, a.double() + d * t, b.double() - d * (1 - t))


def torch_coverage(gen, true, q_low, q_upp):
    S, N, P = gen.shape
    srt = torch.sort(gen.reshape(S, N * P), dim=0).values
    low, upp = lerp_rows(srt, q_low), lerp_rows(srt, q_upp)
    t = true.reshape(1, N * P).double()
    hit = (low < t) & (t <= upp)
    return hit.reshape(-1, N, P).sum(dim=1, dtype=torch.int32)


def torch_summary(x):
    n = x.shape[0]
    flat = x.reshape(n, -1)
    srt = torch.sort(flat, dim=0).values
    pct = lerp_rows(srt, [0.25, 0.5, 0.75])
    mean = flat.mean(dim=0)
    var = flat.var(dim=0, unbiased=False)
    std = var.sqrt()
    return mean, std, var, pct, std / (mean.abs() + 1e-8)


def torch_wsse(sim, obs, A=0.1, B=0.01):
    return ((sim - obs) ** 2 / (A * obs.abs() + B) ** 2).mean(dim=1)


def numpy_coverage(gen, true):
    avg = np.zeros(len(PROB))
    for k, p in enumerate(PROB):
        low = np.percentile(gen, (1 - p) / 2 * 100, axis=0)
        upp = np.percentile(gen, (1 + p) / 2 * 100, axis=0)
        avg[k] = np.mean(((low < true) & (true <= upp)).astype(int))
    return avg


def numpy_summary(x):
    mean, std, var = np.mean(x, axis=0), np.std(x, axis=0), np.var(x, axis=0)
    p = [np.percentile(x, q, axis=0) for q in (25, 50, 75)]
    return mean, std, var, p, std / (np.abs(mean) + 1e-8)


def numpy_wsse(sim, obs, A=0.1, B=0.01):
    out = np.empty((sim.shape[0], sim.shape[2]))
    for s in range(sim.shape[0]):
        for e in range(sim.shape[2]):
            o = obs[:, e]
            out[s, e] = np.average((sim[s][:, e] - o) ** 2 / (A * np.abs(o) + B) ** 2)
    return out


def torch_wasserstein(u, v):
    """scipy's _cdf_distance(p = 1) of every row of u (n, M) against v, composed
    of torch.sort and torch.searchsorted."""
    n = u.shape[0]
    us, vs = torch.sort(u, dim=1).values, torch.sort(v).values
    allv = torch.sort(torch.cat([u, v.expand(n, -1)], dim=1), dim=1).values
    head = allv[:, :-1].contiguous()
    deltas = allv[:, 1:] - head
    u_cdf = torch.searchsorted(us, head, right=True).double() / u.shape[1]
    v_cdf = torch.searchsorted(vs, head, right=True).double() / v.shape[0]
    return ((u_cdf - v_cdf).abs() * deltas).sum(dim=1)


def scipy_wasserstein(sim, obs):
    from scipy.stats import wasserstein_distance
    return [wasserstein_distance(s.flatten(), obs.flatten()) for s in sim]


def row(name, ours, torch_row, numpy_row, in_bytes, extra=None):
    med = ours["median_us"]
    r = {"name": name, "ertdiff": ours, "torch_sort_composition": torch_row, "numpy_host": numpy_row,
         "input_bytes": int(in_bytes), "input_GBps": in_bytes / med / 1e3,
         "share_of_hbm_spec": in_bytes / med / 1e6 / HBM_SPEC_TBS,
         "share_of_hbm_copy": in_bytes / med / 1e6 / HBM_COPY_TBS,
         "speedup_vs_torch_median": torch_row["median_us"] / med if torch_row else None,
         "speedup_vs_numpy_median": numpy_row["median_us"] / med if numpy_row else None}
    r.update(extra or {})
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_probe.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(torch.zeros(1, device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    R, I = a.repeats, a.inner
    rows = []

    # calibration: Uncertainty_params (50, 509, 29) float32
    S, N, P = 50, 509, 29
    centre = torch.randn(N, P, generator=g, device=dev) + 4.0
    gen = centre + 0.3 * torch.randn(S, N, P, generator=g, device=dev)
    true = centre + 0.3 * torch.randn(N, P, generator=g, device=dev)
    q_low, q_upp = stats.interval_fractions(PROB)
    ql, qu = torch.from_numpy(q_low).to(dev), torch.from_numpy(q_upp).to(dev)
    counts = torch.empty(30, P, dtype=torch.int32, device=dev)
    cols = torch.empty(P, dtype=torch.int32, device=dev)
    lib, s = _lib.lib(), _lib.stream_of(dev)

    def cov_dev():
        _lib.check(lib.ertd_coverage(gen.data_ptr(), true.data_ptr(), 0, S, N, P, None, ql.data_ptr(),
                                     qu.data_ptr(), 30, counts.data_ptr(), cols.data_ptr(), s), "coverage")

    cov_dev()
    same = bool(torch.equal(counts, torch_coverage(gen, true, q_low, q_upp)))
    gn, tn = gen.cpu().numpy(), true.cpu().numpy()
    cov_np = host_time(lambda: numpy_coverage(gn, tn), a.host_repeats)
    in_bytes = gen.numel() * 4 + true.numel() * 4
    rows.append(row("coverage (50,509,29) f32, device", device_time(cov_dev, R, I),
                    device_time(lambda: torch_coverage(gen, true, q_low, q_upp), R, I), cov_np, in_bytes,
                    {"counts_equal_torch_composition": same}))
    rows.append(row("coverage_curve (50,509,29) f32, api", device_time(lambda: ertdiff.coverage_curve(gen, true), R, I),
                    device_time(lambda: torch_coverage(gen, true, q_low, q_upp).cpu(), R, I), cov_np, in_bytes))

    # simulated ensemble (100, 4693, 14) float64
    n, M, E = 100, 4693, 14
    loc = torch.rand(M, E, generator=g, device=dev, dtype=torch.float64) * 40 + 2
    x = loc + (torch.rand(M, E, generator=g, device=dev, dtype=torch.float64) * 2 + 0.05) * \
        torch.randn(n, M, E, generator=g, device=dev, dtype=torch.float64)
    obs = loc * 1.01
    xn, on = x.cpu().numpy(), obs.cpu().numpy()
    ours = ertdiff.ensemble_summary(x)
    ref = torch_summary(x)
    same = bool(torch.equal(ours["percentiles"].reshape(3, -1), ref[3]))
    in_bytes = x.numel() * 8
    rows.append(row("ensemble_summary (100,4693,14) f64, api", device_time(lambda: ertdiff.ensemble_summary(x), R, I),
                    device_time(lambda: torch_summary(x), R, I),
                    host_time(lambda: numpy_summary(xn), a.host_repeats), in_bytes,
                    {"percentiles_equal_torch_composition": same,
                     "note": "input_bytes counts the array once; the summary reads it in two launches"}))
    q3 = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64, device=dev)
    rows.append(row("ensemble_percentile P25/50/75 (100,4693,14) f64, api",
                    device_time(lambda: ertdiff.ensemble_percentile(x, [25, 50, 75]), R, I),
                    device_time(lambda: lerp_rows(torch.sort(x.reshape(n, -1), dim=0).values, q3), R, I),
                    None, in_bytes))
    rows.append(row("ensemble_moments (100,4693,14) f64, api", device_time(lambda: ertdiff.ensemble_moments(x), R, I),
                    device_time(lambda: (x.mean(dim=0), x.var(dim=0, unbiased=False)), R, I), None, in_bytes))
    out3 = torch.empty(3, M * E, dtype=torch.float64, device=dev)
    mean_o, var_o = (torch.empty(M * E, dtype=torch.float64, device=dev) for _ in range(2))
    wout = torch.empty(n, E, dtype=torch.float64, device=dev)

    def pct_dev():
        _lib.check(lib.ertd_ens_percentile(x.data_ptr(), 1, n, M * E, M * E, None, 1, q3.data_ptr(), 3,
                                           out3.data_ptr(), None, s), "ens_percentile")

    def mom_dev():
        _lib.check(lib.ertd_ens_moments(x.data_ptr(), 1, n, M * E, M * E, None, 1, mean_o.data_ptr(),
                                        var_o.data_ptr(), s), "ens_moments")

    def wsse_dev():
        _lib.check(lib.ertd_wsse(x.data_ptr(), obs.data_ptr(), 1, n, M, E, 0.1, 0.01, wout.data_ptr(), s), "wsse")

    rows.append(row("percentiles P25/50/75 (100,4693,14) f64, device", device_time(pct_dev, R, I),
                    device_time(lambda: lerp_rows(torch.sort(x.reshape(n, -1), dim=0).values, q3), R, I),
                    None, in_bytes))
    rows.append(row("moments (100,4693,14) f64, device", device_time(mom_dev, R, I),
                    device_time(lambda: (x.mean(dim=0), x.var(dim=0, unbiased=False)), R, I), None, in_bytes))
    rows.append(row("wsse (100,4693,14) f64, device", device_time(wsse_dev, R, I),
                    device_time(lambda: torch_wsse(x, obs), R, I), None, in_bytes + obs.numel() * 8))
    rows.append(row("wsse (100,4693,14) f64, api", device_time(lambda: ertdiff.wsse(x, obs), R, I),
                    device_time(lambda: torch_wsse(x, obs), R, I),
                    host_time(lambda: numpy_wsse(xn, on), a.host_repeats), in_bytes + obs.numel() * 8,
                    {"note": "torch row: eager elementwise + mean (no sort in WSSE)"}))

    # row sort and Wasserstein-1 of every realisation against the observation (csrc/rowsort.hip)
    Mf = M * E
    xf, of = x.reshape(n, Mf), obs.reshape(Mf)
    srt = torch.empty(n, Mf, dtype=torch.float64, device=dev)
    sort_ws = torch.empty(lib.ertd_rows_sort_ws_bytes(1, n, Mf), dtype=torch.uint8, device=dev)
    w1_ws = torch.empty(lib.ertd_wasserstein_ws_bytes(1, n, Mf, Mf), dtype=torch.uint8, device=dev)
    w1 = torch.empty(n, dtype=torch.float64, device=dev)

    def sort_dev():
        _lib.check(lib.ertd_rows_sort(xf.data_ptr(), 1, n, Mf, Mf, srt.data_ptr(), sort_ws.data_ptr(),
                                      sort_ws.numel(), s), "rows_sort")

    def w1_dev():
        _lib.check(lib.ertd_wasserstein(xf.data_ptr(), 1, n, Mf, Mf, of.data_ptr(), Mf, w1.data_ptr(),
                                        w1_ws.data_ptr(), w1_ws.numel(), s), "wasserstein")

    sort_dev()
    same = bool(torch.equal(srt, torch.sort(xf, dim=1).values))
    torch_sort = device_time(lambda: torch.sort(xf, dim=1), R, I)
    rows.append(row("sort_rows (100,65702) f64, device", device_time(sort_dev, R, I), torch_sort, None,
                    in_bytes, {"equal_torch_sort": same, "note": "torch row: torch.sort(x, dim=1)"}))
    rows.append(row("sort_rows (100,65702) f64, api", device_time(lambda: ertdiff.sort_rows(xf), R, I),
                    torch_sort, host_time(lambda: np.sort(xn.reshape(n, Mf), axis=1), a.host_repeats), in_bytes))
    w1_dev()
    tw = torch_wasserstein(xf, of)
    rel = float(((w1 - tw).abs() / tw.abs()).max())
    try:
        sp = host_time(lambda: scipy_wasserstein(xn, on), a.host_repeats)
        sp_rel = float(np.max(np.abs(w1.cpu().numpy() - np.array(scipy_wasserstein(xn, on))) / tw.cpu().numpy()))
    except ImportError:
        sp, sp_rel = None, None
    torch_w1 = device_time(lambda: torch_wasserstein(xf, of), R, I)
    note = {"max_rel_diff_vs_torch_composition": rel, "max_rel_diff_vs_scipy": sp_rel,
            "note": "torch row: torch.sort + torch.searchsorted composition; numpy row: scipy's loop over "
                    "the 100 realisations on the host"}
    rows.append(row("wasserstein (100,4693,14) vs (4693,14) f64, device", device_time(w1_dev, R, I),
                    torch_w1, sp, in_bytes + of.numel() * 8, note))
    rows.append(row("wasserstein (100,4693,14) vs (4693,14) f64, api",
                    device_time(lambda: ertdiff.wasserstein(x, obs), R, I), torch_w1, sp,
                    in_bytes + of.numel() * 8))

    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH), "repeats": R, "inner": I, "host_threads": torch.get_num_threads(),
           "hbm_spec_TBps": HBM_SPEC_TBS, "hbm_copy_TBps": HBM_COPY_TBS, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
