"""Time the data-preparation kernels (csrc/dataprep.hip) and prepare_dataset at
the reference's shape, ert_sim (5076, 4693, 14) float64 and sim_param
(5076, 29, 1), beside the host chain the reference runs
(ERT_Conditional_Diffusion.py:230-269: MinMaxScaler.fit_transform,
DiffusionDataset's transpose and .float(), then the copy to the device),
measured in the same run on the same box.

    python tools/dataprep_probe.py [--out profiles/dataprep_probe.json] [--rows 5076]
                                   [--repeats 7] [--inner 5] [--chunk-rows 512]

Kernel times are HIP events around `inner` back-to-back calls of the C entry
point on preallocated buffers after a warm call; each of `repeats` windows
gives one per-call time, reported as min / median / max.  Bytes moved: the fit
reads the array once; the condition build reads it once and writes the
float32 conditions.  The yardstick is the measured float4 copy rate of the
MI355X, 6.29 TB/s (8.0 TB/s specified).  End-to-end rows are host wall time
of the public call from host arrays to a finished DeviceDataset, transfer and
synchronisation included.
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ertdiff  # noqa: E402
from ertdiff import _lib  # noqa: E402
import dataprep_ref  # noqa: E402

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29


def spread(us):
    return {"min_us": float(np.min(us)), "median_us": float(np.median(us)), "max_us": float(np.max(us)),
            "windows": len(us)}


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


def wall_time(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return spread(out)


def kernel_row(name, t, read_bytes, write_bytes):
    moved = read_bytes + write_bytes
    r = {"name": name, "time": t, "read_bytes": int(read_bytes), "write_bytes": int(write_bytes),
         "TBps": moved / t["median_us"] / 1e6,
         "share_of_hbm_copy": moved / t["median_us"] / 1e6 / HBM_COPY_TBS,
         "share_of_hbm_spec": moved / t["median_us"] / 1e6 / HBM_SPEC_TBS}
    print(json.dumps(r), flush=True)
    return r


def host_chain(sim_param, ert_sim, dev):
    """The reference's lines on the host, then DeviceDataset.from_dataset."""
    N = ert_sim.shape[0]
    try:
        from sklearn.preprocessing import MinMaxScaler
        ps, es = MinMaxScaler(feature_range=(0.0, 1.0)), MinMaxScaler(feature_range=(0, 1))
        par = ps.fit_transform(sim_param.reshape(N, -1)).reshape(sim_param.shape)
        ert = es.fit_transform(ert_sim.reshape(N, -1)).reshape(ert_sim.shape)
        how = "sklearn"
    except ImportError:
        fp = dataprep_ref.fit(sim_param.reshape(N, -1), (0.0, 1.0))
        fe = dataprep_ref.fit(ert_sim.reshape(N, -1), (0, 1))
        par = dataprep_ref.transform(sim_param.reshape(N, -1), fp["scale_"], fp["min_"]).reshape(sim_param.shape)
        ert = dataprep_ref.transform(ert_sim.reshape(N, -1), fe["scale_"], fe["min_"]).reshape(ert_sim.shape)
        how = "numpy"
    ds = ertdiff.DeviceDataset.from_dataset(ertdiff.DiffusionDataset(par, ert), dev)
    return ds, how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataprep_probe.json"))
    ap.add_argument("--rows", type=int, default=5076)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--chunk-rows", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(torch.zeros(1, device=dev))
    N, L, C, P = a.rows, 4693, 14, 29
    F = L * C
    rng = np.random.default_rng(0)
    ert_sim = np.exp(2.3 * rng.standard_normal((N, L, C), dtype=np.float32)).astype(np.float64)
    ert_sim *= 1.0 + 2.0 ** -30 * rng.integers(0, 1 << 20, (1, L, C))     # full float64 mantissas
    sim_param = np.exp(rng.standard_normal((N, P, 1)))
    rows = []

    # the kernels alone, on a resident copy
    lib, s = _lib.lib(), _lib.stream_of(dev)
    d = torch.from_numpy(ert_sim.reshape(N, F)).to(dev)
    vec = torch.empty(5, F, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.ertd_minmax_ws_bytes(N, F), dtype=torch.uint8, device=dev)
    cond = torch.empty(N, C, L, dtype=torch.float32, device=dev)
    back = torch.empty(N, L, C, dtype=torch.float32, device=dev)

    def fit_dev():
        _lib.check(lib.ertd_minmax_partial_fit(d.data_ptr(), N, F, F, vec[2].data_ptr(), vec[3].data_ptr(), 0,
                                               ws.data_ptr(), ws.numel(), s), "minmax_partial_fit")
        _lib.check(lib.ertd_minmax_finalize(vec[2].data_ptr(), vec[3].data_ptr(), F, 0.0, 1.0, vec[0].data_ptr(),
                                            vec[1].data_ptr(), vec[4].data_ptr(), s), "minmax_finalize")

    def cond_dev():
        _lib.check(lib.ertd_minmax_cond(d.data_ptr(), N, L, C, vec[0].data_ptr(), vec[1].data_ptr(),
                                        cond.data_ptr(), s), "minmax_cond")

    def inv_dev():
        _lib.check(lib.ertd_minmax_cond_inverse(cond.data_ptr(), N, L, C, vec[0].data_ptr(), vec[1].data_ptr(),
                                                back.data_ptr(), s), "minmax_cond_inverse")

    raw_bytes = N * F * 8
    rows.append(kernel_row(f"fit: column min/max + finalize ({N}, {F}) f64", device_time(fit_dev, a.repeats, a.inner),
                           raw_bytes + ws.numel(), ws.numel() + 5 * F * 8))
    rows.append(kernel_row(f"condition build ({N}, {L}, {C}) f64 -> ({N}, {C}, {L}) f32",
                           device_time(cond_dev, a.repeats, a.inner), raw_bytes + 2 * F * 8, N * F * 4))
    rows.append(kernel_row(f"condition inverse ({N}, {C}, {L}) f32 -> ({N}, {L}, {C}) f32",
                           device_time(inv_dev, a.repeats, a.inner), N * F * 4 + 2 * F * 8, N * F * 4))
    copy = torch.empty_like(d)
    rows.append(kernel_row(f"torch copy_ of the same ({N}, {F}) f64 array (same-run yardstick)",
                           device_time(lambda: copy.copy_(d), a.repeats, a.inner), raw_bytes, raw_bytes))
    kernels_cond = cond.clone()
    del d, copy, back, ws
    torch.cuda.empty_cache()

    # end to end from host arrays
    e2e = {}
    keep = {}

    def run(key, **kw):
        keep[key] = ertdiff.prepare_dataset(sim_param, ert_sim, dev, **kw)[0]

    e2e["prepare_dataset"] = wall_time(lambda: run("whole"), a.host_repeats)
    e2e[f"prepare_dataset chunk_rows={a.chunk_rows}"] = wall_time(lambda: run("chunked", chunk_rows=a.chunk_rows),
                                                                  a.host_repeats)
    same_chunked = bool(torch.equal(keep["whole"].cond.view(torch.int32), keep["chunked"].cond.view(torch.int32))
                        and torch.equal(keep["whole"].x0.view(torch.int32), keep["chunked"].x0.view(torch.int32)))
    same_kernels = bool(torch.equal(keep["whole"].cond.view(torch.int32), kernels_cond.view(torch.int32)))
    t0 = time.perf_counter()
    hd = torch.from_numpy(ert_sim.reshape(N, F)).to(dev)
    torch.cuda.synchronize()
    e2e["host_to_device copy of ert_sim alone (pageable)"] = spread([(time.perf_counter() - t0) * 1e6])
    del hd, kernels_cond
    keep.pop("chunked")
    torch.cuda.empty_cache()
    host = {}
    how = [None]

    def run_host():
        host["ds"], how[0] = host_chain(sim_param, ert_sim, dev)

    e2e["host chain"] = wall_time(run_host, a.host_repeats)
    same_host = bool(torch.equal(keep["whole"].cond.view(torch.int32), host["ds"].cond.view(torch.int32))
                     and torch.equal(keep["whole"].x0.view(torch.int32), host["ds"].x0.view(torch.int32)))
    for k, v in e2e.items():
        print(json.dumps({"name": k, "wall": v}), flush=True)

    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "shape": {"ert_sim": [N, L, C], "sim_param": [N, P, 1]}, "repeats": a.repeats, "inner": a.inner,
           "host_repeats": a.host_repeats, "host_threads": torch.get_num_threads(),
           "host_cpus": len(os.sched_getaffinity(0)), "host_chain": how[0],
           "hbm_spec_TBps": HBM_SPEC_TBS, "hbm_copy_TBps": HBM_COPY_TBS, "kernels": rows, "end_to_end": e2e,
           "speedup_vs_host_chain_median": e2e["host chain"]["median_us"] / e2e["prepare_dataset"]["median_us"],
           "chunked_equals_whole": same_chunked, "prepare_dataset_equals_kernels": same_kernels,
           "device_equals_host_chain": same_host}
    print(json.dumps({k: res[k] for k in ("speedup_vs_host_chain_median", "chunked_equals_whole",
                                          "prepare_dataset_equals_kernels", "device_equals_host_chain")}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
