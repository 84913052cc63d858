"""Time a training epoch and a validation epoch from a device-resident dataset
(TrainPlan.run_epoch, ValidationPlan.run) at the reference's shapes -- B = 32,
L = 4693, 127 batches over 4060 rows (126 full + one of 28); 507 validation rows
(15 full batches + one of 27) -- beside, in the same run on the same box:

  (a) plan.run_epoch(data, order)                      one graph replay per epoch
  (b) plan.run(127) on one constant batch              the README's steps/s basis
  (c) the loop a user writes without run_epoch: index_select into plan.x0 /
      plan.cond, then plan.step(return_tensor=True), per batch (126 full
      batches; the partial one would need a second plan)
  validation: ValidationPlan.run against validation_loss(model, x0[idx], cond[idx], ...)
      per batch (its loss.item() host sync included, as the reference loop has it)

    python tools/epoch_probe.py [--out profiles/epoch_probe.json] [--repeats 9] [--inner 10]

Times are HIP events around `inner` back-to-back epochs after a warm epoch
(every graph captured, every shape warm); each of `repeats` windows gives one
per-step time, reported as min / median / max.  The three train variants are
timed alternately, window by window, so drift of the box hits all alike.  The
dataset is synthetic (seeded); the order is a fresh permutation per epoch.
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
from ertdiff import _lib  # noqa: E402

B, L, P, T = 32, 4693, 29, 500
N_TRAIN, N_VAL = 4060, 507


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3   # us per call of fn


def spread(us):
    return {"min_us": float(np.min(us)), "median_us": float(np.median(us)), "max_us": float(np.max(us)),
            "windows": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_probe.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(torch.zeros(1, device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    n_all = N_TRAIN + N_VAL
    data = ertdiff.DeviceDataset(torch.randn(n_all, P, device=dev, generator=g) * 2,
                                 torch.rand(n_all, 14, L, device=dev, generator=g))
    train_idx = torch.arange(N_TRAIN, device=dev)
    val_idx = torch.arange(N_TRAIN, n_all, device=dev)
    _, _, ab = ertdiff.get_diffusion_schedule(T, device=dev)
    torch.manual_seed(42)
    model = ertdiff.ConditionalDiffusionModel(P, 128).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    plan = ertdiff.TrainPlan(model, opt, B, L, T, ab, seed=1234)
    val = ertdiff.ValidationPlan(model, B, L, T, ab, seed=1234)
    nb = -(-N_TRAIN // B)
    nb_val = -(-N_VAL // B)
    nfull = N_TRAIN // B

    def order():
        return train_idx[torch.randperm(N_TRAIN, device=dev, generator=g)]

    def epoch():                  # (a)
        plan.run_epoch(data, order())

    def constant():               # (b)
        plan.run(nb)

    def user_loop():              # (c)
        o = order()
        for i in range(nfull):
            idx = o[i * B:(i + 1) * B]
            torch.index_select(data.x0, 0, idx, out=plan.x0)
            torch.index_select(data.cond, 0, idx, out=plan.cond)
            plan.step(return_tensor=True)

    def val_epoch():
        val.run(data, val_idx)

    def val_loop():
        model.eval()
        for i in range(nb_val):
            idx = val_idx[i * B:(i + 1) * B]
            ertdiff.validation_loss(model, data.x0[idx], data.cond[idx], T, ab)
        model.train()

    plan.x0.copy_(data.x0[:B])
    plan.cond.copy_(data.cond[:B])
    for fn in (epoch, constant, user_loop, val_epoch, val_loop):   # warm: graphs, shapes
        fn()
    torch.cuda.synchronize()
    t_epoch, t_const, t_user, t_val, t_vloop = [], [], [], [], []
    for _ in range(a.repeats):
        t_epoch.append(window(epoch, a.inner) / nb)
        t_const.append(window(constant, a.inner) / nb)
        t_user.append(window(user_loop, a.inner) / nfull)
        t_val.append(window(val_epoch, a.inner) / nb_val)
        t_vloop.append(window(val_loop, a.inner) / nb_val)
    rows = {
        "run_epoch_us_per_step": spread(t_epoch),
        "run_constant_batch_us_per_step": spread(t_const),
        "index_select_plus_step_us_per_step": spread(t_user),
        "validation_plan_us_per_batch": spread(t_val),
        "validation_loss_loop_us_per_batch": spread(t_vloop),
    }
    e, c, u = (rows[k] for k in ("run_epoch_us_per_step", "run_constant_batch_us_per_step",
                                 "index_select_plus_step_us_per_step"))
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "B": B, "L": L, "train_rows": N_TRAIN, "train_batches": nb, "val_rows": N_VAL,
           "val_batches": nb_val, "repeats": a.repeats, "inner": a.inner,
           "dataset_bytes": int(data.x0.numel() * 4 + data.cond.numel() * 4),
           "cond_bytes_per_step": B * 14 * L * 4, **rows,
           "run_epoch_vs_user_loop_median": u["median_us"] / e["median_us"],
           "run_epoch_beats_user_loop_beyond_spread": bool(e["max_us"] < u["min_us"]),
           "run_epoch_vs_constant_batch_median": e["median_us"] / c["median_us"],
           "validation_plan_vs_loop_median": rows["validation_loss_loop_us_per_batch"]["median_us"] /
           rows["validation_plan_us_per_batch"]["median_us"],
           "final_loss_finite": bool(torch.isfinite(plan.loss).item())}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
