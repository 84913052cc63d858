"""Data contract and post-processing around the hot path (SURVEY.md 8a row a13,
8f rows 2-3).  These are host-side transforms the reference applies before
training and after sampling; they are not part of the device hot path.

  transform_to_unconstrained / inverse_transform   ERT_Conditional_Diffusion.py:26-53
  DiffusionDataset                                 :55-78
  check_param_bounds                               :183-218
  load_best_model / save_checkpoint                :345-353, :369-375
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch.utils.data import Dataset, Subset

_EPS = 1e-6


def transform_to_unconstrained(x, a, b):
    """[a,b] -> R logit with clamp eps=1e-6 (:26-40); tensor or ndarray."""
    if isinstance(x, torch.Tensor):
        xn = torch.clamp((x - a) / (b - a), min=_EPS, max=1 - _EPS)
        return torch.log(xn / (1 - xn))
    xn = np.clip((x - a) / (b - a), _EPS, 1 - _EPS)
    return np.log(xn / (1 - xn))


def inverse_transform(u, a, b):
    """Sigmoid back to [a,b] (:42-53); tensor or ndarray."""
    if isinstance(u, torch.Tensor):
        return a + (b - a) * torch.sigmoid(u)
    return a + (b - a) * (1 / (1 + np.exp(-u)))


class DiffusionDataset(Dataset):
    """(params (N,29[,1]), ert (N,4693,14)) -> (logit params (29,), cond (14,4693)).

    Same contract as the reference (:55-78).  ``a``/``b`` are explicit here
    (the reference reads module globals a, b = 0, 1 set at :230).  The
    condition is stored transposed as a view; default collation makes each
    batch a contiguous (B,14,L) tensor, which is what the kernels read.
    """

    def __init__(self, sim_param, ert_sim, a: float = 0.0, b: float = 1.0):
        if sim_param.ndim == 3 and sim_param.shape[2] == 1:
            raw = np.squeeze(sim_param, axis=2)
        else:
            raw = sim_param.copy()
        self.params = transform_to_unconstrained(torch.from_numpy(raw).float(), a, b)
        self.conditions = torch.from_numpy(np.transpose(ert_sim, (0, 2, 1))).float()

    def __len__(self):
        return self.params.shape[0]

    def __getitem__(self, idx):
        return self.params[idx], self.conditions[idx]


class DeviceDataset:
    """The whole dataset resident on one device: x0 (N, P) and cond (N, 14, L)
    as contiguous float32 tensors.  TrainPlan.run_epoch / ValidationPlan.run read
    their batches out of it through a row index, so an epoch needs no
    per-batch gather or copy (the reference's 5076 x 14 x 4693 floats are
    1.33 GB).  Works on CPU tensors too (nothing here launches a kernel)."""

    def __init__(self, x0: torch.Tensor, cond: torch.Tensor):
        if x0.dtype != torch.float32 or cond.dtype != torch.float32:
            raise RuntimeError(f"ertdiff: DeviceDataset holds float32 (got {x0.dtype}, {cond.dtype})")
        if x0.dim() != 2 or cond.dim() != 3 or cond.shape[0] != x0.shape[0] or cond.shape[1] != 14:
            raise RuntimeError("ertdiff: DeviceDataset takes x0 (N, P) and cond (N, 14, L), got "
                               f"{tuple(x0.shape)} and {tuple(cond.shape)}")
        if x0.device != cond.device:
            raise RuntimeError(f"ertdiff: x0 on {x0.device}, cond on {cond.device}")
        self.x0 = x0.contiguous()
        self.cond = cond.contiguous()

    def __len__(self):
        return self.x0.shape[0]

    @property
    def device(self):
        return self.x0.device

    @classmethod
    def from_dataset(cls, ds, device=None):
        """Stack a DiffusionDataset, or a torch.utils.data.Subset of one (nested
        subsets too), once: row i is bitwise what ds[i] returns, and the
        transposed (non-contiguous) ERT view is made contiguous."""
        idx = None
        while isinstance(ds, Subset):
            sub = torch.as_tensor(ds.indices, dtype=torch.int64)
            idx = sub if idx is None else sub[idx]
            ds = ds.dataset
        if not isinstance(ds, DiffusionDataset):
            raise RuntimeError("ertdiff: DeviceDataset.from_dataset takes a DiffusionDataset or a "
                               f"Subset of one, got {type(ds).__name__}")
        x0, cond = ds.params, ds.conditions
        if idx is not None:
            x0, cond = x0[idx], cond[idx]
        if device is not None:   # the copy is made contiguous on the host first: one plain transfer
            x0, cond = x0.contiguous().to(device), cond.contiguous().to(device)
        return cls(x0, cond)


def bounds_mask(param: np.ndarray, limits: np.ndarray) -> np.ndarray:
    """Row validity of (n, P) parameter sets against (P, 2) [min, max] limits:
    rejected when some value is < min or > max (:205-207; a NaN passes)."""
    lo, hi = limits[:, 0], limits[:, 1]
    return ~np.any((param < lo) | (param > hi), axis=1)


def check_param_bounds(param: np.ndarray, limits: np.ndarray, verbose: bool = True) -> Optional[np.ndarray]:
    """Keep only parameter sets inside the limits (:183-218); None if none are."""
    mask = bounds_mask(param, limits)
    if verbose:
        lo, hi = limits[:, 0], limits[:, 1]
        for i in np.nonzero(~mask)[0]:
            bad = np.nonzero((param[i] < lo) | (param[i] > hi))[0][0]
            print(f"Sample {i} Parameter {bad}: {param[i, bad]:.4f} "
                  f"(out of bounds [{lo[bad]:.4f}, {hi[bad]:.4f}])")
    if not mask.any():
        return None
    return np.stack(list(param[mask]))


def save_checkpoint(path, model, optimizer, epoch: int, best_val_loss: float,
                    train_history, val_history, param_dim: int) -> None:
    """The reference's best-model dict format (:345-353)."""
    torch.save({
        "epoch": epoch,
        "model_state_dict": model.state_dict(),
        "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else {},
        "best_val_loss": best_val_loss,
        "train_history": list(train_history),
        "val_history": list(val_history),
        "param_dim": param_dim,
    }, path)


def load_best_model(path, model, optimizer=None, map_location=None):
    """Restore model (+ optimizer) from a reference-format checkpoint (:369-375).
    Loaded with weights_only=True: the dict holds tensors, ints, floats, lists."""
    ckpt = torch.load(path, map_location=map_location, weights_only=True)
    model.load_state_dict(ckpt["model_state_dict"])
    if optimizer is not None and "optimizer_state_dict" in ckpt:
        optimizer.load_state_dict(ckpt["optimizer_state_dict"])
    print(f'Loaded best model from epoch {ckpt["epoch"]} with val loss {ckpt["best_val_loss"]:.6f}')
    return ckpt
