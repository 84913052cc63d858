"""Host side of the device-resident epoch (no GPU): DeviceDataset stacking,
the reference's size-weighted epoch mean, and the batch split of an epoch."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Subset, TensorDataset

import ertdiff
from ertdiff.train import batch_sizes
from synth import synth_uniform


def _dataset(N=7, L=11):
    params = synth_uniform((N, 29, 1), 900).astype(np.float32)
    ert = synth_uniform((N, L, 14), 901).astype(np.float32)
    return ertdiff.DiffusionDataset(params, ert)


def _stacked(ds):
    items = [ds[i] for i in range(len(ds))]
    return torch.stack([a for a, _ in items]), torch.stack([c for _, c in items])


def test_from_dataset_equals_stacked_items():
    ds = _dataset()
    assert not ds.conditions.is_contiguous()   # the transposed ERT view
    dd = ertdiff.DeviceDataset.from_dataset(ds)
    x0, cond = _stacked(ds)
    assert len(dd) == len(ds)
    assert dd.x0.dtype == dd.cond.dtype == torch.float32
    assert dd.x0.is_contiguous() and dd.cond.is_contiguous()
    assert tuple(dd.cond.shape) == (7, 14, 11)
    assert torch.equal(dd.x0, x0) and torch.equal(dd.cond, cond)


def test_from_dataset_subset():
    ds = _dataset()
    sub = Subset(ds, [5, 0, 3, 3])
    dd = ertdiff.DeviceDataset.from_dataset(sub, device="cpu")
    x0, cond = _stacked(sub)
    assert torch.equal(dd.x0, x0) and torch.equal(dd.cond, cond)
    assert dd.cond.is_contiguous()
    nested = Subset(sub, [2, 1])   # rows 3, 0 of ds
    dn = ertdiff.DeviceDataset.from_dataset(nested)
    x0n, condn = _stacked(nested)
    assert torch.equal(dn.x0, x0n) and torch.equal(dn.cond, condn)
    with pytest.raises(RuntimeError):
        ertdiff.DeviceDataset.from_dataset(TensorDataset(torch.zeros(3, 2)))
    with pytest.raises(RuntimeError):
        ertdiff.DeviceDataset(torch.zeros(3, 29, dtype=torch.float64), torch.zeros(3, 14, 5))
    with pytest.raises(RuntimeError):
        ertdiff.DeviceDataset(torch.zeros(3, 29), torch.zeros(4, 14, 5))


def test_epoch_loss_partial_last_batch():
    n_rows, B = 11, 4
    losses = torch.tensor([0.75, 1.125, 0.3], dtype=torch.float32)
    ref = (np.float64(losses.numpy().astype(np.float64)) * np.array([4, 4, 3], np.float64)).sum() / 11
    got = ertdiff.epoch_loss(losses, n_rows, B)
    assert isinstance(got, float)
    assert abs(got - ref) <= 1e-15 * abs(ref)
    # the reference's own accumulation (:320-322), in its order
    run = 0.0
    for l, b in zip(losses, (4, 4, 3)):
        run += l.item() * b
    assert got == run / n_rows
    with pytest.raises(RuntimeError):
        ertdiff.epoch_loss(losses[:2], n_rows, B)


@pytest.mark.parametrize("n_rows", [1, 4, 11, 4060])
@pytest.mark.parametrize("B", [4, 32])
def test_batch_split_matches_dataloader(n_rows, B):
    loader = DataLoader(TensorDataset(torch.arange(n_rows)), batch_size=B, shuffle=False)
    sizes = [b[0].shape[0] for b in loader]
    assert batch_sizes(n_rows, B) == sizes
    assert sum(sizes) == n_rows
