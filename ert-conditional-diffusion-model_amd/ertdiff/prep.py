"""Loading and scaling on the device.

The reference prepares its training set on the host
(ERT_Conditional_Diffusion.py:230-274): two sklearn MinMaxScaler.fit_transform
calls -- the (5076, 65702) float64 ERT array and the (5076, 29) parameters --
then DiffusionDataset's transpose to (N, 14, L) and .float(), then
random_split.  At :417-419 the ERT scaler is used once more, backwards, on
float32 test conditions.  Here the scaler's arithmetic runs in HIP kernels
(csrc/dataprep.hip) and reproduces sklearn 1.7 bit for bit: every float64
operation is separately rounded, in sklearn's order.

    DeviceMinMaxScaler(feature_range)      MinMaxScaler with the data on the device
    prepare_dataset(sim_param, ert_sim, device)
                                           -> DeviceDataset, param_scaler, ert_scaler (:230-269)
    split_indices(n, generator)            -> train / val / test indices (:271-274)

Out of scope: float32 input to fit / transform (sklearn would process it in
float32), clip=True, sparse input, other scalers.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .data import DeviceDataset, transform_to_unconstrained

_FITTED = ("scale_", "min_", "data_min_", "data_max_", "data_range_")


def _as_f64(X, what: str) -> torch.Tensor:
    """numpy array or tensor -> float64 tensor (no copy, device unchanged)."""
    if isinstance(X, np.ndarray):
        if X.dtype != np.float64:
            raise RuntimeError(f"ertdiff: {what} must be float64, got {X.dtype}"
                               + _f32_note(X.dtype == np.float32))
        return torch.from_numpy(X)
    if isinstance(X, torch.Tensor):
        if X.dtype != torch.float64:
            raise RuntimeError(f"ertdiff: {what} must be float64, got {X.dtype}"
                               + _f32_note(X.dtype == torch.float32))
        return X.detach()
    raise RuntimeError(f"ertdiff: {what} must be a numpy array or a torch tensor, got {type(X).__name__}")


def _f32_note(is_f32: bool) -> str:
    return (" (sklearn would fit and transform float32 data in float32; that case is not "
            "reproduced here -- pass the raw float64 array)") if is_f32 else ""


def _rows(t: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """A 2-D tensor the kernels can walk: unit column stride, row pitch >= F."""
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, t.stride(0)


class DeviceMinMaxScaler:
    """sklearn.preprocessing.MinMaxScaler (clip=False) on the device.

    Input to partial_fit / fit / transform / transform_cond is float64: a
    device tensor, a host tensor or a numpy array (host data is copied to
    `device`, default the current one).  Results stay on the device.  After a
    fit, scale_, min_, data_min_, data_max_ and data_range_ are numpy float64
    arrays, copied to the host once on first access, so the object can stand
    wherever a fitted sklearn scaler is read (ertdiff.postprocess); the device
    copies serve this object's own launches."""

    def __init__(self, feature_range=(0, 1), device=None):
        fr0, fr1 = feature_range
        if not fr0 < fr1:
            raise RuntimeError(f"ertdiff: feature_range minimum must be below its maximum, got {feature_range}")
        self.feature_range = (fr0, fr1)
        self._device = None if device is None else torch.device(device)
        self._reset()

    def _reset(self):
        self._dv = None          # device: (5, F) float64, rows in _FITTED order
        self._host = None        # host: dict of numpy arrays, filled lazily
        self._ws = None
        self.n_samples_seen_ = 0
        self.n_features_in_ = None

    # ---- fitted attributes -----------------------------------------------------
    def _fitted_host(self) -> dict:
        if self._host is None:
            if self._dv is None:
                raise AttributeError("this DeviceMinMaxScaler is not fitted yet")
            arr = self._dv.cpu().numpy()
            self._host = {k: arr[i].copy() for i, k in enumerate(_FITTED)}
        return self._host

    scale_ = property(lambda self: self._fitted_host()["scale_"])
    min_ = property(lambda self: self._fitted_host()["min_"])
    data_min_ = property(lambda self: self._fitted_host()["data_min_"])
    data_max_ = property(lambda self: self._fitted_host()["data_max_"])
    data_range_ = property(lambda self: self._fitted_host()["data_range_"])

    def _dev_of(self, t: Optional[torch.Tensor] = None) -> torch.device:
        if self._device is None:
            if t is not None and t.is_cuda:
                self._device = t.device
            else:
                if not torch.cuda.is_available():
                    raise RuntimeError("ertdiff runs only on an MI355X (gfx950) device; none is visible")
                self._device = torch.device("cuda", torch.cuda.current_device())
        if self._device.type == "cuda" and self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    def _vectors(self, dev: torch.device) -> torch.Tensor:
        """The (5, F) device block; uploaded from the host copies after from_sklearn."""
        if self._dv is None:
            if self._host is None:
                raise RuntimeError("ertdiff: this DeviceMinMaxScaler is not fitted yet")
            self._dv = torch.from_numpy(np.stack([self._host[k] for k in _FITTED])).to(dev)
        if self._dv.device != dev:
            raise RuntimeError(f"ertdiff: scaler lives on {self._dv.device}, data on {dev}")
        return self._dv

    def _input(self, X, what: str, ndim=(2,)) -> torch.Tensor:
        t = _as_f64(X, what)
        if t.dim() not in ndim:
            raise RuntimeError(f"ertdiff: {what} must have {' or '.join(str(d) for d in ndim)} dimensions, "
                               f"got shape {tuple(t.shape)}")
        if t.numel() == 0:
            raise RuntimeError(f"ertdiff: {what} is empty, shape {tuple(t.shape)}")
        dev = self._dev_of(t)
        if not t.is_cuda:
            t = t.to(dev)
        return t

    def _features(self, F: int):
        if self.n_features_in_ is not None and F != self.n_features_in_:
            raise RuntimeError(f"ertdiff: X has {F} features, the scaler was fitted with {self.n_features_in_}")

    # ---- fitting -----------------------------------------------------------------
    def partial_fit(self, X):
        """MinMaxScaler.partial_fit: fold the rows of X (n, F) into the running
        column minima / maxima and recompute scale_ / min_."""
        t = self._input(X, "X")
        dev = _lib.require_device(t)
        t, ldx = _rows(t)
        n, F = t.shape
        first = self.n_samples_seen_ == 0
        if first:
            self.n_features_in_ = F
            self._dv = torch.empty(5, F, dtype=torch.float64, device=dev)
        else:
            self._features(F)
            self._vectors(dev)
        lib = _lib.lib()
        need = lib.ertd_minmax_ws_bytes(n, F)
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        v = self._dv
        with torch.cuda.device(dev):
            s = _lib.stream_of(dev)
            _lib.check(lib.ertd_minmax_partial_fit(t.data_ptr(), n, F, ldx, v[2].data_ptr(), v[3].data_ptr(),
                                                   0 if first else 1, self._ws.data_ptr(),
                                                   self._ws.numel(), s), "minmax_partial_fit")
            _lib.check(lib.ertd_minmax_finalize(v[2].data_ptr(), v[3].data_ptr(), F,
                                                float(self.feature_range[0]), float(self.feature_range[1]),
                                                v[0].data_ptr(), v[1].data_ptr(), v[4].data_ptr(), s),
                       "minmax_finalize")
        self._host = None
        self.n_samples_seen_ += n
        return self

    def fit(self, X):
        self._reset()
        return self.partial_fit(X)

    # ---- plain (n, F) float64 ------------------------------------------------------
    def transform(self, X, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """X (n, F) float64 -> X * scale_ + min_ (float64, on the device).
        out=X transforms a device tensor in place."""
        t = self._input(X, "X")
        return self._plain(t, out, inverse=False)

    def fit_transform(self, X, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        t = self._input(X, "X")
        return self.fit(t).transform(t, out=out)

    def inverse_transform(self, X, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(X - min_) / scale_ in X's dtype, as sklearn computes it: a float64
        X gets one rounding per operation; a float32 X is rounded to float32
        after the subtraction and again after the division (sklearn applies
        its float64 vectors in place to the float32 array)."""
        if isinstance(X, np.ndarray):
            X = torch.from_numpy(X)
        if not isinstance(X, torch.Tensor) or X.dtype not in (torch.float32, torch.float64):
            raise RuntimeError("ertdiff: inverse_transform takes a float32 or float64 array or tensor")
        t = X.detach()
        if t.dim() != 2 or t.numel() == 0:
            raise RuntimeError(f"ertdiff: X must be a non-empty 2-D array, got shape {tuple(t.shape)}")
        if not t.is_cuda:
            t = t.to(self._dev_of(t))
        return self._plain(t, out, inverse=True)

    def _plain(self, t: torch.Tensor, out, inverse: bool) -> torch.Tensor:
        dev = _lib.require_device(t)
        n, F = t.shape
        self._features(F)
        v = self._vectors(dev)
        if v.shape[1] != F:
            raise RuntimeError(f"ertdiff: X has {F} features, the scaler has {v.shape[1]}")
        t, ldx = _rows(t)
        if out is None:
            out = torch.empty(n, F, dtype=t.dtype, device=dev)
        if (not isinstance(out, torch.Tensor) or out.shape != t.shape or out.dtype != t.dtype
                or out.device != dev or out.stride(1) != 1 or out.stride(0) < F):
            raise RuntimeError("ertdiff: out must be a device tensor shaped and typed like X with unit "
                               "column stride")
        lib = _lib.lib()
        with torch.cuda.device(dev):
            s = _lib.stream_of(dev)
            if inverse:
                _lib.check(lib.ertd_minmax_inverse(t.data_ptr(), 0 if t.dtype == torch.float32 else 1, n, F,
                                                   ldx, v[0].data_ptr(), v[1].data_ptr(), out.data_ptr(),
                                                   out.stride(0), s), "minmax_inverse")
            else:
                _lib.check(lib.ertd_minmax_transform(t.data_ptr(), n, F, ldx, v[0].data_ptr(), v[1].data_ptr(),
                                                     out.data_ptr(), out.stride(0), s), "minmax_transform")
        return out

    # ---- the condition layout --------------------------------------------------------
    def transform_cond(self, X, L: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """transform + DiffusionDataset's transpose + .float() in one pass:
        X (n, L, 14) or (n, L * 14) float64 -> (n, 14, L) float32,
        cond[i, c, l] = float32(X[i, l, c] * scale_ + min_).  `out` may be a
        row slice cond[r0:r1] of a larger (N, 14, L) buffer."""
        t = self._input(X, "X", ndim=(2, 3))
        dev = _lib.require_device(t)
        C = _lib.CIN
        n = t.shape[0]
        F = t.numel() // n
        if t.dim() == 3:
            if t.shape[2] != C or (L is not None and L != t.shape[1]):
                raise RuntimeError(f"ertdiff: X must be (n, L, {C}), got {tuple(t.shape)} with L={L}")
            L = t.shape[1]
        else:
            L = F // C if L is None else int(L)
            if L < 1 or L * C != F:
                raise RuntimeError(f"ertdiff: X has {F} columns, not L * {C} (L={L})")
        self._features(F)
        v = self._vectors(dev)
        if v.shape[1] != F:
            raise RuntimeError(f"ertdiff: X has {F} features, the scaler has {v.shape[1]}")
        t = t.contiguous()
        if out is None:
            out = torch.empty(n, C, L, dtype=torch.float32, device=dev)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, C, L) or out.dtype != torch.float32
                or out.device != dev or not out.is_contiguous()):
            raise RuntimeError(f"ertdiff: out must be a contiguous float32 device tensor of shape ({n}, {C}, {L})")
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ertd_minmax_cond(t.data_ptr(), n, L, C, v[0].data_ptr(), v[1].data_ptr(),
                                                   out.data_ptr(), _lib.stream_of(dev)), "minmax_cond")
        return out

    def inverse_cond(self, cond: torch.Tensor) -> torch.Tensor:
        """The reference's :417-419: cond (n, 14, L) float32 -> (n, L, 14)
        float32 in the scaler's original units, bit for bit
        scaler.inverse_transform(cond.swapaxes(1, 2).reshape(n, -1))."""
        if isinstance(cond, np.ndarray):
            cond = torch.from_numpy(cond)
        if not isinstance(cond, torch.Tensor) or cond.dtype != torch.float32 or cond.dim() != 3 \
                or cond.shape[1] != _lib.CIN or cond.numel() == 0:
            raise RuntimeError("ertdiff: inverse_cond takes a non-empty float32 (n, 14, L) tensor")
        t = cond.detach()
        if not t.is_cuda:
            t = t.to(self._dev_of(t))
        dev = _lib.require_device(t)
        t = t.contiguous()
        n, C, L = t.shape
        self._features(C * L)
        v = self._vectors(dev)
        if v.shape[1] != C * L:
            raise RuntimeError(f"ertdiff: cond has {C * L} features, the scaler has {v.shape[1]}")
        out = torch.empty(n, L, C, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ertd_minmax_cond_inverse(t.data_ptr(), n, L, C, v[0].data_ptr(),
                                                           v[1].data_ptr(), out.data_ptr(),
                                                           _lib.stream_of(dev)), "minmax_cond_inverse")
        return out

    # ---- sklearn interchange ---------------------------------------------------------
    @classmethod
    def from_sklearn(cls, scaler, device=None) -> "DeviceMinMaxScaler":
        """A fitted sklearn MinMaxScaler (or any object with its fitted
        attributes) as a DeviceMinMaxScaler; the vectors go to the device on
        first use."""
        if getattr(scaler, "clip", False):
            raise RuntimeError("ertdiff: clip=True is not supported")
        self = cls(tuple(scaler.feature_range), device=device)
        self._host = {k: np.array(getattr(scaler, k), dtype=np.float64).reshape(-1) for k in _FITTED}
        self.n_features_in_ = int(self._host["scale_"].shape[0])
        self.n_samples_seen_ = int(scaler.n_samples_seen_)
        return self

    def to_sklearn(self):
        """A fitted sklearn MinMaxScaler carrying this scaler's vectors."""
        from sklearn.preprocessing import MinMaxScaler
        sk = MinMaxScaler(feature_range=self.feature_range)
        for k, v in self._fitted_host().items():
            setattr(sk, k, v.copy())
        sk.n_features_in_ = self.n_features_in_
        sk.n_samples_seen_ = self.n_samples_seen_
        return sk


def _raw_array(x, what: str) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise RuntimeError(f"ertdiff: {what} must be a host array (prepare_dataset does the transfer)")
        x = x.detach().numpy()
    if not isinstance(x, np.ndarray):
        raise RuntimeError(f"ertdiff: {what} must be a numpy array or a host tensor, got {type(x).__name__}")
    if x.dtype != np.float64:
        raise RuntimeError(f"ertdiff: {what} must be float64, got {x.dtype}" + _f32_note(x.dtype == np.float32))
    return x


def prepare_dataset(sim_param, ert_sim, device, a: float = 0.0, b: float = 1.0,
                    chunk_rows: Optional[int] = None):
    """The reference's lines :230-269 in one call: returns
    (DeviceDataset, param_scaler, ert_scaler).

    sim_param (N, P, 1) or (N, P) and ert_sim (N, L, 14) are the raw float64
    host arrays.  param_scaler is fitted with feature_range (a, b), ert_scaler
    with (0, 1), both on the device; cond (N, 14, L) float32 is written by one
    kernel from the raw array and never exists in float64 or untransposed.

    chunk_rows=None copies ert_sim to the device once (2.67 GB at the
    reference's size).  chunk_rows=k streams it twice in k-row pieces through
    one pinned staging buffer -- partial_fit over the pieces, then
    transform_cond of each piece into cond[r0:r1] -- so the device never holds
    the raw array; the result has the same bits (a column that is NaN
    throughout one piece but not throughout the array is the exception:
    partial_fit, like sklearn's, then yields NaN).

    x0 makes a host round trip on purpose: the parameters are fitted and
    transformed on the device in float64, the (N, P) result (1.2 MB) is read
    back and goes through the host transform_to_unconstrained(
    torch.from_numpy(...).float(), a, b) exactly as DiffusionDataset does,
    then to the device.  That keeps x0 bitwise equal to DiffusionDataset.params
    -- DeviceDataset's contract -- which a device logarithm would not
    guarantee."""
    par = _raw_array(sim_param, "sim_param")
    ert = _raw_array(ert_sim, "ert_sim")
    if ert.ndim != 3 or ert.shape[2] != _lib.CIN or ert.size == 0:
        raise RuntimeError(f"ertdiff: ert_sim must be (N, L, {_lib.CIN}), got {ert.shape}")
    if not (par.ndim == 2 or (par.ndim == 3 and par.shape[2] == 1)) or par.size == 0:
        raise RuntimeError(f"ertdiff: sim_param must be (N, P, 1) or (N, P), got {par.shape}")
    if par.shape[0] != ert.shape[0]:
        raise RuntimeError(f"ertdiff: sim_param has {par.shape[0]} rows, ert_sim has {ert.shape[0]}")
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise RuntimeError(f"ertdiff: chunk_rows must be positive, got {chunk_rows}")
    dev = torch.device(device)
    N, L, C = ert.shape

    param_scaler = DeviceMinMaxScaler((a, b), device=dev)
    scaled = param_scaler.fit_transform(np.ascontiguousarray(par.reshape(N, -1)))
    raw = scaled.cpu().numpy()
    x0 = transform_to_unconstrained(torch.from_numpy(raw).float(), a, b).to(dev)

    ert_scaler = DeviceMinMaxScaler((0, 1), device=dev)
    ert2d = torch.from_numpy(np.ascontiguousarray(ert).reshape(N, L * C))
    cond = torch.empty(N, C, L, dtype=torch.float32, device=dev)
    if chunk_rows is None:
        d = ert2d.to(dev)
        ert_scaler.fit(d)
        ert_scaler.transform_cond(d, L, out=cond)
        del d
    else:
        k = min(int(chunk_rows), N)
        stage = torch.empty(k, L * C, dtype=torch.float64).pin_memory()
        dbuf = torch.empty(k, L * C, dtype=torch.float64, device=dev)
        for second in (False, True):
            for r0 in range(0, N, k):
                r1 = min(r0 + k, N)
                stage[:r1 - r0].copy_(ert2d[r0:r1])
                dbuf[:r1 - r0].copy_(stage[:r1 - r0], non_blocking=True)
                if second:
                    ert_scaler.transform_cond(dbuf[:r1 - r0], L, out=cond[r0:r1])
                else:
                    ert_scaler.partial_fit(dbuf[:r1 - r0])
                torch.cuda.synchronize(dev)   # the one staging buffer is reused next
    return DeviceDataset(x0, cond), param_scaler, ert_scaler


def split_indices(n: int, generator: Optional[torch.Generator] = None, fractions=(0.8, 0.1)):
    """The row indices of the reference's random_split(dataset, [int(.8 N),
    int(.1 N), rest]) (:271-274) as three int64 tensors: one
    torch.randperm(n, generator=generator) cut into consecutive pieces, which
    is what torch.utils.data.random_split draws.  Host code; the pieces feed
    fit(train_idx, val_idx)."""
    n = int(n)
    if n < 1:
        raise RuntimeError(f"ertdiff: split_indices needs n >= 1, got {n}")
    n_train, n_val = int(fractions[0] * n), int(fractions[1] * n)
    if n_train < 0 or n_val < 0 or n_train + n_val > n:
        raise RuntimeError(f"ertdiff: fractions {fractions} do not fit {n} rows")
    perm = torch.randperm(n, generator=generator)
    return perm[:n_train], perm[n_train:n_train + n_val], perm[n_train + n_val:]
