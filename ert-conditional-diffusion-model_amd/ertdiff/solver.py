"""Few-step samplers on a timestep subset: DDIM and DPM-Solver++(2M).

``sample_model`` walks t = n-1, n-2, ..., 0.  ``sample_fast`` visits K chosen
timesteps tau_0 > ... > tau_{K-1} instead: step k evaluates the network at
tau_k and applies

    D = p_k x + q_k eps;   D = clamp(D, -clip, clip)   (clip_denoised only)
    x <- a_k x + b_k D + c_k D_prev + s_k z;   D_prev <- D

with the six scalars of every step formed on the host (schedule.solver_tables).
The update is one device function (csrc/head_dev.h solver_update) for both
networks: the reference model runs all K steps in one persistent kernel
(ertd_sample_solver), the U-Net replays one step graph K times
(ertd_unet_sample_solver, UNetSolverPlan).

Noise: "philox" draws x_T as philox_normal(B, P, tau_0 + 1, 1, seed,
member_offset) -- the x_T sample_model(num_steps=tau_0 + 1) draws for the same
members -- and z_k from the ancestral sampler's stream at t = tau_k; a tensor
(K, B, P) injects x_T = noise[0] and z_k = noise[k + 1] (the last step draws
none).  Member ids are member_offset + b, so a member_range shard equals the
same members of the whole ensemble bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Union

import torch

from . import _lib
from .model import _PREC
from .schedule import solver_tables, spaced_timesteps, timestep_frequencies


class _Tables:
    """Device tables of one solver call."""

    def __init__(self, T, alpha_bar, steps, timesteps, solver, eta, temperature, dev):
        if alpha_bar.shape[0] != T:
            raise RuntimeError(f"ertdiff: alpha_bar has {alpha_bar.shape[0]} entries, T={T}")
        ts = spaced_timesteps(T, steps) if timesteps is None else timesteps
        t_cpu, coef_cpu = solver_tables(alpha_bar, ts, solver, eta, temperature)
        self.t_cpu = t_cpu
        self.K = int(t_cpu.numel())
        self.tau0 = int(t_cpu[0])
        self.timesteps = t_cpu.to(dev)
        self.coef = coef_cpu.to(dev)
        self.needs_d_prev = bool((coef_cpu[:, 4] != 0).any())


def _condition(condition):
    cond = _lib.f32c(condition, "condition")
    if cond.dim() == 2:
        cond = cond.unsqueeze(0)
    if cond.dim() != 3 or cond.shape[1] != _lib.CIN:
        raise RuntimeError(f"ertdiff: condition must be (B, 14, L), got {tuple(condition.shape)}")
    return cond


def _clip(clip_denoised) -> float:
    c = 0.0 if clip_denoised is None else float(clip_denoised)
    if not c >= 0.0:
        raise ValueError("clip_denoised must be None or a positive bound")
    return c


def _initial(tab, noise, B, P, seed, member_offset, dev):
    """(x_T, injected buffer or None, B)."""
    if isinstance(noise, torch.Tensor):
        inj = _lib.f32c(noise, "noise")
        if inj.dim() != 3 or inj.shape[0] != tab.K or inj.shape[2] != P:
            raise RuntimeError(f"ertdiff: noise must be (K={tab.K}, B, {P}), got {tuple(noise.shape)}")
        _lib.require_device(inj)
        return inj[0].clone(), inj, inj.shape[1]
    if noise != "philox":
        raise ValueError("noise must be 'philox' or a (K, B, P) tensor")
    if B is None:
        raise RuntimeError("ertdiff: shared_condition needs n_members (or a noise tensor)")
    from .sampler import philox_normal
    return philox_normal(B, P, tab.tau0 + 1, 1, seed, member_offset, dev), None, B


def reference_solver_segment(model, cond, stride, tab, x, d_prev, k_first, n_run, *, clip=0.0,
                             noise=None, seed=0, member_offset=0, precision=None,
                             mode="hoisted"):
    """Steps k_first .. k_first+n_run-1 of a reference-model chain on x (and
    d_prev) in place: one ertd_sample_solver call."""
    from .sampler import _MODES
    dev = x.device
    B, L = x.shape[0], cond.shape[2]
    model._check_supported()
    ws = model.workspace(dev, B, L, tab.K, _lib.OP_SAMPLE)
    w = model.weights_struct()
    freq = timestep_frequencies(_lib.HIDDEN, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ertd_sample_solver(
            ctypes.byref(w), model.packed_weights(dev).data_ptr(), cond.data_ptr(), stride, B, L,
            tab.K, k_first, n_run, tab.timesteps.data_ptr(), tab.coef.data_ptr(), clip,
            freq.data_ptr(), _lib.ptr(noise), int(seed) & (2**64 - 1),
            int(member_offset) & 0xFFFFFFFF, _MODES[mode], _PREC[precision or model.precision],
            x.data_ptr(), _lib.ptr(d_prev), ws.data_ptr(), ws.numel(), _lib.stream_of(dev)),
            "sample_solver")
    return x


def _unet_args(model, cond, stride, tab, B, x, d_prev, k_first, n_run, clip, noise, seed,
               member_offset, ws, packed):
    return (ctypes.byref(model.cfg), packed.data_ptr(), cond.data_ptr(), stride, cond.shape[2], B,
            tab.K, k_first, n_run, tab.timesteps.data_ptr(), tab.coef.data_ptr(), clip,
            _lib.ptr(noise), int(seed) & (2**64 - 1), int(member_offset) & 0xFFFFFFFF,
            x.data_ptr(), d_prev.data_ptr(), ws.data_ptr(), ws.numel())


def solver_update(x: torch.Tensor, eps: torch.Tensor, d_prev: Optional[torch.Tensor],
                  coef_row: torch.Tensor, clip: float = 0.0,
                  z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bare update of one step on (B, P) device tensors, in place on x
    (and d_prev): ertd_solver_update.  coef_row = (6,) p, q, a, b, c, s."""
    dev = _lib.require_device(x, eps, coef_row)
    if x.dim() != 2 or eps.shape != x.shape or coef_row.numel() != 6:
        raise RuntimeError("ertdiff: solver_update takes x, eps (B, P) and a (6,) coefficient row")
    for name, t in (("x", x), ("eps", eps), ("d_prev", d_prev), ("coef_row", coef_row), ("z", z)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"ertdiff: {name} must be contiguous float32")
        if t is not None and name in ("d_prev", "z") and t.shape != x.shape:
            raise RuntimeError(f"ertdiff: {name} must have the shape of x")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ertd_solver_update(
            x.data_ptr(), eps.data_ptr(), _lib.ptr(d_prev), coef_row.data_ptr(), float(clip),
            _lib.ptr(z), x.shape[0], x.shape[1], _lib.stream_of(dev)), "solver_update")
    return x


@torch.no_grad()
def sample_fast(model, condition, T, alpha_bar, param_dim, *, steps: int = 50,
                timesteps: Optional[Sequence[int]] = None, solver: str = "ddim", eta: float = 0.0,
                temperature: float = 1.0, clip_denoised: Optional[float] = None,
                noise: Union[str, torch.Tensor] = "philox", seed: int = 0, member_offset: int = 0,
                shared_condition: bool = False, n_members: Optional[int] = None,
                mode: str = "hoisted") -> torch.Tensor:
    """x_0 (B, param_dim) after K solver steps on ``timesteps`` (default:
    spaced_timesteps(T, steps)).  solver "ddim" (eta, temperature) or
    "dpmpp_2m"; clip_denoised clamps the x_0 prediction of every step to
    [-c, c].  ``model`` is a ConditionalDiffusionModel (any module with the
    reference's state_dict) or a ConditionalUNet.  mode: "hoisted" only -- the
    faithful modes of sample_model would produce the same bits and are
    refused."""
    from .sampler import _MODES, as_ertdiff_model
    from .unet import ConditionalUNet
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {list(_MODES)}")
    dev = _lib.require_device(condition)
    tab = _Tables(T, alpha_bar, steps, timesteps, solver, eta, temperature, dev)
    clip = _clip(clip_denoised)
    cond = _condition(condition)
    stride = 0 if shared_condition else _lib.CIN * cond.shape[2]
    is_unet = isinstance(model, ConditionalUNet)
    if not is_unet:
        model = as_ertdiff_model(model, dev)
    if model.param_dim != param_dim:
        raise RuntimeError(f"ertdiff: param_dim={param_dim} but the model predicts {model.param_dim}")
    B = n_members if shared_condition else cond.shape[0]
    x, inj, B = _initial(tab, noise, B, param_dim, seed, member_offset, dev)
    if not shared_condition and cond.shape[0] != B:
        raise RuntimeError(f"ertdiff: condition batch {cond.shape[0]} != noise batch {B}")
    if is_unet:
        if mode != "hoisted":
            raise RuntimeError(f"ertdiff: mode={mode!r} applies to ConditionalDiffusionModel only")
        _lib.require_device(model.conv_in.weight, x)
        d_prev = torch.empty_like(x)
        ws = model.workspace(dev, B, cond.shape[2])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ertd_unet_sample_solver(
                *_unet_args(model, cond, stride, tab, B, x, d_prev, 0, tab.K, clip, inj, seed,
                            member_offset, ws, model.packed_weights(dev)), _lib.stream_of(dev)),
                "unet_sample_solver")
        return x
    _lib.require_device(model.mlp[0].weight, x)
    d_prev = torch.empty_like(x) if tab.needs_d_prev else None
    return reference_solver_segment(model, cond, stride, tab, x, d_prev, 0, tab.K, clip=clip,
                                    noise=inj, seed=seed, member_offset=member_offset, mode=mode)


class UNetSolverPlan:
    """hipGraph plan of one U-Net solver chain (head graph + one step graph
    replayed K times).  ``x`` holds the state: set it to x_T before launch
    (``x_T()`` returns the Philox draw sample_fast starts from)."""

    def __init__(self, model, condition, T, alpha_bar, *, steps: int = 50,
                 timesteps: Optional[Sequence[int]] = None, solver: str = "ddim",
                 eta: float = 0.0, temperature: float = 1.0,
                 clip_denoised: Optional[float] = None, B: Optional[int] = None, seed: int = 0,
                 member_offset: int = 0, shared_condition: bool = False,
                 noise: Optional[torch.Tensor] = None):
        dev = _lib.require_device(condition, model.conv_in.weight)
        self.dev = dev
        self.model = model
        self.tab = _Tables(T, alpha_bar, steps, timesteps, solver, eta, temperature, dev)
        self.cond = _condition(condition)
        L = self.cond.shape[2]
        stride = 0 if shared_condition else _lib.CIN * L
        self.B = B if B is not None else self.cond.shape[0]
        self.seed, self.member_offset = seed, member_offset
        self.noise = None if noise is None else _lib.f32c(noise, "noise")
        if self.noise is not None and tuple(self.noise.shape) != (self.tab.K, self.B, model.param_dim):
            raise RuntimeError(f"ertdiff: noise must be (K={self.tab.K}, {self.B}, {model.param_dim})")
        self.x = torch.zeros(self.B, model.param_dim, dtype=torch.float32, device=dev)
        self.d_prev = torch.zeros_like(self.x)
        self.packed = model.packed_weights(dev)
        # a workspace of its own, as UNetSamplerPlan
        nbytes = _lib.lib().ertd_unet_workspace_bytes(ctypes.byref(model.cfg), self.B, L)
        if nbytes == 0:
            raise RuntimeError("ertdiff: unsupported U-Net configuration")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._plan = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ertd_unet_sample_solver_plan_create(
                *_unet_args(model, self.cond, stride, self.tab, self.B, self.x, self.d_prev, 0,
                            self.tab.K, _clip(clip_denoised), self.noise, seed, member_offset,
                            self.ws, self.packed), _lib.stream_of(dev), ctypes.byref(self._plan)),
                "unet_sample_solver_plan_create")

    @property
    def K(self) -> int:
        return self.tab.K

    def x_T(self) -> torch.Tensor:
        if self.noise is not None:
            return self.noise[0].clone()
        from .sampler import philox_normal
        return philox_normal(self.B, self.model.param_dim, self.tab.tau0 + 1, 1, self.seed,
                             self.member_offset, self.dev)

    def launch(self, stream: Optional[torch.cuda.Stream] = None, n_steps: Optional[int] = None):
        """Replays the head graph and the K steps (or only the first n_steps)."""
        s = (stream or torch.cuda.current_stream(self.dev)).cuda_stream
        with torch.cuda.device(self.dev):
            if n_steps is None:
                _lib.check(_lib.lib().ertd_unet_plan_launch(self._plan, s), "unet_plan_launch")
            else:
                _lib.check(_lib.lib().ertd_unet_plan_launch_steps(self._plan, int(n_steps), s),
                           "unet_plan_launch_steps")

    def close(self):
        if self._plan:
            _lib.lib().ertd_unet_plan_destroy(self._plan)
            self._plan = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
