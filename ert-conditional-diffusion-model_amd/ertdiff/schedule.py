"""Diffusion schedule and per-step scalar tables.

These are host-side setup values (a few hundred floats, computed once per
sampler call) formed with exactly the reference's expressions so the device
receives bit-identical inputs:

  get_diffusion_schedule   ERT_Conditional_Diffusion.py:90-94 (float32 linspace /
                           cumprod, evaluated with CPU semantics -- the
                           reference's documented devices are CPU/MPS, :282)
  step_tables              the scalars sample_model forms per step (:111-118):
                           c2 = (1-a_t)/(sqrt(1-ab_t)+1e-8) is a float32 tensor,
                           c1 = 1/sqrt(a_t) and sigma = sqrt(b_t)*temperature are
                           Python doubles that torch rounds to float32 when it
                           multiplies them into a float32 tensor
  timestep_frequencies     exp(arange(half) * -ln(1e4)/(half-1)) in float32 (:81-83)
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Tuple

import torch


def get_diffusion_schedule(T: int, beta_start: float = 1e-4, beta_end: float = 0.02,
                           device="cpu") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Linear beta schedule (ERT_Conditional_Diffusion.py:90-94)."""
    betas = torch.linspace(beta_start, beta_end, T)
    alphas = 1 - betas
    alpha_bar = torch.cumprod(alphas, dim=0)
    return betas.to(device), alphas.to(device), alpha_bar.to(device)


def step_tables(betas: torch.Tensor, alphas: torch.Tensor, alpha_bar: torch.Tensor,
                num_steps: int, temperature: float = 1.0) -> torch.Tensor:
    """(3, num_steps) float32 CPU tensor: rows c1, c2, sigma, indexed by t."""
    b = betas.detach().to("cpu", torch.float32)
    a = alphas.detach().to("cpu", torch.float32)
    ab = alpha_bar.detach().to("cpu", torch.float32)
    if num_steps > a.shape[0]:
        raise RuntimeError(f"num_steps={num_steps} exceeds the schedule length {a.shape[0]}")
    out = torch.empty(3, num_steps, dtype=torch.float32)
    for t in range(num_steps):
        a_t, ab_t = a[t], ab[t]
        out[1, t] = (1 - a_t) / (math.sqrt(1 - ab_t) + 1e-8)
        out[0, t] = 1.0 / math.sqrt(a_t)
        out[2, t] = math.sqrt(b[t]) * temperature
    return out


def _check_timesteps(timesteps, T: int) -> list:
    ts = [int(t) for t in (timesteps.tolist() if hasattr(timesteps, "tolist") else timesteps)]
    if not ts:
        raise ValueError("timesteps must not be empty")
    if any(t < 0 or t >= T for t in ts):
        raise ValueError(f"timesteps must lie in [0, T={T})")
    if any(b >= a for a, b in zip(ts, ts[1:])):
        raise ValueError("timesteps must be strictly descending")
    return ts


def spaced_timesteps(T: int, steps: int) -> list:
    """round(linspace(T-1, 0, steps)), descending, duplicates removed."""
    T, steps = int(T), int(steps)
    if T < 1 or steps < 1:
        raise ValueError("spaced_timesteps needs T >= 1 and steps >= 1")
    if steps == 1:
        return [T - 1]
    out = []
    for i in range(steps):
        t = int(round((T - 1) * (1.0 - i / (steps - 1))))
        if not out or t < out[-1]:
            out.append(t)
    return out


SOLVERS = ("ddim", "dpmpp_2m")


def solver_tables(alpha_bar: torch.Tensor, timesteps, solver: str = "ddim", eta: float = 0.0,
                  temperature: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-step tables of a few-step sampler on the timestep subset
    ``timesteps`` (strictly descending, inside [0, T)).

    Returns (timesteps int32 (K), coef float32 (K, 6)); row k = p, q, a, b, c, s
    of the device update (csrc/head_dev.h solver_update)

        D = p x + q eps;   x <- a x + b D + c D_prev + s z

    With A = alpha_bar[tau_k], A' = alpha_bar[tau_{k+1}] (A' = 1 on the last
    step, which denoises to x_0), alpha = sqrt(A), sigma = sqrt(1 - A):
    p = 1/alpha, q = -sigma/alpha for every solver, and

      "ddim"      s0 = eta sqrt((1-A')/(1-A)) sqrt(1 - A/A') (0 on the last
                  step), d = sqrt(max(1 - A' - s0^2, 0)), a = d/sigma,
                  b = alpha' - d alpha/sigma, c = 0, s = temperature s0
                  (Song et al., DDIM)
      "dpmpp_2m"  a = sigma'/sigma, B0 = alpha' - sigma' alpha/sigma, s = 0;
                  first and last step b = B0, c = 0; otherwise with
                  lambda = ln(alpha/sigma), h = lambda' - lambda,
                  r = (lambda - lambda_prev)/h:
                  b = B0 (1 + 1/(2r)), c = -B0/(2r)
                  (Lu et al., DPM-Solver++ 2M, data prediction)

    Computed in Python float64 from the float32 alpha_bar, rounded to float32
    once at the end."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {list(SOLVERS)}")
    eta = float(eta)
    if solver == "dpmpp_2m" and eta != 0.0:
        raise ValueError("dpmpp_2m is deterministic: eta must be 0")
    if eta < 0.0:
        raise ValueError("eta must be >= 0")
    ab = [float(v) for v in alpha_bar.detach().to("cpu", torch.float32).tolist()]
    ts = _check_timesteps(timesteps, len(ab))
    K = len(ts)

    def lam(A):
        return 0.5 * math.log(A / (1.0 - A))

    rows = []
    for k, t in enumerate(ts):
        last = k == K - 1
        A = ab[t]
        An = 1.0 if last else ab[ts[k + 1]]
        al, sg = math.sqrt(A), math.sqrt(1.0 - A)
        aln, sgn = math.sqrt(An), math.sqrt(1.0 - An)
        p, q = 1.0 / al, -sg / al
        if solver == "ddim":
            s0 = 0.0 if last else eta * math.sqrt((1.0 - An) / (1.0 - A)) * math.sqrt(1.0 - A / An)
            d = math.sqrt(max(1.0 - An - s0 * s0, 0.0))
            a, b, c, s = d / sg, aln - d * al / sg, 0.0, float(temperature) * s0
        else:
            a, B0, c, s = sgn / sg, aln - sgn * al / sg, 0.0, 0.0
            b = B0
            if 0 < k < K - 1:
                h = lam(An) - lam(A)
                r = (lam(A) - lam(ab[ts[k - 1]])) / h
                b = B0 * (1.0 + 1.0 / (2.0 * r))
                c = -B0 / (2.0 * r)
        rows.append([p, q, a, b, c, s])
    coef = torch.tensor(rows, dtype=torch.float64).to(torch.float32)
    return torch.tensor(ts, dtype=torch.int32), coef


@lru_cache(maxsize=16)
def _freq_cpu(dim: int) -> torch.Tensor:
    half = dim // 2
    scale = math.log(10000.0) / (half - 1)
    return torch.exp(torch.arange(half, dtype=torch.float32) * -scale)


_freq_dev = {}


def timestep_frequencies(dim: int, device: torch.device) -> torch.Tensor:
    key = (dim, str(device))
    f = _freq_dev.get(key)
    if f is None:
        f = _freq_cpu(dim).to(device)
        _freq_dev[key] = f
    return f
