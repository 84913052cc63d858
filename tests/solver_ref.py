"""Float64 restatement of the two few-step solvers in their textbook step
form (eps -> x0 -> next x), independent of the table form the product uses
(ertdiff.schedule.solver_tables): test infrastructure only.

  ddim      Song et al., "Denoising Diffusion Implicit Models", eq. 12 / 16:
            x' = alpha' x0 + sqrt(1 - A' - sigma^2) eps + sigma z
  dpmpp_2m  Lu et al., "DPM-Solver++", Algorithm 2 (2M, data prediction):
            x' = (sigma'/sigma) x - alpha' expm1(-h) D,
            D = (1 + 1/(2r)) x0 - 1/(2r) x0_prev,  r = h_prev / h

Both end by denoising to x0 (A' = 1 after the last timestep).  ``model`` is
any callable model(x, t) -> eps on float64 numpy arrays (t a Python int).
With ``clip`` the x0 prediction is clamped and eps re-derived from it, as
the common implementations do.
"""
import math

import numpy as np


def _lam(A):
    return 0.5 * math.log(A / (1.0 - A))


def sample(model, alpha_bar, timesteps, x_T, solver="ddim", eta=0.0, temperature=1.0, noise=None,
           clip=None):
    """x_0 after len(timesteps) steps from x_T.  alpha_bar: (T,) array (its
    float32 values are used as they are, in float64).  noise: indexable, z of
    step k = noise[k + 1] (noise[0] is x_T's slot and is not read)."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    ts = [int(t) for t in timesteps]
    K = len(ts)
    x = np.asarray(x_T, dtype=np.float64).copy()
    x0_prev = None
    for k, t in enumerate(ts):
        last = k == K - 1
        A = float(ab[t])
        alpha, sigma = math.sqrt(A), math.sqrt(1.0 - A)
        eps = np.asarray(model(x, t), dtype=np.float64)
        x0 = (x - sigma * eps) / alpha
        if clip:
            x0 = np.clip(x0, -clip, clip)
            eps = (x - alpha * x0) / sigma
        if last:
            x = x0
            break
        An = float(ab[ts[k + 1]])
        alpha_n, sigma_n = math.sqrt(An), math.sqrt(1.0 - An)
        if solver == "ddim":
            sig = eta * math.sqrt((1.0 - An) / (1.0 - A)) * math.sqrt(1.0 - A / An)
            x = alpha_n * x0 + math.sqrt(max(1.0 - An - sig * sig, 0.0)) * eps
            if sig != 0.0:
                x = x + temperature * sig * np.asarray(noise[k + 1], dtype=np.float64)
        elif solver == "dpmpp_2m":
            h = _lam(An) - _lam(A)
            D = x0
            if k > 0:
                r = (_lam(A) - _lam(float(ab[ts[k - 1]]))) / h
                D = (1.0 + 1.0 / (2.0 * r)) * x0 - (1.0 / (2.0 * r)) * x0_prev
            x = (sigma_n / sigma) * x - alpha_n * math.expm1(-h) * D
        else:
            raise ValueError(solver)
        x0_prev = x0
    return x


def table_walk(model, timesteps, coef, x_T, noise=None, clip=None):
    """The product's update driven by its own (K, 6) table, in float64:
    D = p x + q eps;  x <- a x + b D + c D_prev + s z."""
    x = np.asarray(x_T, dtype=np.float64).copy()
    d_prev = np.zeros_like(x)
    for k, t in enumerate(int(v) for v in timesteps):
        p, q, a, b, c, s = (float(v) for v in coef[k])
        D = p * x + q * np.asarray(model(x, t), dtype=np.float64)
        if clip:
            D = np.clip(D, -clip, clip)
        x = a * x + b * D + c * d_prev
        if s != 0.0:
            x = x + s * np.asarray(noise[k + 1], dtype=np.float64)
        d_prev = D
    return x


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
