"""Host-side checks of the few-step solver tables (ertdiff.schedule
spaced_timesteps / solver_tables) against the textbook step forms restated in
tests/solver_ref.py.  No GPU.

Gate of the table-vs-textbook walks: 1e-6 rel-L2.  The table is rounded to
float32 once (2^-24 = 6e-8 per coefficient), which the K-step walk carries to
3e-8 .. 2e-7; a wrong r or a dropped term moves the result by 1e-2."""
import math

import numpy as np
import pytest
import torch

import solver_ref as SR
from ertdiff.schedule import get_diffusion_schedule, solver_tables, spaced_timesteps

TOL = 1e-6
CASES = [("ddim", 0.0), ("ddim", 0.7), ("ddim", 1.0), ("dpmpp_2m", 0.0)]


def _denoiser(x, t):
    """A fixed nonlinear stand-in for the network."""
    return np.tanh(0.7 * x + 0.3 * math.sin(0.05 * t)) + 0.1 * x * math.cos(0.01 * t)


def _inputs(K, P=29, B=4, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, P)), rng.standard_normal((K, B, P))


@pytest.mark.parametrize("T", [50, 1000])
@pytest.mark.parametrize("K", [1, 2, 7, 20])
@pytest.mark.parametrize("solver,eta", CASES)
def test_tables_match_textbook(T, K, solver, eta):
    ab = get_diffusion_schedule(T)[2]
    ts = spaced_timesteps(T, K)
    tsd, coef = solver_tables(ab, ts, solver, eta, temperature=0.9)
    assert tsd.dtype == torch.int32 and coef.dtype == torch.float32
    assert tsd.tolist() == ts and tuple(coef.shape) == (len(ts), 6)
    x_T, noise = _inputs(len(ts))
    got = SR.table_walk(_denoiser, ts, coef.numpy(), x_T, noise)
    ref = SR.sample(_denoiser, ab.numpy(), ts, x_T, solver, eta, 0.9, noise)
    err = SR.rel_l2(got, ref)
    print(f"T={T} K={K} {solver} eta={eta}: rel-L2 {err:.2e}")
    assert err <= TOL, err


@pytest.mark.parametrize("solver,eta", CASES)
def test_tables_match_textbook_clipped_uneven(solver, eta):
    """Uneven timesteps (tau_k != k) and a clamp that binds."""
    T, ts = 50, [49, 40, 33, 20, 9, 3, 0]
    ab = get_diffusion_schedule(T)[2]
    _, coef = solver_tables(ab, ts, solver, eta)
    x_T, noise = _inputs(len(ts))
    got = SR.table_walk(_denoiser, ts, coef.numpy(), x_T, noise, clip=0.5)
    ref = SR.sample(_denoiser, ab.numpy(), ts, x_T, solver, eta, 1.0, noise, clip=0.5)
    assert np.abs(ref).max() <= 0.5 + 1e-12          # the last clamp is the result's bound
    assert SR.rel_l2(got, ref) <= TOL


@pytest.mark.parametrize("T,K", [(50, 7), (1000, 20), (1000, 1)])
def test_table_structure(T, K):
    ab = get_diffusion_schedule(T)[2]
    ts = spaced_timesteps(T, K)
    ddim0 = solver_tables(ab, ts, "ddim", 0.0)[1]
    ddim7 = solver_tables(ab, ts, "ddim", 0.7)[1]
    dpm = solver_tables(ab, ts, "dpmpp_2m")[1]
    for c in (ddim0, ddim7, dpm):
        assert c[-1, 2:].tolist() == [0.0, 1.0, 0.0, 0.0]     # a, b, c, s of the last row
        assert c[0, 4].item() == 0.0                          # c_0
        A = ab[ts].double()
        assert torch.equal(c[:, 0], (1.0 / A.sqrt()).float())
        assert torch.equal(c[:, 1], (-(1.0 - A).sqrt() / A.sqrt()).float())
    assert torch.equal(dpm[0], ddim0[0])
    assert torch.count_nonzero(ddim0[:, 5]) == 0 and torch.count_nonzero(ddim0[:, 4]) == 0
    assert torch.count_nonzero(dpm[:, 5]) == 0
    if K > 2:
        assert torch.all(ddim7[:-1, 5] > 0) and torch.all(dpm[1:-1, 4] != 0)
    # temperature scales the s column only
    hot = solver_tables(ab, ts, "ddim", 0.7, temperature=2.0)[1]
    assert torch.equal(hot[:, :5], ddim7[:, :5])
    assert torch.allclose(hot[:, 5], 2.0 * ddim7[:, 5], rtol=1e-6, atol=0)


@pytest.mark.parametrize("solver,eta", CASES)
@pytest.mark.parametrize("T,K", [(50, 7), (1000, 20), (1000, 2)])
def test_point_mass_denoiser_returns_the_mass(solver, eta, T, K):
    """For data concentrated on one point m the exact denoiser is
    eps = (x - alpha m) / sigma; every solver then lands on m."""
    abt = get_diffusion_schedule(T)[2]
    ab = abt.double().numpy()
    ts = spaced_timesteps(T, K)
    _, coef = solver_tables(abt, ts, solver, eta)
    x_T, noise = _inputs(len(ts))
    m = np.random.default_rng(9).standard_normal(x_T.shape)

    def model(x, t):
        return (x - math.sqrt(ab[t]) * m) / math.sqrt(1.0 - ab[t])

    got = SR.table_walk(model, ts, coef.numpy(), x_T, noise)
    err = SR.rel_l2(got, m)
    print(f"point mass T={T} K={K} {solver} eta={eta}: rel-L2 {err:.2e}")
    assert err <= TOL, err
    assert SR.rel_l2(SR.sample(model, ab, ts, x_T, solver, eta, 1.0, noise), m) <= 1e-12


def test_spaced_timesteps():
    for T in (1, 2, 50, 1000):
        assert spaced_timesteps(T, T) == list(range(T - 1, -1, -1))
    assert spaced_timesteps(1000, 1) == [999]
    assert spaced_timesteps(1000, 2) == [999, 0]
    ts = spaced_timesteps(1000, 50)
    assert len(ts) == 50 and ts[0] == 999 and ts[-1] == 0
    assert ts == [int(v) for v in np.round(np.linspace(999, 0, 50))]
    # more steps than timesteps: duplicates are removed, the order stays strict
    ts = spaced_timesteps(10, 25)
    assert ts == list(range(9, -1, -1))
    ts = spaced_timesteps(50, 37)
    assert all(b < a for a, b in zip(ts, ts[1:])) and len(ts) < 50 and ts[0] == 49 and ts[-1] == 0


@pytest.mark.parametrize("bad", [[0, 3, 9], [9, 9, 3], [9, 3, 3], [9, 3, -1], [50, 9, 0], []])
def test_bad_timesteps_rejected(bad):
    ab = get_diffusion_schedule(50)[2]
    with pytest.raises(ValueError):
        solver_tables(ab, bad)


def test_bad_solver_arguments_rejected():
    ab = get_diffusion_schedule(50)[2]
    with pytest.raises(ValueError):
        solver_tables(ab, [9, 3, 0], solver="euler")
    with pytest.raises(ValueError):
        solver_tables(ab, [9, 3, 0], solver="dpmpp_2m", eta=0.5)
    with pytest.raises(ValueError):
        spaced_timesteps(50, 0)
    # a tensor of timesteps is accepted like a list
    assert solver_tables(ab, torch.tensor([9, 3, 0]))[0].tolist() == [9, 3, 0]
