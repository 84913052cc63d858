"""The few-step samplers (DDIM, DPM-Solver++(2M)) on the GPU: the bare update
against float64, whole chains of both networks against the textbook step
forms (tests/solver_ref.py) around the float64 oracle models, and the bitwise
properties of the segment / member / plan contracts.

Gates: the update's elementwise bound is worked out below; chains <= 1e-4
rel-L2, the project's full-chain gate (measured values go to record_error)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ertdiff
import solver_ref as SR
from conftest import record_error
from ertdiff import _lib
from ertdiff import solver as S
from oracle import ref_torch as RT
from oracle import unet_torch as U
from synth import synth_normal, synth_uniform

pytestmark = pytest.mark.gpu

CHAIN_TOL = 1e-4
T = 50
TS = [49, 40, 33, 20, 9, 3, 0]       # uneven, tau_k != k everywhere but the end
B, L, P = 5, 37, 29                  # B = 5: the last workgroup of four waves is partly empty


def _ab():
    return ertdiff.get_diffusion_schedule(T)[2]


@pytest.fixture(scope="module")
def cond():
    return torch.from_numpy(synth_uniform((B, 14, L), 702))


@pytest.fixture(scope="module")
def model64(golden_weights, cond):
    """oracle/ref_torch's model in float64 (the sinusoid stays float32, as the
    reference defines it), the condition encoder evaluated once."""
    W = {k: torch.from_numpy(v).double() for k, v in golden_weights.items()}
    cemb = RT.encoder(cond.double(), W)

    def model(x, t):
        xt = torch.from_numpy(np.asarray(x))
        tt = torch.full((xt.shape[0],), int(t), dtype=torch.long)
        te = F.relu(F.linear(RT.timestep_embedding(tt, 128).double(), W["time_embed.0.weight"],
                             W["time_embed.0.bias"]))
        h = F.relu(F.linear(torch.cat([xt, te, cemb], dim=1), W["mlp.0.weight"], W["mlp.0.bias"]))
        return F.linear(h, W["mlp.2.weight"], W["mlp.2.bias"]).numpy()

    return model


def _noise(K, seed=703, b=B, p=P):
    return torch.from_numpy(synth_normal((K, b, p), seed))


# ---- ertd_solver_update alone ------------------------------------------------------------
def _f64_update(x, eps, dp, z, row, clip):
    p, q, a, b, c, s = (float(v) for v in row)
    x, eps, dp, z = (v.double() for v in (x, eps, dp, z))
    D = p * x + q * eps
    if clip:
        D = D.clamp(-clip, clip)
    new = a * x + b * D + c * dp + s * z
    # five or six fp32 roundings, each at most 2^-24 of a magnitude that bounds its result
    bound = 8 * 2.0 ** -24 * ((a * x).abs() + abs(b) * ((p * x).abs() + (q * eps).abs()) +
                              (c * dp).abs() + (s * z).abs())
    d_bound = 4 * 2.0 ** -24 * ((p * x).abs() + (q * eps).abs())
    return new, D, bound, d_bound


@pytest.mark.parametrize("clip", [0.0, 0.8])
@pytest.mark.parametrize("case", ["full", "no_noise", "no_d_prev_term", "null_buffers"])
def test_solver_update_alone(case, clip, cuda_dev):
    Bu, Pu = 3, 37
    g = torch.Generator().manual_seed(11)
    x, eps, dp, z = (torch.randn(Bu, Pu, generator=g) for _ in range(4))
    row = torch.randn(6, generator=g) * torch.tensor([1.5, 1.5, 1.0, 1.0, 0.7, 0.5])
    z_dev, dp_dev = z.clone(), dp.clone()
    if case == "no_noise":            # s = 0: z must not be read
        row[5] = 0.0
        z_dev.fill_(float("nan"))
    if case == "no_d_prev_term":      # c = 0: D_prev must not be read (it is still written)
        row[4] = 0.0
        dp_dev.fill_(float("nan"))
    if case == "null_buffers":
        row[4] = 0.0
        row[5] = 0.0
    assert case != "full" or (row[4] != 0 and row[5] != 0)
    ref, Dref, bound, d_bound = _f64_update(x, eps, dp, z, row, clip)
    xd = x.to(cuda_dev)
    dpd = None if case == "null_buffers" else dp_dev.to(cuda_dev)
    zd = None if case == "null_buffers" else z_dev.to(cuda_dev)
    S.solver_update(xd, eps.to(cuda_dev), dpd, row.to(cuda_dev), clip, zd)
    err = (xd.cpu().double() - ref).abs()
    print(f"update {case} clip={clip}: max err/bound {(err / bound).max().item():.3f}")
    assert torch.all(err <= bound)
    if dpd is not None:
        assert torch.all((dpd.cpu().double() - Dref).abs() <= d_bound)
        if clip:
            # the device clamps at float32(clip)
            assert dpd.abs().max().item() <= float(np.float32(clip)) and (Dref.abs() == clip).any()


# ---- reference-model chains against the textbook forms -------------------------------------
CHAINS = [("ddim", 0.0, "philox", None), ("ddim", 0.7, "injected", 2.0),
          ("dpmpp_2m", 0.0, "philox", None), ("dpmpp_2m", 0.0, "injected", 1.5)]


@pytest.mark.parametrize("solver,eta,src,clip", CHAINS)
def test_reference_chain_vs_textbook(solver, eta, src, clip, gpu_model, model64, cond, cuda_dev):
    ab = _ab()
    noise = _noise(len(TS))
    if src == "philox":
        x_T = ertdiff.philox_normal(B, P, TS[0] + 1, 1, 77, 0, cuda_dev).cpu()
        arg = "philox"
    else:
        x_T, arg = noise[0], noise.to(cuda_dev)
    got = ertdiff.sample_fast(gpu_model, cond.to(cuda_dev), T, ab, P, timesteps=TS, solver=solver,
                              eta=eta, temperature=0.9, clip_denoised=clip, noise=arg, seed=77).cpu()
    ref = SR.sample(model64, ab.numpy(), TS, x_T.numpy(), solver, eta, 0.9, noise.numpy(), clip)
    err = SR.rel_l2(got.numpy(), ref)
    record_error(f"solver_chain_ref_{solver}_eta{eta}_{src}", err)
    print(f"chain {solver} eta={eta} {src} clip={clip}: rel-L2 {err:.2e}")
    assert err <= CHAIN_TOL, err
    if clip:
        assert got.abs().max().item() <= clip


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_reference_single_step_chain(solver, gpu_model, model64, cond, cuda_dev):
    """K = 1 runs the single last row: x_0 = the x0 prediction at tau_0."""
    ab = _ab()
    noise = _noise(1)
    got = ertdiff.sample_fast(gpu_model, cond.to(cuda_dev), T, ab, P, timesteps=[20], solver=solver,
                              noise=noise.to(cuda_dev)).cpu()
    ref = SR.sample(model64, ab.numpy(), [20], noise[0].numpy(), solver)
    err = SR.rel_l2(got.numpy(), ref)
    record_error(f"solver_chain_ref_{solver}_K1", err)
    assert err <= CHAIN_TOL, err


# ---- bitwise properties, reference model ------------------------------------------------------
def _segments(gpu_model, cond, dev, solver, eta, splits, seed=5, x_T=None):
    tab = S._Tables(T, _ab(), None, TS, solver, eta, 1.0, dev)
    x = (ertdiff.philox_normal(B, P, TS[0] + 1, 1, seed, 0, dev) if x_T is None else x_T.clone())
    d_prev = torch.full_like(x, float("nan"))        # never read before it is written
    cd = cond.to(dev)
    k = 0
    for n in splits:
        S.reference_solver_segment(gpu_model, cd, 14 * L, tab, x, d_prev, k, n, seed=seed)
        k += n
    assert k == tab.K
    return x.cpu()


@pytest.mark.parametrize("solver,eta", [("dpmpp_2m", 0.0), ("ddim", 0.7)])
def test_split_chain_equals_unsplit(solver, eta, gpu_model, cond, cuda_dev):
    whole = _segments(gpu_model, cond, cuda_dev, solver, eta, [7])
    assert torch.isfinite(whole).all()
    assert torch.equal(_segments(gpu_model, cond, cuda_dev, solver, eta, [3, 4]), whole)
    assert torch.equal(_segments(gpu_model, cond, cuda_dev, solver, eta, [1, 1, 5]), whole)
    # the public call is the unsplit chain
    pub = ertdiff.sample_fast(gpu_model, cond.to(cuda_dev), T, _ab(), P, timesteps=TS, solver=solver,
                              eta=eta, seed=5).cpu()
    assert torch.equal(pub, whole)


def test_member_shards_and_reruns_are_bitwise(gpu_model, cond, cuda_dev):
    cd = cond.to(cuda_dev)
    kw = dict(timesteps=TS, solver="ddim", eta=0.7, seed=21)
    whole = ertdiff.sample_fast(gpu_model, cd, T, _ab(), P, **kw).cpu()
    again = ertdiff.sample_fast(gpu_model, cd, T, _ab(), P, **kw).cpu()
    assert torch.equal(whole, again)
    lo = ertdiff.sample_fast(gpu_model, cd[:2], T, _ab(), P, member_offset=0, **kw).cpu()
    hi = ertdiff.sample_fast(gpu_model, cd[2:], T, _ab(), P, member_offset=2, **kw).cpu()
    assert torch.equal(torch.cat([lo, hi]), whole)
    other = ertdiff.sample_fast(gpu_model, cd, T, _ab(), P, **{**kw, "seed": 22}).cpu()
    assert not torch.equal(other, whole)
    # x_T is the draw sample_model(num_steps = tau_0 + 1) starts from
    one = ertdiff.sample_fast(gpu_model, cd, T, _ab(), P, timesteps=[TS[0]], seed=21).cpu()
    x_T = ertdiff.philox_normal(B, P, TS[0] + 1, 1, 21, 0, cuda_dev)
    inj = ertdiff.sample_fast(gpu_model, cd, T, _ab(), P, timesteps=[TS[0]], noise=x_T[None]).cpu()
    assert torch.equal(one, inj)


def test_deterministic_ddim_ignores_seed_after_x_T(gpu_model, cond, cuda_dev):
    """eta = 0: every s_k is zero, so no z is drawn -- the same x_T under two
    seeds of the Philox source gives the same bits."""
    x_T = torch.from_numpy(synth_normal((B, P), 704)).to(cuda_dev)
    a = _segments(gpu_model, cond, cuda_dev, "ddim", 0.0, [7], seed=1, x_T=x_T)
    b = _segments(gpu_model, cond, cuda_dev, "ddim", 0.0, [7], seed=2, x_T=x_T)
    c = _segments(gpu_model, cond, cuda_dev, "ddim", 0.7, [7], seed=1, x_T=x_T)
    d = _segments(gpu_model, cond, cuda_dev, "ddim", 0.7, [7], seed=2, x_T=x_T)
    assert torch.equal(a, b)
    assert not torch.equal(c, d) and not torch.equal(a, c)


# ---- cross-path: the bare update and the persistent kernel's step ---------------------------------
@pytest.mark.parametrize("clip", [None, 0.6])
def test_update_kernel_equals_persistent_step(clip, gpu_model, cond, cuda_dev):
    """A K = 1 chain whose eps is read back through ertd_forward: one
    ertd_solver_update call on the same x, eps and row gives the same bits."""
    cd = cond.to(cuda_dev)
    x_T = torch.from_numpy(synth_normal((B, P), 705)).to(cuda_dev)
    tab = S._Tables(T, _ab(), None, [33], "dpmpp_2m", 0.0, 1.0, cuda_dev)
    chain = ertdiff.sample_fast(gpu_model, cd, T, _ab(), P, timesteps=[33], solver="dpmpp_2m",
                                clip_denoised=clip, noise=x_T[None].contiguous())
    with torch.no_grad():
        eps = gpu_model(x_T, torch.full((B,), 33, device=cuda_dev), cd)
    x = x_T.clone()
    S.solver_update(x, eps.contiguous(), None, tab.coef[0].contiguous(), clip or 0.0, None)
    assert torch.equal(x, chain)
    # the same with a general row (a, b != 0, 1): the first step of a two-step chain
    tab2 = S._Tables(T, _ab(), None, [33, 9], "ddim", 0.0, 1.0, cuda_dev)
    assert tab2.coef[0, 2].item() != 0.0
    seg, d_seg = x_T.clone(), torch.zeros_like(x_T)
    S.reference_solver_segment(gpu_model, cd, 14 * L, tab2, seg, d_seg, 0, 1, clip=clip or 0.0)
    x, d = x_T.clone(), torch.zeros_like(x_T)
    S.solver_update(x, eps.contiguous(), d, tab2.coef[0].contiguous(), clip or 0.0, None)
    assert torch.equal(x, seg) and torch.equal(d, d_seg)


# ---- U-Net -------------------------------------------------------------------------------------------
UB, UTS = 2, [45, 30, 12, 0]
# ertd_unet_workspace_bytes(cfg, B = 2, L = 37) of the commit before the solver
# plans were added (d624bde), noted from a build of that commit (8526336,
# 68379392), less the 256 bytes of the walk's GroupNorm-fold counters (one
# allocation of B words), which went with the fold
UNET_WS_BYTES = {"U1": 8526336 - 256, "U2": 68379392 - 256}


@pytest.fixture(scope="module")
def unet_pair(cuda_dev):
    m = ertdiff.ConditionalUNet.from_config("U1", seed=0).to(cuda_dev).eval()
    W = {k: v.double() for k, v in U.init_weights(U.CONFIGS["U1"], 0).items()}
    return m, W


@pytest.fixture(scope="module")
def unet_cond():
    return torch.from_numpy(synth_uniform((UB, 14, L), 706))


@pytest.mark.parametrize("solver,eta", [("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_unet_chain_vs_textbook_and_plan(solver, eta, unet_pair, unet_cond, cuda_dev):
    m, W = unet_pair
    cfg = U.CONFIGS["U1"]
    ab = _ab()
    noise = _noise(len(UTS), 707, UB, cfg.param_dim)
    cd = unet_cond.to(cuda_dev)

    def model(x, t):
        with torch.no_grad():
            return U.forward(torch.from_numpy(np.asarray(x)), torch.full((UB,), int(t)),
                             unet_cond.double(), W, cfg).numpy()

    kw = dict(timesteps=UTS, solver=solver, eta=eta, temperature=0.9)
    got = ertdiff.sample_fast(m, cd, T, ab, cfg.param_dim, noise=noise.to(cuda_dev), **kw)
    ref = SR.sample(model, ab.numpy(), UTS, noise[0].numpy(), solver, eta, 0.9, noise.numpy())
    err = SR.rel_l2(got.cpu().numpy(), ref)
    record_error(f"solver_chain_unet_U1_{solver}_eta{eta}", err)
    print(f"U-Net chain {solver} eta={eta}: rel-L2 {err:.2e}")
    assert err <= CHAIN_TOL, err
    # the plan equals the eager call bit for bit, and replays to the same bits
    plan = ertdiff.UNetSolverPlan(m, cd, T, ab, noise=noise.to(cuda_dev), **kw)
    assert plan.K == len(UTS)
    for _ in range(2):
        plan.x.copy_(plan.x_T())
        plan.d_prev.fill_(float("nan"))
        plan.launch()
        torch.cuda.synchronize(cuda_dev)
        assert torch.equal(plan.x, got)
    plan.close()


def test_unet_philox_plan_and_member_shards(unet_pair, unet_cond, cuda_dev):
    m, _ = unet_pair
    Pu = U.CONFIGS["U1"].param_dim
    cd = unet_cond.to(cuda_dev)
    kw = dict(timesteps=UTS, solver="ddim", eta=1.0, seed=31)
    whole = ertdiff.sample_fast(m, cd, T, _ab(), Pu, **kw)
    parts = [ertdiff.sample_fast(m, cd[i:i + 1], T, _ab(), Pu, member_offset=i, **kw) for i in range(UB)]
    assert torch.equal(torch.cat(parts), whole)
    plan = ertdiff.UNetSolverPlan(m, cd, T, _ab(), **kw)
    plan.x.copy_(plan.x_T())
    plan.launch()
    torch.cuda.synchronize(cuda_dev)
    assert torch.equal(plan.x, whole)
    plan.close()


def test_unet_plan_long_enough_for_the_multi_step_graph(unet_pair, unet_cond, cuda_dev):
    """From 16 steps on a plan also replays a graph of 8 consecutive steps:
    17 steps = two of those and a single one, against the eager call."""
    m, _ = unet_pair
    Pu = U.CONFIGS["U1"].param_dim
    cd = unet_cond.to(cuda_dev)
    kw = dict(steps=17, solver="dpmpp_2m", seed=32)
    eager = ertdiff.sample_fast(m, cd, T, _ab(), Pu, **kw)
    plan = ertdiff.UNetSolverPlan(m, cd, T, _ab(), **kw)
    assert plan.K == 17
    plan.x.copy_(plan.x_T())
    plan.launch()
    torch.cuda.synchronize(cuda_dev)
    assert torch.isfinite(eager).all() and torch.equal(plan.x, eager)
    plan.close()


@pytest.mark.parametrize("name", ["U1", "U2"])
def test_unet_workspace_bytes_unchanged(name):
    m = ertdiff.ConditionalUNet.from_config(name, seed=0)
    assert _lib.lib().ertd_unet_workspace_bytes(ctypes.byref(m.cfg), 2, L) == UNET_WS_BYTES[name]


# ---- guards ---------------------------------------------------------------------------------------------
def _einval(excinfo):
    return f"({_lib.ERTD_EINVAL})" in str(excinfo.value)


def test_guards_reference_model(gpu_model, cond, cuda_dev):
    cd = cond.to(cuda_dev)
    for mode in ("faithful", "faithful_steps"):
        with pytest.raises(RuntimeError) as e:
            ertdiff.sample_fast(gpu_model, cd, T, _ab(), P, timesteps=TS, mode=mode)
        assert _einval(e)
    x = torch.zeros(B, P, device=cuda_dev)
    tab = S._Tables(T, _ab(), None, TS, "dpmpp_2m", 0.0, 1.0, cuda_dev)
    assert tab.needs_d_prev
    with pytest.raises(RuntimeError) as e:       # c != 0 needs the D_prev buffer
        S.reference_solver_segment(gpu_model, cd, 14 * L, tab, x, None, 0, tab.K)
    assert _einval(e)
    for bad in ([49, 40, 40, 20, 9, 3, 0], [0, 3, 9, 20, 33, 40, 49], [49, 40, 33, 20, 9, 3, -1]):
        tab = S._Tables(T, _ab(), None, TS, "ddim", 0.0, 1.0, cuda_dev)
        tab.timesteps.copy_(torch.tensor(bad, dtype=torch.int32))
        with pytest.raises(RuntimeError) as e:
            S.reference_solver_segment(gpu_model, cd, 14 * L, tab, x, None, 0, tab.K)
        assert _einval(e)
    tab = S._Tables(T, _ab(), None, TS, "ddim", 0.0, 1.0, cuda_dev)
    for k_first, n_run in ((0, 8), (7, 1), (-1, 2), (3, 5), (0, 0)):
        with pytest.raises(RuntimeError) as e:   # steps outside the table
            S.reference_solver_segment(gpu_model, cd, 14 * L, tab, x, None, k_first, n_run)
        assert _einval(e)
    # an injected (K, B, P) buffer has no row for a z of the last step
    tab.coef[-1, 5] = 0.5
    with pytest.raises(RuntimeError) as e:
        S.reference_solver_segment(gpu_model, cd, 14 * L, tab, x, None, 0, tab.K,
                                   noise=_noise(len(TS)).to(cuda_dev))
    assert _einval(e)
    assert torch.count_nonzero(x) == 0           # nothing was enqueued


def test_guards_unet_and_python(unet_pair, unet_cond, gpu_model, cond, cuda_dev):
    m, _ = unet_pair
    Pu = U.CONFIGS["U1"].param_dim
    cd = unet_cond.to(cuda_dev)
    with pytest.raises(RuntimeError):
        ertdiff.sample_fast(m, cd, T, _ab(), Pu, timesteps=UTS, mode="faithful")
    with pytest.raises(ValueError):
        ertdiff.sample_fast(m, cd, T, _ab(), Pu, timesteps=[0, 12])
    with pytest.raises(ValueError):
        ertdiff.sample_fast(gpu_model, cond.to(cuda_dev), T, _ab(), P, timesteps=[T, 3])
    with pytest.raises(ValueError):
        ertdiff.sample_fast(gpu_model, cond.to(cuda_dev), T, _ab(), P, solver="dpmpp_2m", eta=0.3)
    with pytest.raises(RuntimeError):            # noise rows must match K
        ertdiff.sample_fast(gpu_model, cond.to(cuda_dev), T, _ab(), P, timesteps=TS,
                            noise=_noise(3).to(cuda_dev))
    bad = S._Tables(T, _ab(), None, UTS, "dpmpp_2m", 0.0, 1.0, cuda_dev)
    bad.timesteps.copy_(torch.tensor([45, 30, 30, 0], dtype=torch.int32))
    x = torch.zeros(UB, Pu, device=cuda_dev)
    ws = m.workspace(cuda_dev, UB, L)
    args = S._unet_args(m, cd, 14 * L, bad, UB, x, torch.zeros_like(x), 0, bad.K, 0.0, None, 0, 0,
                        ws, m.packed_weights(cuda_dev))
    with torch.cuda.device(cuda_dev):
        s = _lib.stream_of(cuda_dev)
        assert _lib.lib().ertd_unet_sample_solver(*args, s) == _lib.ERTD_EINVAL
        plan = ctypes.c_void_p()
        assert _lib.lib().ertd_unet_sample_solver_plan_create(*args, s, ctypes.byref(plan)) == _lib.ERTD_EINVAL
        assert not plan.value
    assert torch.count_nonzero(x) == 0
