"""The Python API on the memory a long-running process hands it.

  clean vs dirty   every public call once normally and once under
                   dirty_state.dirty_allocator (every torch.empty /
                   torch.empty_like CUDA tensor inside ertdiff/*.py -- the
                   workspaces, the outputs, the scratch gradients -- filled
                   with 0xFF), on fresh objects with the same seeds and
                   inputs: bitwise equal, finite.
  pre-seeded cache a 0xFF tensor of twice the needed size in model._ws[...]:
                   the results of a fresh model.
  reuse            one model across (B, L, T) geometries and entry points,
                   every layout offset landing on another call's leftovers:
                   each result the same call gives on a fresh model.
  hoisted status   SamplerPlan(mode="hoisted").status() after a launch on a
                   dirty cache is 0.

The references are the library's own results on clean memory; their accuracy
is the neighbouring modules' business (and test_gpu_dirty_entries.py's (d))."""
import numpy as np
import pytest
import torch

import dirty_state as DS
import ertdiff
from ertdiff import _lib
from ertdiff.unet import attention, conv2d, group_norm_act_bf16, group_norm_stats
from synth import synth_normal, synth_timesteps, synth_uniform

pytestmark = pytest.mark.gpu


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _flat(r, prefix="result"):
    if isinstance(r, torch.Tensor):
        return [(prefix, r)]
    if isinstance(r, dict):
        return [p for k, v in r.items() for p in _flat(v, f"{prefix}[{k!r}]")]
    if isinstance(r, (list, tuple)):
        return [p for k, v in enumerate(r) for p in _flat(v, f"{prefix}[{k}]")]
    return [(prefix, torch.as_tensor(np.asarray(r)))]


def assert_same(dirty, clean, finite=True):
    a, b = _flat(dirty), _flat(clean)
    assert [k for k, _ in a] == [k for k, _ in b]
    for (k, x), (_, y) in zip(a, b):
        DS.assert_same_bits(x, y, k, finite=finite)


def clean_vs_dirty(fn, monkeypatch, finite=True):
    clean = fn()
    torch.cuda.synchronize()
    with DS.dirty_allocator(monkeypatch):
        dirty = fn()
        torch.cuda.synchronize()
    assert_same(dirty, clean, finite)
    return clean


# ---- single operators ----------------------------------------------------------------------------
@pytest.mark.parametrize("Ca,Cb,Cout,H,mode,act,precision", [
    (64, 0, 64, 16, "same", "gn_silu", "fp32"),      # F(2x2) with its K split
    (20, 12, 40, 16, "up", "none", "fp32"),          # sub-pixel direct, ragged tiles
    (20, 0, 64, 16, "same", "gn_silu", "bf16"),      # bf16 image with pad lanes
])
def test_conv2d(Ca, Cb, Cout, H, mode, act, precision, monkeypatch, cuda_dev):
    B, Cin, d = 2, Ca + Cb, cuda_dev
    x, x2 = _rand((B, Ca, H, H), 1).to(d), _rand((B, Cb, H, H), 2).to(d) if Cb else None
    w, b = _rand((Cout, Cin, 3, 3), 3, 1.0 / np.sqrt(9 * Cin)).to(d), _rand((Cout,), 4, 0.1).to(d)
    gn = None
    if act != "none":
        gn = torch.stack([_rand((B, Cin), 5, 0.3) + 1.0, _rand((B, Cin), 6, 0.2)], -1).to(d)
    clean_vs_dirty(lambda: conv2d(x, w, b, mode=mode, act=act, gn=gn, x2=x2, precision=precision), monkeypatch)


def test_group_norm_and_attention(monkeypatch, cuda_dev):
    d = cuda_dev
    x, x2 = (_rand((3, 128, 32, 32), 12, 2.0) + 0.5).to(d), _rand((3, 64, 32, 32), 13).to(d)
    gamma, beta = (_rand((192,), 14) + 1).to(d), _rand((192,), 15).to(d)
    clean_vs_dirty(lambda: group_norm_stats(x, 32, gamma, beta, x2=x2), monkeypatch)
    clean_vs_dirty(lambda: group_norm_act_bf16(x, 32, gamma, beta, x2=x2), monkeypatch)
    qkv = _rand((1, 768, 256), 16, 0.5).to(d)
    clean_vs_dirty(lambda: attention(qkv), monkeypatch)


# ---- the U-Net ----------------------------------------------------------------------------------------
def _unet_inputs(name, B, L, dev, T=3):
    P = ertdiff.ConditionalUNet.from_config(name, seed=0).param_dim
    x = torch.from_numpy(synth_normal((B, P), 111)).to(dev)
    cond = torch.from_numpy(synth_uniform((B, 14, L), 112)).to(dev)
    t = torch.tensor([999, 5, 17, 400][:B], device=dev)
    noise = torch.from_numpy(synth_normal((T, B, P), 113)).to(dev)
    return P, x, cond, t, noise


def _unet_calls(name, B, L, dev, precision="fp32", T=3):
    """The public U-Net calls at one geometry, each on the model it is given."""
    P, x, cond, t, noise = _unet_inputs(name, B, L, dev, T)
    sched = ertdiff.get_diffusion_schedule(T, device=dev)
    ab50 = ertdiff.get_diffusion_schedule(50)[2]

    def forward(m):
        with torch.no_grad():
            return m(x, t, cond)

    def sample(m):
        return ertdiff.sample_model(m, cond, T, *sched, P, dev, noise=noise)

    def plan(m):
        p = ertdiff.UNetSamplerPlan(m, cond, T, *sched, noise=noise)
        p.x.copy_(noise[0])
        p.launch()
        torch.cuda.synchronize()
        out = p.x.clone()
        p.close()
        return out

    def fast(m):
        return ertdiff.sample_fast(m, cond, 50, ab50, P, timesteps=[49, 20, 0], solver="dpmpp_2m", noise=noise)

    def fast_plan(m):
        p = ertdiff.UNetSolverPlan(m, cond, 50, ab50, timesteps=[49, 20, 0], solver="dpmpp_2m", noise=noise)
        p.x.copy_(p.x_T())
        p.launch()
        torch.cuda.synchronize()
        out = p.x.clone()
        p.close()
        return out
    return {"forward": forward, "sample": sample, "plan": plan, "fast": fast, "fast_plan": fast_plan}


def _new_unet(name, dev, precision="fp32"):
    return ertdiff.ConditionalUNet.from_config(name, seed=0, precision=precision).to(dev).eval()


@pytest.mark.parametrize("call", ["forward", "sample", "plan", "fast", "fast_plan"])
def test_unet_clean_vs_dirty(call, monkeypatch, cuda_dev):
    fn = _unet_calls("U1", 3, 129, cuda_dev)[call]
    clean_vs_dirty(lambda: fn(_new_unet("U1", cuda_dev)), monkeypatch)


def test_unet_train_step_clean_vs_dirty(monkeypatch, cuda_dev):
    """unet_train_step (U1, B = 2, L = 65): the loss, every gradient and every
    parameter after the step."""
    from ertdiff.unet_train import unet_train_step
    dev, B, L, T = cuda_dev, 2, 65, 1000
    P = _new_unet("U1", dev).param_dim
    x0 = torch.from_numpy(synth_normal((B, P), 530)).to(dev)
    cond = torch.from_numpy(synth_uniform((B, 14, L), 531)).to(dev)
    t = torch.from_numpy(synth_timesteps(B, T, 532)).to(dev)
    noise = torch.from_numpy(synth_normal((B, P), 533)).to(dev)
    ab = ertdiff.get_diffusion_schedule(T, device=dev)[2]

    def fn():
        m = ertdiff.ConditionalUNet.from_config("U1", seed=9).to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        loss = unet_train_step(m, opt, x0, cond, T, ab, t=t, noise=noise, return_tensor=True)
        return {"loss": loss, "grads": [p.grad for p in m.parameters()],
                "params": [p.detach() for p in m.parameters()]}
    clean_vs_dirty(fn, monkeypatch)


def test_unet_preseeded_cache(cuda_dev):
    dev = cuda_dev
    calls = _unet_calls("U1", 3, 129, dev)
    for k in ("forward", "sample", "fast"):
        want = calls[k](_new_unet("U1", dev))
        m = _new_unet("U1", dev)
        n = m.workspace(dev, 3, 129).numel()
        m._ws[dev] = torch.full((2 * n,), 0xFF, dtype=torch.uint8, device=dev)
        assert_same(calls[k](m), want)
        assert m._ws[dev].numel() == 2 * n        # the seeded tensor was the one used


def test_unet_reuse_across_geometries(cuda_dev):
    """One ConditionalUNet (U3: attention) through forward (4, 257), forward
    (2, 129), a 3-step sample at B = 3, a solver sample, forward (4, 257)
    again: the cache only grows, so every later layout lands on leftovers."""
    dev = cuda_dev
    seq = [("forward", 4, 257), ("forward", 2, 129), ("sample", 3, 129), ("fast", 3, 129), ("forward", 4, 257)]
    shared = _new_unet("U3", dev)
    for k, B, L in seq:
        fn = _unet_calls("U3", B, L, dev)[k]
        assert_same(fn(shared), fn(_new_unet("U3", dev)))


# ---- the reference model ----------------------------------------------------------------------------
def _fresh_model(golden_weights, dev, train=False):
    m = ertdiff.ConditionalDiffusionModel(29, 128)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_weights.items()})
    m = m.to(dev)
    return m.train() if train else m.eval()


def _ref_inputs(B, L, T, dev):
    x = torch.from_numpy(synth_normal((B, 29), 1)).to(dev)
    t = torch.from_numpy(synth_timesteps(B, T, 3)).to(dev)
    cond = torch.from_numpy(synth_uniform((B, 14, L), 2)).to(dev)
    noise = torch.from_numpy(synth_normal((T, B, 29), 4)).to(dev)
    return x, t, cond, noise


@pytest.mark.parametrize("call", ["forward", "hoisted", "faithful", "faithful_steps"])
def test_reference_model_clean_vs_dirty(call, golden_weights, monkeypatch, cuda_dev):
    dev, B, L, T = cuda_dev, 3, 37, 5
    x, t, cond, noise = _ref_inputs(B, L, T, dev)
    sched = ertdiff.get_diffusion_schedule(T, device=dev)

    def fn():
        m = _fresh_model(golden_weights, dev)
        with torch.no_grad():
            if call == "forward":
                return m(x, t, cond, return_intermediates=True)
            return ertdiff.sample_model(m, cond, T, *sched, 29, dev, noise=noise, mode=call)
    clean_vs_dirty(fn, monkeypatch)


@pytest.mark.parametrize("call", ["train_step", "plan_step", "plan_run", "run_epoch", "validation"])
def test_reference_train_clean_vs_dirty(call, golden_weights, monkeypatch, cuda_dev):
    dev, B, L, T = cuda_dev, 3, 37, 500
    x0, t, cond, _ = _ref_inputs(7, L, T, dev)
    noise = torch.from_numpy(synth_normal((7, 29), 5)).to(dev)
    ab = ertdiff.get_diffusion_schedule(T, device=dev)[2]
    order = torch.tensor([3, 0, 6, 1, 5, 2, 4])

    def fn():
        m = _fresh_model(golden_weights, dev, train=True)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        r = {}
        if call == "train_step":
            r["loss"] = ertdiff.train_step(m, opt, x0[:B], cond[:B], T, ab, t=t[:B], noise=noise[:B], return_tensor=True)
        elif call == "validation":
            val = ertdiff.ValidationPlan(m, B, L, T, ab, seed=11)
            r["loss"] = val.run(ertdiff.DeviceDataset(x0, cond), order)
            r["eps"], r["t"], r["noise"] = val.eps.clone(), val.t.clone(), val.noise.clone()
            return r
        else:
            plan = ertdiff.TrainPlan(m, opt, B, L, T, ab, seed=11)
            if call == "plan_step":
                r["loss"] = plan.step(x0[:B], cond[:B], t=t[:B], noise=noise[:B], return_tensor=True)
            elif call == "plan_run":
                plan.x0.copy_(x0[:B])
                plan.cond.copy_(cond[:B])
                plan.run(3)
                r["loss"], r["t"], r["noise"] = plan.loss.clone(), plan.t.clone(), plan.noise.clone()
            else:
                r["loss"] = plan.run_epoch(ertdiff.DeviceDataset(x0, cond), order)
                r["t"], r["noise"] = plan.epoch_t.clone(), plan.epoch_noise.clone()
        torch.cuda.synchronize()
        r["grads"] = [p.grad.clone() for p in m.parameters()]
        r["params"] = [p.detach().clone() for p in m.parameters()]
        r["exp_avg"] = [opt.state[p]["exp_avg"].clone() for p in m.parameters()]
        r["exp_avg_sq"] = [opt.state[p]["exp_avg_sq"].clone() for p in m.parameters()]
        r["step"] = [opt.state[p]["step"].clone() for p in m.parameters()]
        return r
    clean_vs_dirty(fn, monkeypatch)


def test_reference_preseeded_cache_and_reuse(golden_weights, gpu_model, cuda_dev):
    """A 0xFF tensor of twice the needed size in model._ws[(dev, op)], then one
    model through faithful (3, 37, 5), hoisted (5, 250, 3), faithful again,
    with a forward in between: each the fresh model's bits."""
    dev = cuda_dev

    def calls(B, L, T, mode):
        x, t, cond, noise = _ref_inputs(B, L, T, dev)
        sched = ertdiff.get_diffusion_schedule(T, device=dev)

        def forward(m):
            with torch.no_grad():
                return m(x, t, cond)
        return forward, lambda m: ertdiff.sample_model(m, cond, T, *sched, 29, dev, noise=noise, mode=mode)
    shared = _fresh_model(golden_weights, dev)
    lib = _lib.lib()
    for op, (B, L, T) in ((_lib.OP_FORWARD, (3, 37, 0)), (_lib.OP_SAMPLE, (3, 37, 5))):
        n = max(lib.ertd_workspace_bytes(B, L, 29, T, op), 256)
        shared._ws[(dev, op)] = torch.full((2 * n,), 0xFF, dtype=torch.uint8, device=dev)
    for B, L, T, mode in ((3, 37, 5, "faithful"), (5, 250, 3, "hoisted"), (3, 37, 5, "faithful")):
        forward, sample = calls(B, L, T, mode)
        assert_same(forward(shared), forward(_fresh_model(golden_weights, dev)))
        assert_same(sample(shared), sample(_fresh_model(golden_weights, dev)))


def test_hoisted_plan_status_on_dirty_workspace(golden_weights, cuda_dev):
    """SamplerPlan.status() reads the status word of its workspace whatever the
    mode; the hoisted schedule has no wait that could time out, and clears the
    word like the faithful schedules do (it once returned before the clear, so
    a workspace that had held anything else reported a timeout)."""
    dev, B, L, T = cuda_dev, 3, 37, 5
    _, _, cond, noise = _ref_inputs(B, L, T, dev)
    sched = ertdiff.get_diffusion_schedule(T, device=dev)
    m = _fresh_model(golden_weights, dev)
    n = max(_lib.lib().ertd_workspace_bytes(B, L, 29, T, _lib.OP_SAMPLE), 256)
    m._ws[(dev, _lib.OP_SAMPLE)] = torch.full((2 * n,), 0xFF, dtype=torch.uint8, device=dev)
    for mode in ("hoisted", "faithful"):
        plan = ertdiff.SamplerPlan(m, cond, T, *sched, mode=mode, noise=noise)
        plan.x.copy_(noise[0])
        plan.launch()
        assert plan.status() == 0, mode
        plan.x.copy_(noise[0])
        plan.enqueue_direct()
        assert plan.status() == 0, mode
        want = ertdiff.sample_model(_fresh_model(golden_weights, dev), cond, T, *sched, 29, dev, noise=noise, mode=mode)
        assert_same(plan.x, want)
        plan.close()
        m._ws[(dev, _lib.OP_SAMPLE)].fill_(0xFF)


# ---- post-processing, statistics, data preparation ---------------------------------------------------
def test_postprocess_and_stats_clean_vs_dirty(postproc_chain_kat, monkeypatch, cuda_dev):
    dev = cuda_dev
    k = postproc_chain_kat
    u = torch.from_numpy(k["u"]).to(dev)
    clean_vs_dirty(lambda: ertdiff.postprocess(u, (k["min_"], k["scale_"]), k["limits"]), monkeypatch, finite=False)
    n, cells = 50, 29
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n, cells, generator=g, dtype=torch.float64).to(dev)
    clean_vs_dirty(lambda: ertdiff.ensemble_percentile(x, [2.5, 25, 50, 75, 97.5]), monkeypatch)
    clean_vs_dirty(lambda: ertdiff.ensemble_moments(x), monkeypatch)
    gen = torch.randn(n, 11, cells, generator=g, dtype=torch.float64).to(dev)
    true = torch.randn(11, cells, generator=g, dtype=torch.float64).to(dev)
    clean_vs_dirty(lambda: ertdiff.coverage_counts(gen, true), monkeypatch)
    pred = torch.randn(n, cells, 14, generator=g, dtype=torch.float64).to(dev)
    obs = torch.randn(cells, 14, generator=g, dtype=torch.float64).to(dev)
    clean_vs_dirty(lambda: ertdiff.wsse(pred, obs), monkeypatch)
    M = _lib.lib().ertd_rows_sort_tile(0) + 7
    sim = torch.randn(3, M, generator=g).to(dev)
    ob = torch.randn(M, generator=g).to(dev)
    clean_vs_dirty(lambda: ertdiff.sort_rows(sim), monkeypatch)
    clean_vs_dirty(lambda: ertdiff.wasserstein(sim, ob), monkeypatch)


def test_kde_clean_vs_dirty(kde_kat, monkeypatch, cuda_dev):
    x = torch.from_numpy(kde_kat["x"]).to(cuda_dev)      # (40, 48): the smallest fixture
    clean_vs_dirty(lambda: ertdiff.ensemble_mode(x, grid=int(kde_kat["grid"])), monkeypatch)


def test_data_preparation_clean_vs_dirty(monkeypatch, cuda_dev):
    dev, n, L = cuda_dev, 5, 37
    g = torch.Generator().manual_seed(9)
    X = torch.randn(300, 14, generator=g, dtype=torch.float64)
    par = torch.rand(n, 29, 1, generator=g, dtype=torch.float64).numpy()
    ert = (torch.rand(n, L, 14, generator=g, dtype=torch.float64) * 100 + 1).numpy()

    def scaler():
        s = ertdiff.DeviceMinMaxScaler(device=dev)
        s.partial_fit(X[:100].to(dev))
        s.partial_fit(X[100:].to(dev))
        return {"y": s.transform(X.to(dev)), "min_": torch.as_tensor(s.min_), "scale_": torch.as_tensor(s.scale_)}
    clean_vs_dirty(scaler, monkeypatch)

    def prep():
        ds, ps, es = ertdiff.prepare_dataset(par, ert, dev)
        return {"x0": ds.x0, "cond": ds.cond, "pmin": torch.as_tensor(ps.min_), "emin": torch.as_tensor(es.min_),
                "escale": torch.as_tensor(es.scale_)}
    clean_vs_dirty(prep, monkeypatch)
