"""Whole epochs from a device-resident dataset (TrainPlan.run_epoch,
ValidationPlan, fit) against the per-batch eager train_step on the gathered
batch -- bit for bit: the kernels read the same numbers in the same order --
and against the float64 restatement of the reference's step.

Shapes: N = 11 rows at L = 37 with B = 4 (batches of 4, 4, 3: one strip per
member, a partial last batch) and N = 5 at L = 4693 with B = 2 (2, 2, 1: many
strips per member, B_last = 1).  The orders are non-monotone, include rows 0 and
N - 1 and repeat a row in two batches."""
import numpy as np
import pytest
import torch

import ertdiff
from conftest import record_error
from oracle import ref_numpy as RN
from synth import synth_normal, synth_uniform

pytestmark = pytest.mark.gpu

T = 500
SHAPES = {
    "small": dict(N=11, L=37, B=4, order=[10, 3, 0, 7, 5, 3, 9, 1, 8, 0, 2],
                  order2=[2, 10, 6, 0, 4, 4, 1, 9, 0, 10, 5], short=[6, 0, 10, 2, 6, 3, 1]),
    "long": dict(N=5, L=4693, B=2, order=[4, 0, 2, 0, 3], order2=[1, 4, 4, 0, 2], short=[3, 0, 4]),
}
_DATA = {}


def _case(name, dev):
    """(spec, DeviceDataset) of a shape; the dataset is made once and never written."""
    s = SHAPES[name]
    if name not in _DATA:
        x0 = torch.from_numpy(synth_normal((s["N"], 29), 700 + s["L"])).to(dev)
        cond = torch.from_numpy(synth_uniform((s["N"], 14, s["L"]), 701 + s["L"])).to(dev)
        _DATA[name] = ertdiff.DeviceDataset(x0, cond)
    return s, _DATA[name]


def _fresh(golden_weights, dev):
    m = ertdiff.ConditionalDiffusionModel(29, 128)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_weights.items()})
    m = m.to(dev).train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-4)


def _ab(dev):
    return ertdiff.get_diffusion_schedule(T, device=dev)[2]


def _draws(n, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randint(0, T, (n,), device=dev, generator=g),
            torch.randn(n, 29, device=dev, generator=g))


def _eager_epoch(m, opt, data, order, B, ab, t, noise):
    """The loop a user writes without run_epoch: gather, then the eager step."""
    order = torch.as_tensor(order, device=data.device)
    losses = []
    for i0 in range(0, order.numel(), B):
        idx = order[i0:i0 + B]
        losses.append(ertdiff.train_step(m, opt, data.x0[idx], data.cond[idx], T, ab, t=t[i0:i0 + B],
                                         noise=noise[i0:i0 + B], return_tensor=True))
    return torch.stack(losses)


def _assert_same(m1, o1, m2, o2, steps):
    for (k, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p1, p2), k
        assert torch.equal(p1.grad, p2.grad), k
        s1, s2 = o1.state[p1], o2.state[p2]
        assert float(s1["step"]) == float(s2["step"]) == float(steps), k
        assert torch.equal(s1["exp_avg"], s2["exp_avg"]), k
        assert torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"]), k


@pytest.mark.parametrize("name", ["small", "long"])
def test_epoch_equals_eager_steps_explicit_draws(name, golden_weights, cuda_dev):
    s, data = _case(name, cuda_dev)
    ab = _ab(cuda_dev)
    order = torch.tensor(s["order"])
    t, noise = _draws(order.numel(), 811, cuda_dev)
    m1, o1 = _fresh(golden_weights, cuda_dev)
    plan = ertdiff.TrainPlan(m1, o1, s["B"], s["L"], T, ab)
    losses = plan.run_epoch(data, order, t=t, noise=noise)
    m2, o2 = _fresh(golden_weights, cuda_dev)
    ref = _eager_epoch(m2, o2, data, order, s["B"], ab, t, noise)
    nb = -(-order.numel() // s["B"])
    assert tuple(losses.shape) == (nb,) and losses.is_cuda
    assert torch.equal(losses, ref), (losses, ref)
    _assert_same(m1, o1, m2, o2, nb)
    assert torch.equal(plan.epoch_t, t) and torch.equal(plan.epoch_noise, noise)


@pytest.mark.parametrize("name", ["small", "long"])
def test_epoch_device_draws(name, golden_weights, cuda_dev):
    s, data = _case(name, cuda_dev)
    ab = _ab(cuda_dev)
    B = s["B"]
    order = torch.tensor(s["order"], device=cuda_dev)   # a device order: one aminmax
    m1, o1 = _fresh(golden_weights, cuda_dev)
    plan = ertdiff.TrainPlan(m1, o1, B, s["L"], T, ab, seed=4321)
    losses = plan.run_epoch(data, order)
    t, noise = plan.epoch_t.clone(), plan.epoch_noise.clone()
    assert int(t.min()) >= 0 and int(t.max()) < T
    assert not torch.equal(noise[:B], noise[B:2 * B])   # every step its own draws
    m2, o2 = _fresh(golden_weights, cuda_dev)
    ref = _eager_epoch(m2, o2, data, order, B, ab, t, noise)
    assert torch.equal(losses, ref)
    _assert_same(m1, o1, m2, o2, losses.numel())
    # the first (full) batch's draws are plan.step()'s at the same seed and Adam step
    m3, o3 = _fresh(golden_weights, cuda_dev)
    plan3 = ertdiff.TrainPlan(m3, o3, B, s["L"], T, ab, seed=4321)
    idx = order[:B]
    l3 = plan3.step(data.x0[idx], data.cond[idx], return_tensor=True)
    assert torch.equal(plan3.t, t[:B]) and torch.equal(plan3.noise, noise[:B])
    assert torch.equal(l3, losses[0])


def test_second_epoch_new_order_other_length_then_steps(golden_weights, cuda_dev):
    s, data = _case("small", cuda_dev)
    ab = _ab(cuda_dev)
    B = s["B"]
    m1, o1 = _fresh(golden_weights, cuda_dev)
    plan = ertdiff.TrainPlan(m1, o1, B, s["L"], T, ab, seed=99)
    m2, o2 = _fresh(golden_weights, cuda_dev)
    steps = 0
    # two epochs of one length (the second replays the captured graph on a new
    # order), then an epoch of another length
    for k, order in enumerate((s["order"], s["order2"], s["short"])):
        order = torch.tensor(order)
        t, noise = _draws(order.numel(), 820 + k, cuda_dev)
        losses = plan.run_epoch(data, order, t=t, noise=noise)
        ref = _eager_epoch(m2, o2, data, order, B, ab, t, noise)
        assert torch.equal(losses, ref), k
        steps += losses.numel()
        _assert_same(m1, o1, m2, o2, steps)
    assert steps == 8
    # drop_last leaves the partial batch out
    order = torch.tensor(s["order"])
    t, noise = _draws(8, 830, cuda_dev)
    losses = plan.run_epoch(data, order, t=t, noise=noise, drop_last=True)
    ref = _eager_epoch(m2, o2, data, order[:8], B, ab, t, noise)
    assert torch.equal(losses, ref) and losses.numel() == 2
    steps += 2
    # plan.step and plan.run go on from there
    idx = torch.tensor([1, 0, 10, 5], device=cuda_dev)
    t, noise = _draws(B, 831, cuda_dev)
    la = plan.step(data.x0[idx], data.cond[idx], t=t, noise=noise)
    lb = ertdiff.train_step(m2, o2, data.x0[idx], data.cond[idx], T, ab, t=t, noise=noise)
    assert la == lb
    steps += 1
    _assert_same(m1, o1, m2, o2, steps)
    plan.run(2)
    torch.cuda.synchronize()
    assert float(o1.state_dict()["state"][0]["step"]) == steps + 2
    assert np.isfinite(float(plan.loss))


@pytest.mark.parametrize("name", ["small", "long"])
def test_epoch_vs_float64_reference(name, golden_weights, cuda_dev):
    """oracle.ref_numpy.train_steps' body (q_sample -> forward -> backward ->
    Adam, float64) batch by batch over the gathered rows, the Adam state carried
    across the batches; tolerances of tests/test_gpu_train.py."""
    s, data = _case(name, cuda_dev)
    ab = _ab(cuda_dev)
    B = s["B"]
    order = np.asarray(s["order"])
    t, noise = _draws(order.size, 840, cuda_dev)
    m1, o1 = _fresh(golden_weights, cuda_dev)
    plan = ertdiff.TrainPlan(m1, o1, B, s["L"], T, ab)
    losses = plan.run_epoch(data, torch.from_numpy(order), t=t, noise=noise).cpu().numpy()
    x0, cond = data.x0.cpu().numpy(), data.cond.cpu().numpy()
    tn, nn = t.cpu().numpy(), noise.cpu().numpy()
    ab32 = np.cumprod(1.0 - np.linspace(1e-4, 0.02, T, dtype=np.float32), dtype=np.float32)
    params = {k: np.asarray(golden_weights[k], np.float64) for k in RN.KEYS}
    state = {}
    for i, i0 in enumerate(range(0, order.size, B)):
        idx = order[i0:i0 + B]
        xn = RN.q_sample(x0[idx], tn[i0:i0 + B], nn[i0:i0 + B], ab32.astype(np.float64))
        f = RN.forward_full(xn, tn[i0:i0 + B], cond[idx], params)
        loss, g = RN.backward(f, nn[i0:i0 + B], params)
        params = RN.adam_update(params, g, state, lr=1e-4)
        err = abs(float(losses[i]) - loss) / abs(loss)
        record_error(f"epoch_{name}_loss{i}_vs_fp64", err)
        print(f"{name} batch {i}: loss rel err {err:.3e}")
        assert err <= 1e-5, (i, float(losses[i]), loss)
    for k, p in m1.named_parameters():
        d = p.detach().double().cpu().numpy() - golden_weights[k]
        dref = params[k] - golden_weights[k].astype(np.float64)
        err = RN.rel_l2(d, dref)
        record_error(f"epoch_{name}_delta_{k}_vs_fp64", err)
        print(f"{name} {k}: Adam delta rel-L2 {err:.3e}")
        assert err < 1e-3, (k, err)


def test_validation_plan(golden_weights, cuda_dev):
    s, data = _case("small", cuda_dev)
    ab = _ab(cuda_dev)
    B = s["B"]
    rows = torch.tensor(s["order"])
    m, o = _fresh(golden_weights, cuda_dev)
    t1, n1 = _draws(B, 850, cuda_dev)
    ertdiff.train_step(m, o, data.x0[:B], data.cond[:B], T, ab, t=t1, noise=n1)  # Adam state exists
    before = [p.detach().clone() for p in m.parameters()]
    state = [(float(o.state[p]["step"]), o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone())
             for p in m.parameters()]
    val = ertdiff.ValidationPlan(m, B, s["L"], T, ab, seed=2024)
    losses = val.run(data, rows)
    nb = -(-rows.numel() // B)
    assert tuple(losses.shape) == (nb,) and tuple(val.eps.shape) == (rows.numel(), 29)
    t, noise, eps = val.t.clone(), val.noise.clone(), val.eps.clone()
    assert int(t.min()) >= 0 and int(t.max()) < T
    m.eval()
    for i, i0 in enumerate(range(0, rows.numel(), B)):
        idx = rows[i0:i0 + B].to(cuda_dev)
        tb, nb_ = t[i0:i0 + B], noise[i0:i0 + B]
        with torch.no_grad():
            ref = m(ertdiff.q_sample(data.x0[idx], tb, nb_, ab), tb, data.cond[idx])
        e = eps[i0:i0 + B]
        err = RN.rel_l2(e.double().cpu().numpy(), ref.double().cpu().numpy())
        record_error(f"validation_eps_batch{i}_vs_forward", err)
        assert err <= 1e-5, (i, err)
        mse = float(((e.double() - nb_.double()) ** 2).mean())
        lerr = abs(float(losses[i]) - mse) / mse
        record_error(f"validation_loss_batch{i}_vs_fp64_mean", lerr)
        assert lerr <= 1e-5, (i, float(losses[i]), mse)
    m.train()
    # forward only: parameters and Adam state bitwise unchanged
    for p, b, (st, ea, es) in zip(m.parameters(), before, state):
        assert torch.equal(p, b)
        assert float(o.state[p]["step"]) == st
        assert torch.equal(o.state[p]["exp_avg"], ea) and torch.equal(o.state[p]["exp_avg_sq"], es)
    # a second call draws anew; a second plan with the seed repeats the first
    val.run(data, rows)
    t2, n2 = val.t.clone(), val.noise.clone()
    assert not torch.equal(t2, t) and not torch.equal(n2, noise)
    val_b = ertdiff.ValidationPlan(m, B, s["L"], T, ab, seed=2024)
    lb = val_b.run(data, rows)
    assert torch.equal(val_b.t, t) and torch.equal(val_b.noise, noise) and torch.equal(lb, losses)
    # explicit draws are used as given
    lc = val_b.run(data, rows, t=t, noise=noise)
    assert torch.equal(lc, losses) and torch.equal(val_b.eps, eps)
    # a TrainPlan on the same seed draws another stream: validation batch 1 has
    # counter 1, the Adam step of the epoch's batch 0 -- same (member, counter)
    m2, o2 = _fresh(golden_weights, cuda_dev)
    plan = ertdiff.TrainPlan(m2, o2, B, s["L"], T, ab, seed=2024)
    plan.run_epoch(data, rows)
    assert not torch.equal(plan.epoch_t[:B], t[B:2 * B])
    assert not torch.equal(plan.epoch_noise[:B], noise[B:2 * B])
    # ... and it is the derived seed alone that separates them
    m3, o3 = _fresh(golden_weights, cuda_dev)
    plan3 = ertdiff.TrainPlan(m3, o3, B, s["L"], T, ab, seed=val.val_seed)
    plan3.run_epoch(data, rows)
    assert torch.equal(plan3.epoch_t[:B], t[B:2 * B])
    assert torch.equal(plan3.epoch_noise[:B], noise[B:2 * B])


def test_guards_raise_before_any_launch(golden_weights, cuda_dev):
    s, data = _case("small", cuda_dev)
    _, other = _case("long", cuda_dev)   # another L
    ab = _ab(cuda_dev)
    B, N = s["B"], s["N"]
    m, o = _fresh(golden_weights, cuda_dev)
    plan = ertdiff.TrainPlan(m, o, B, s["L"], T, ab)
    val = ertdiff.ValidationPlan(m, B, s["L"], T, ab)
    before = [p.detach().clone() for p in m.parameters()]
    t, noise = _draws(4, 860, cuda_dev)
    good = torch.tensor([0, 1, 2, 3])
    for run in (plan.run_epoch, val.run):
        for bad in ([0, N, 1], [2, -1, 3]):
            for dev in ("cpu", cuda_dev):
                with pytest.raises(IndexError):
                    run(data, torch.tensor(bad, device=dev))
        with pytest.raises(RuntimeError):
            run(other, torch.tensor([0, 1]))                    # wrong L
        with pytest.raises(RuntimeError):
            run(data, torch.tensor([], dtype=torch.int64))      # empty
        with pytest.raises(RuntimeError):
            run(data, torch.tensor([0.0, 1.0]))                 # not integers
        with pytest.raises(RuntimeError):
            run(data, good, t=t)                                # t without noise
        with pytest.raises(RuntimeError):
            run(data, good, t=t[:2], noise=noise)               # misshapen t
        bad_t = t.clone()
        bad_t[1] = T
        with pytest.raises(IndexError):
            run(data, good, t=bad_t, noise=noise)
    with pytest.raises(RuntimeError):
        plan.run_epoch(data, torch.tensor([0, 1, 2]), drop_last=True)   # nothing left
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(m.parameters(), before))
    assert all(float(o.state[p]["step"]) == 0.0 for p in m.parameters())
    assert plan.host_step == 0 and val.ctr == 0


def test_fit_three_epochs(golden_weights, cuda_dev, tmp_path):
    s, data = _case("small", cuda_dev)
    ab = _ab(cuda_dev)
    B = s["B"]
    train_idx = torch.tensor([0, 2, 3, 5, 6, 8, 9, 10, 1])   # 4, 4, 1
    val_idx = torch.tensor([7, 4])
    path = str(tmp_path / "best_model.pt")
    m1, o1 = _fresh(golden_weights, cuda_dev)
    out = ertdiff.fit(m1, o1, data, train_idx, val_idx, T, ab, num_epochs=3, batch_size=B,
                      checkpoint_path=path, generator=torch.Generator().manual_seed(5), seed=77)
    # the same loop by hand
    m2, o2 = _fresh(golden_weights, cuda_dev)
    plan = ertdiff.TrainPlan(m2, o2, B, s["L"], T, ab, seed=77)
    val = ertdiff.ValidationPlan(m2, B, s["L"], T, ab, seed=77)
    g = torch.Generator().manual_seed(5)
    th, vh, best, best_epoch, best_sd = [], [], float("inf"), 0, None
    for epoch in range(3):
        order = train_idx[torch.randperm(train_idx.numel(), generator=g)]
        th.append(ertdiff.epoch_loss(plan.run_epoch(data, order), train_idx.numel(), B))
        vh.append(ertdiff.epoch_loss(val.run(data, val_idx), val_idx.numel(), B))
        if vh[-1] < best:
            best, best_epoch = vh[-1], epoch + 1
            best_sd = {k: v.detach().clone() for k, v in m2.state_dict().items()}
    assert out["train_history"] == th and out["val_history"] == vh
    assert out["best_val_loss"] == best and out["best_epoch"] == best_epoch
    assert all(np.isfinite(th)) and all(np.isfinite(vh))
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p1, p2)
    m3 = ertdiff.ConditionalDiffusionModel(29, 128).to(cuda_dev)
    ckpt = ertdiff.load_best_model(path, m3, map_location=cuda_dev)
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_val_loss",
                         "train_history", "val_history", "param_dim"}
    assert ckpt["epoch"] == best_epoch and ckpt["best_val_loss"] == best and ckpt["param_dim"] == 29
    assert ckpt["train_history"] == th[:best_epoch] and ckpt["val_history"] == vh[:best_epoch]
    for k, v in m3.state_dict().items():
        assert torch.equal(v, best_sd[k]), k
    o4 = torch.optim.Adam(m3.parameters(), lr=1e-4)
    o4.load_state_dict(ckpt["optimizer_state_dict"])
