"""Training path on the GPU (ERT_Conditional_Diffusion.py:294-320).

  DiffusionForwardFn   autograd.Function: model(x, t, cond) under autograd runs
                       the HIP training forward (activations kept in a per-call
                       workspace) and, on backward, the HIP backward: gradients
                       of all 12 parameters (and of x).  So the reference's own
                       loop -- MSELoss, loss.backward(), optimizer.step() --
                       works unchanged on an ertdiff model.
  train_step           the reference's train-step body (:309-320) fused into one
                       library call: q_sample -> forward -> MSELoss -> backward
                       -> Adam, updating the torch.optim.Adam state in place so
                       optimizer.state_dict() stays valid (:348).
  TrainPlan            the same step for a fixed (B, L) captured once as a graph
                       (the draws of t and noise and the Adam step count on the
                       device): the reference loop's 63,500 steps at one graph
                       launch each.
  validation_loss      the no-grad validation pass body (:327-336).
  TrainPlan.run_epoch  one whole epoch (:308-320) as ONE graph replay: the train
                       kernels read each batch out of a device-resident
                       DeviceDataset through a row index (no gather, no copy, no
                       per-step call boundary, no host sync), the partial last
                       batch included; per-batch losses stay on the device.
  ValidationPlan       the validation pass (:325-338) the same way, forward only.
  epoch_loss           the reference's size-weighted epoch mean (:320-322, :336-338).
  fit                  the loop of :305-356 on those three.
"""
from __future__ import annotations

import ctypes
import weakref

import torch
import torch.nn.functional as F
from torch.autograd.graph import increment_version

from . import _lib
from .schedule import timestep_frequencies


def _train_ws(dev, B, L, P):
    n = _lib.lib().ertd_workspace_bytes(B, L, P, 0, _lib.OP_TRAIN)
    return torch.empty(max(n, 256), dtype=torch.uint8, device=dev)


class DiffusionForwardFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, t, cond, *params):
        dev = x.device
        x = _lib.f32c(x, "x")
        cond = _lib.f32c(cond, "condition")
        tt = t.to(torch.int64).contiguous()
        B, L, P = x.shape[0], cond.shape[2], model.param_dim
        ws = _train_ws(dev, B, L, P)
        eps = torch.empty(B, P, dtype=torch.float32, device=dev)
        freq = timestep_frequencies(_lib.HIDDEN, dev)
        w = model.weights_struct()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ertd_train_forward(
                ctypes.byref(w), None, x.data_ptr(), None, None, None, tt.data_ptr(),
                cond.data_ptr(), B, L, freq.data_ptr(), eps.data_ptr(), ws.data_ptr(), ws.numel(),
                _lib.stream_of(dev)), "train_forward")
        ctx.model = model
        ctx.ws, ctx.cond, ctx.B, ctx.L = ws, cond, B, L
        ctx.save_for_backward(*params)
        return eps

    @staticmethod
    def backward(ctx, grad_eps):
        params = ctx.saved_tensors
        dev = grad_eps.device
        dout = _lib.f32c(grad_eps, "grad")
        grads = [torch.empty_like(p) for p in params]
        dx = (torch.empty(ctx.B, ctx.model.param_dim, dtype=torch.float32, device=dev)
              if ctx.needs_input_grad[1] else None)
        w = ctx.model.weights_struct()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ertd_train_backward(
                ctypes.byref(w), None, dout.data_ptr(), None, ctx.cond.data_ptr(),
                ctx.B, ctx.L, _lib.ptr_array(grads), None, _lib.ptr(dx), ctx.ws.data_ptr(),
                ctx.ws.numel(), _lib.stream_of(dev)), "train_backward")
        return (None, dx, None, None, *grads)


def _adam_hparams(optimizer, params):
    if not isinstance(optimizer, torch.optim.Adam):
        raise RuntimeError("ertdiff.train_step drives torch.optim.Adam (the reference optimizer, :294)")
    if len(optimizer.param_groups) != 1:
        raise RuntimeError("ertdiff.train_step expects one parameter group")
    g = optimizer.param_groups[0]
    gp = g["params"]
    if len(gp) != len(params) or any(a is not b for a, b in zip(gp, params)):
        raise RuntimeError("optimizer parameters must be model.parameters() in module order")
    if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
        raise RuntimeError("ertdiff Adam supports weight_decay=0, amsgrad=False, maximize=False")
    lr = g["lr"]
    if isinstance(lr, torch.Tensor):
        lr = float(lr)
    return float(lr), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])


def _adam_state(optimizer, params):
    """exp_avg / exp_avg_sq of every parameter, created as torch.optim.Adam
    creates them on its first step (step = 0-dim float32 CPU tensor)."""
    exp_avg, exp_avg_sq = [], []
    for p in params:
        st = optimizer.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        exp_avg.append(st["exp_avg"])
        exp_avg_sq.append(st["exp_avg_sq"])
    return exp_avg, exp_avg_sq


_STEP_BASES = weakref.WeakKeyDictionary()   # optimizer -> the CPU tensor its step counters view


def _shared_step_base(optimizer, params):
    """ONE CPU float32 tensor per optimizer whose elements the 12
    optimizer.state[p]["step"] counters are views of, shared by every TrainPlan
    on that optimizer: a replay of any plan bumps it with one add_, and every
    other plan (and torch.optim.Adam itself, and the eager train_step) reads and
    bumps the same memory.  Re-made when the state no longer views it
    (optimizer.load_state_dict replaces the state tensors).  Returns
    (base, the state's own view tensors)."""
    base = _STEP_BASES.get(optimizer)
    steps = [optimizer.state[p]["step"] for p in params]
    if base is not None and base.numel() == len(params) and all(
            isinstance(s, torch.Tensor) and s.device.type == "cpu" and s.dtype == torch.float32
            and s.data_ptr() == base[i].data_ptr() for i, s in enumerate(steps)):
        return base, steps
    base = torch.tensor([float(s) for s in steps], dtype=torch.float32)
    for i, p in enumerate(params):
        optimizer.state[p]["step"] = base[i]
    _STEP_BASES[optimizer] = base
    return base, [optimizer.state[p]["step"] for p in params]


def _hp_key(g0):
    """The optimizer's lr / betas / eps by VALUE: a Tensor lr a scheduler
    fill_()s in place is the same object with another value."""
    lr = g0["lr"]
    return (float(lr) if isinstance(lr, torch.Tensor) else lr, g0["betas"], g0["eps"])


def _refuse_device_steps(optimizer, params):
    """capturable=True / fused=True keep state["step"] on the device, where the
    plan's host-side step bookkeeping cannot follow it."""
    g0 = optimizer.param_groups[0]
    if g0.get("capturable", False) or g0.get("fused", False):
        raise RuntimeError("ertdiff: TrainPlan needs host step counters; build the optimizer with "
                           "capturable=False and fused=False")
    for p in params:
        s = optimizer.state[p].get("step") if p in optimizer.state else None
        if isinstance(s, torch.Tensor) and s.device.type != "cpu":
            raise RuntimeError("ertdiff: TrainPlan needs host step counters; optimizer.state[p]['step'] "
                               f"is on {s.device}")


def train_step(model, optimizer, x0, cond, T, alpha_bar, *, t=None, noise=None,
               return_tensor: bool = False):
    """One reference train step (:309-320); returns loss.item() (or the device
    scalar if ``return_tensor``).  t / noise default to the reference's draws
    (torch.randint then torch.randn_like, :312-313)."""
    from .unet import ConditionalUNet
    if isinstance(model, ConditionalUNet):   # the same call surface over the U-Net denoiser
        from .unet_train import unet_train_step
        return unet_train_step(model, optimizer, x0, cond, T, alpha_bar, t=t, noise=noise,
                               return_tensor=return_tensor)
    model._check_supported()
    params = model._params()
    dev = _lib.require_device(x0, cond, alpha_bar, params[0])
    B = x0.size(0)
    if t is None:
        t = torch.randint(0, T, (B,), device=dev).long()
    if noise is None:
        noise = torch.randn_like(x0)
    x0 = _lib.f32c(x0, "x0")
    noise = _lib.f32c(noise, "noise")
    cond = _lib.f32c(cond, "condition")
    ab = _lib.f32c(alpha_bar, "alpha_bar")
    if ab.dim() != 1 or ab.numel() < int(T):   # the device reads alpha_bar[t], t < T
        raise IndexError(f"ertdiff: alpha_bar has {ab.numel()} entries, T = {T}")
    tt = t.to(device=dev, dtype=torch.int64).contiguous()
    model._check_inputs(x0, tt, cond)
    lr, b1, b2, eps = _adam_hparams(optimizer, params)
    exp_avg, exp_avg_sq = _adam_state(optimizer, params)
    for p in params:
        optimizer.state[p]["step"] += 1
        if p.grad is None:
            p.grad = torch.empty_like(p)
    step = int(optimizer.state[params[0]]["step"].item())
    grads = [p.grad for p in params]
    L = cond.shape[2]
    ws = model.workspace(dev, B, L, 0, _lib.OP_TRAIN)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    freq = timestep_frequencies(_lib.HIDDEN, dev)
    w = model.weights_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ertd_train_step(
            ctypes.byref(w), None, x0.data_ptr(), tt.data_ptr(), noise.data_ptr(),
            cond.data_ptr(), ab.data_ptr(), B, L, freq.data_ptr(), _lib.ptr_array(grads),
            _lib.ptr_array(exp_avg), _lib.ptr_array(exp_avg_sq), step, lr, b1, b2, eps,
            loss.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_of(dev)), "train_step")
    model._packed_key = None  # parameters changed in place behind autograd's back: re-pack
    increment_version(params)  # ... and say so to autograd
    return loss if return_tensor else loss.item()


def batch_sizes(n_rows: int, B: int):
    """The batch sizes DataLoader(batch_size=B, drop_last=False) yields over
    n_rows items: n_rows // B full batches, then the remainder if any."""
    n_rows, B = int(n_rows), int(B)
    return [B] * (n_rows // B) + ([n_rows % B] if n_rows % B else [])


def _epoch_order(order, n_data: int, B: int, drop_last: bool):
    """The epoch's row indices, checked on the host side BEFORE any launch (the
    device cannot report a bad index): (order, n_rows)."""
    if not isinstance(order, torch.Tensor):
        order = torch.as_tensor(order)
    if order.dtype.is_floating_point or order.dtype.is_complex or order.dtype == torch.bool:
        raise RuntimeError(f"ertdiff: the epoch order must be an integer tensor, got {order.dtype}")
    if order.dim() != 1:
        raise RuntimeError(f"ertdiff: the epoch order must be 1-D, got {tuple(order.shape)}")
    n = order.numel()
    if drop_last:
        n = n // B * B
        order = order[:n]
    if n == 0:
        raise RuntimeError("ertdiff: the epoch order is empty")
    lo, hi = torch.aminmax(order)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi >= n_data:
        raise IndexError(f"ertdiff: row index {lo if lo < 0 else hi} out of range [0, {n_data})")
    return order, n


def _check_data(data, dev, L: int, P: int):
    from .data import DeviceDataset
    if not isinstance(data, DeviceDataset):
        raise RuntimeError(f"ertdiff: expected a DeviceDataset, got {type(data).__name__}")
    x0, cond = data.x0, data.cond
    if x0.dtype != torch.float32 or cond.dtype != torch.float32:
        raise RuntimeError("ertdiff: the dataset must be float32")
    if not (x0.is_contiguous() and cond.is_contiguous()):
        raise RuntimeError("ertdiff: the dataset tensors must be contiguous")
    if x0.device != dev or cond.device != dev:
        raise RuntimeError(f"ertdiff: the dataset is on {x0.device}, the plan on {dev}")
    if x0.dim() != 2 or x0.shape[1] != P:
        raise RuntimeError(f"ertdiff: this plan takes x0 rows of {P} parameters, got {tuple(x0.shape)}")
    if cond.dim() != 3 or cond.shape[0] != x0.shape[0] or tuple(cond.shape[1:]) != (_lib.CIN, L):
        raise RuntimeError(f"ertdiff: this plan was captured for conditions (N, {_lib.CIN}, {L}), got "
                           f"{tuple(cond.shape)}")


def _check_draws(t, noise, n: int, P: int, n_alpha: int, what: str):
    """t / noise of a whole epoch: both or neither; True when the device draws."""
    if (t is None) != (noise is None):
        raise RuntimeError(f"ertdiff: {what} takes both t and noise, or neither")
    if t is None:
        return True
    if tuple(t.shape) != (n,) or tuple(noise.shape) != (n, P):
        raise RuntimeError(f"ertdiff: {what} takes t of shape ({n},) and noise of shape ({n}, {P})")
    if noise.dtype != torch.float32:
        raise RuntimeError(f"ertdiff: noise must be float32, got {noise.dtype}")
    tl = t.to(torch.int64)
    if int(tl.min()) < 0 or int(tl.max()) >= n_alpha:
        raise IndexError(f"ertdiff: t out of range [0, {n_alpha})")
    return False


class _EpochBufs:
    """The fixed buffers an epoch graph of n_rows rows addresses."""

    def __init__(self, n: int, B: int, P: int, dev, with_eps: bool = False):
        nb = -(-n // B)
        self.rows = torch.zeros(n, dtype=torch.int32, device=dev)
        self.t = torch.zeros(n, dtype=torch.int64, device=dev)
        self.noise = torch.zeros(n, P, dtype=torch.float32, device=dev)
        self.losses = torch.zeros(nb, dtype=torch.float32, device=dev)
        if with_eps:
            self.eps = torch.zeros(n, P, dtype=torch.float32, device=dev)
            self.ctr = torch.zeros(nb, dtype=torch.int32, device=dev)


class TrainPlan:
    """train_step for a fixed (B, L), captured ONCE as a graph
    (torch.cuda.CUDAGraph = hipGraph) and replayed per step: the draws
    t ~ U{0..T-1} and noise ~ N(0, 1) (:312-313), q_sample -> forward -> MSELoss
    -> backward -> Adam (the four kernels of csrc/train.hip).

    rng="philox" (default): the step draws t and noise itself inside its head
      kernel (Philox4x32-10 keyed by (seed, member, Adam step): reproducible,
      no extra launches); seed defaults to one drawn from torch's CPU generator.
    rng="torch": torch.randint / torch.randn_like on torch's own generator are
      captured too (graph-safe): the same numbers the reference's eager draws
      give after the same manual_seed, at the cost of their extra launches.  The Adam step count lives on the
    device (advanced inside the graph); the bias corrections come from a table
    the host formed as torch does (ertd_adam_table), so a replay needs no host
    scalars.  optimizer.state[p]["step"], exp_avg, exp_avg_sq and p.grad stay
    the torch.optim.Adam state of the eager path (optimizer.state_dict() is
    valid after every step, :348).

        plan = TrainPlan(model, optimizer, B, L, T, alpha_bar)
        loss = plan.step(x0, cond)                # == train_step(...), bit for bit
        plan.x0.copy_(...); plan.cond.copy_(...)  # or fill the inputs in place
        plan.run(n)                               # n steps, no per-step host sync
        losses = plan.run_epoch(data, order)      # a whole epoch of a DeviceDataset: one replay

    The graph addresses the parameters, their gradients and the Adam state:
    keep them (optimizer.step() / load_state_dict on the model copy in place;
    build a new plan after optimizer.load_state_dict(), which replaces the
    state tensors)."""

    TABLE = 65536  # Adam steps per table; a plan past its table re-captures

    def __init__(self, model, optimizer, B: int, L: int, T: int, alpha_bar, warmup: int = 1,
                 rng: str = "philox", seed=None):
        if rng not in ("philox", "torch"):
            raise ValueError("ertdiff: TrainPlan rng must be 'philox' or 'torch'")
        self.rng = rng
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        model._check_supported()
        self.model, self.optimizer, self.T = model, optimizer, int(T)
        self.params = model._params()
        dev = _lib.require_device(alpha_bar, self.params[0])
        self.dev, self.B, self.L = dev, int(B), int(L)
        P = model.param_dim
        self.lr, self.b1, self.b2, self.eps = _adam_hparams(optimizer, self.params)
        _refuse_device_steps(optimizer, self.params)
        self.alpha_bar = _lib.f32c(alpha_bar, "alpha_bar")
        # the head kernel draws t in [0, T) and reads alpha_bar[t] on the device:
        # a shorter schedule would read past its end (the reference's
        # alpha_bar[t] raises IndexError instead, :96-99)
        if self.alpha_bar.dim() != 1 or self.alpha_bar.numel() < self.T:
            raise IndexError(f"ertdiff: alpha_bar has {self.alpha_bar.numel()} entries, "
                             f"TrainPlan needs at least T = {self.T}")
        z = dict(dtype=torch.float32, device=dev)
        self.x0 = torch.zeros(B, P, **z)
        self.cond = torch.zeros(B, _lib.CIN, L, **z)
        self.t = torch.zeros(B, dtype=torch.int64, device=dev)
        self.noise = torch.zeros(B, P, **z)
        self.loss = torch.zeros((), **z)
        self.exp_avg, self.exp_avg_sq = _adam_state(optimizer, self.params)
        for p in self.params:
            if p.grad is None:
                p.grad = torch.empty_like(p)
        self.grads = [p.grad for p in self.params]
        # the 12 step counters become views of ONE CPU tensor: a replay bumps them
        # with one add_ instead of a 12-tensor foreach (host time per step);
        # torch.optim.Adam reads and bumps state["step"] in place alike.  The
        # tensor belongs to the OPTIMIZER, not to the plan: every plan on one
        # optimizer (one per sequence length L) counts the same steps
        self._step_base, self._steps = _shared_step_base(optimizer, self.params)
        self._hp_raw = _hp_key(optimizer.param_groups[0])
        self.ws = torch.empty(max(_lib.lib().ertd_workspace_bytes(B, L, P, 0, _lib.OP_TRAIN), 256),
                              dtype=torch.uint8, device=dev)
        self.freq = timestep_frequencies(_lib.HIDDEN, dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._graphs = {}
        self._ebufs = {}   # run_epoch: n_rows -> the buffers its graphs address
        self.epoch_t = self.epoch_noise = None   # the last epoch's draws
        self._table_at(int(self._steps[0].item()))
        # warm-up outside any capture (module load, lazily created state): the
        # forward + backward on the zero inputs, into scratch gradient buffers --
        # parameters, p.grad, Adam state and the generator are untouched
        w = model.weights_struct()
        scratch = torch.empty((), **z)
        scratch_grads = [torch.empty_like(p) for p in self.params]
        with torch.cuda.device(dev):
            for _ in range(max(1, int(warmup))):
                _lib.check(_lib.lib().ertd_train_forward(
                    ctypes.byref(w), None, None, self.x0.data_ptr(), self.noise.data_ptr(),
                    self.alpha_bar.data_ptr(), self.t.data_ptr(), self.cond.data_ptr(), B, L,
                    self.freq.data_ptr(), None, self.ws.data_ptr(), self.ws.numel(),
                    _lib.stream_of(dev)), "train_forward")
                _lib.check(_lib.lib().ertd_train_backward(
                    ctypes.byref(w), None, None, self.noise.data_ptr(), self.cond.data_ptr(), B, L,
                    _lib.ptr_array(scratch_grads), scratch.data_ptr(), None, self.ws.data_ptr(),
                    self.ws.numel(), _lib.stream_of(dev)), "train_backward")
            torch.cuda.synchronize(dev)
        del scratch_grads

    def _table_at(self, step0: int):
        """Adam scalars of steps step0+1 ... step0+TABLE; drops captured graphs
        (the table's first step is a kernel argument)."""
        n = self.TABLE
        host = torch.empty(n * 6, dtype=torch.float32)
        _lib.check(_lib.lib().ertd_adam_table(step0 + 1, n, self.lr, self.b1, self.b2, self.eps,
                                              host.data_ptr()), "adam_table")
        torch.cuda.synchronize(self.dev)
        self.table = host.to(self.dev)
        self.table_first = step0 + 1
        self.step_dev.fill_(step0)
        self.host_step = step0
        self._graphs = {}

    def _body(self, draw: bool, k: int = 1):
        dev_draw = draw and self.rng == "philox"
        if dev_draw and k > 1:   # k steps in ONE call: no gap between them in the graph
            w = self.model.weights_struct()
            _lib.check(_lib.lib().ertd_train_steps_dev(
                ctypes.byref(w), self.x0.data_ptr(), self.t.data_ptr(), self.noise.data_ptr(),
                self.cond.data_ptr(), self.alpha_bar.data_ptr(), self.B, self.L, self.freq.data_ptr(),
                _lib.ptr_array(self.grads), _lib.ptr_array(self.exp_avg), _lib.ptr_array(self.exp_avg_sq),
                self.step_dev.data_ptr(), self.table.data_ptr(), self.table_first, self.TABLE,
                1, self.T, self.seed, k, self.loss.data_ptr(), self.ws.data_ptr(),
                self.ws.numel(), _lib.stream_of(self.dev)), "train_steps_dev")
            return
        if k > 1:
            for _ in range(k):
                self._body(draw)
            return
        if draw and not dev_draw:
            self.t.random_(0, self.T)   # torch.randint(0, T, (B,)) (:312)
            self.noise.normal_()        # torch.randn_like(x0) (:313)
        w = self.model.weights_struct()
        _lib.check(_lib.lib().ertd_train_step_dev(
            ctypes.byref(w), self.x0.data_ptr(), self.t.data_ptr(), self.noise.data_ptr(),
            self.cond.data_ptr(), self.alpha_bar.data_ptr(), self.B, self.L, self.freq.data_ptr(),
            _lib.ptr_array(self.grads), _lib.ptr_array(self.exp_avg), _lib.ptr_array(self.exp_avg_sq),
            self.step_dev.data_ptr(), self.table.data_ptr(), self.table_first, self.TABLE,
            1 if dev_draw else 0, self.T, self.seed, self.loss.data_ptr(), self.ws.data_ptr(),
            self.ws.numel(), _lib.stream_of(self.dev)), "train_step_dev")

    def _graph(self, draw: bool, k: int = 1):
        """The step graph, or k consecutive steps in one graph (run(): the
        device advances the Adam step count and draws per step, so the k steps
        of one replay are k ordinary steps)."""
        g = self._graphs.get((draw, k))
        if g is None:
            with torch.cuda.device(self.dev):
                torch.cuda.synchronize(self.dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._body(draw, k)
            self._graphs[(draw, k)] = g
        return g

    def _sync_step(self):
        """Follow Adam steps taken outside the plan (eager train_step, a
        user's optimizer.step()) -- the step counters are host tensors -- and
        edits of the optimizer's lr / betas / eps (a scheduler): the table of
        Adam scalars is rebuilt from the current hyper-parameters."""
        raw = _hp_key(self.optimizer.param_groups[0])
        if raw != self._hp_raw:
            self._hp_raw = raw
            hp = _adam_hparams(self.optimizer, self.params)
            if hp != (self.lr, self.b1, self.b2, self.eps):
                self.lr, self.b1, self.b2, self.eps = hp
                self._table_at(self.host_step)
        if self.optimizer.state[self.params[0]]["step"] is not self._steps[0]:
            # the state tensors were replaced (another plan re-made the shared
            # base after a load_state_dict): count on the live ones
            _refuse_device_steps(self.optimizer, self.params)
            self._step_base, self._steps = _shared_step_base(self.optimizer, self.params)
        s = int(self._steps[0].item())
        if s != self.host_step:
            if self.table_first <= s + 1 < self.table_first + self.TABLE:
                self.step_dev.fill_(s)
                self.host_step = s
            else:
                self._table_at(s)

    @torch.no_grad()
    def _replay(self, draw: bool, k: int = 1):
        self._sync_step()
        if self.host_step + k >= self.table_first + self.TABLE:
            self._table_at(self.host_step)
        g = self._graph(draw, k)
        with torch.cuda.device(self.dev):
            g.replay()
        self.host_step += k
        self._step_base.add_(float(k))   # every state["step"] is a view of it
        for p, gr in zip(self.params, self.grads):
            if p.grad is not gr:
                p.grad = gr
        self.model._packed_key = None  # parameters changed in place: re-pack for sampling
        increment_version(self.params)  # ... and say so to autograd, as train_step does

    @torch.no_grad()
    def step(self, x0=None, cond=None, *, t=None, noise=None, return_tensor: bool = False):
        """One optimizer step (the contract of train_step).  x0 / cond default to
        the plan's input buffers (fill them in place to skip the copies); t and
        noise are drawn in the graph unless both are given."""
        for src, dst, nm in ((x0, self.x0, "x0"), (cond, self.cond, "condition")):
            if src is not None and src.data_ptr() != dst.data_ptr():
                if src.shape != dst.shape:
                    raise RuntimeError(f"ertdiff: this plan was captured for {nm} {tuple(dst.shape)}")
                dst.copy_(src)
        if (t is None) != (noise is None):
            raise RuntimeError("ertdiff: TrainPlan.step takes both t and noise, or neither")
        draw = t is None
        if not draw:
            if tuple(t.shape) != (self.B,) or tuple(noise.shape) != tuple(self.noise.shape):
                raise RuntimeError(f"ertdiff: TrainPlan.step takes t of shape ({self.B},) and noise of "
                                   f"shape {tuple(self.noise.shape)}")
            tl = t.to(torch.int64)
            if tl.numel() and (int(tl.min()) < 0 or int(tl.max()) >= self.alpha_bar.numel()):
                raise IndexError(f"ertdiff: t out of range [0, {self.alpha_bar.numel()})")
            self.t.copy_(tl)
            self.noise.copy_(noise)
        self._replay(draw)
        return self.loss.clone() if return_tensor else self.loss.item()

    RUN_STEPS = (32, 8)   # steps per graph replay in run(), each launched by ONE C call
                          # (ertd_train_steps_dev): the ~8 us gap at every call boundary
                          # of a graph (rocprofv3 trace, B = 32) is paid once per replay

    @torch.no_grad()
    def run(self, n: int):
        """n steps on the plan's inputs with fresh draws; no per-step host sync
        (the loss of the last step stays in plan.loss).  Replays a 32-step graph
        n // 32 times, an 8-step graph for the rest // 8, and the 1-step graph
        for what remains."""
        n = int(n)
        for k in self.RUN_STEPS:
            for _ in range(n // k):
                self._replay(True, k)
            n %= k
        for _ in range(n):
            self._replay(True)

    @torch.no_grad()
    def run_epoch(self, data, order, *, t=None, noise=None, drop_last: bool = False):
        """One epoch (:308-320) over a device-resident dataset, as one graph
        replay: batch i trains on data rows order[i*B : (i+1)*B], the last batch
        with whatever is left (drop_last=True leaves it out, as DataLoader does).
        Returns the per-batch losses as a device tensor (n_batches,); no host
        sync (epoch_loss() turns them into the reference's epoch figure).

        ``order``: any integer tensor of row indices into ``data`` -- not
        necessarily a permutation, so a train split is ``train_idx[perm]``.  It
        is range-checked before anything is launched (on the host for a CPU
        tensor; one aminmax for a device tensor).  Every batch is bit for bit
        the plan.step() on the gathered batch: same kernels, same draws (keyed
        by seed, batch position and Adam step), same Adam bookkeeping.

        t (n_rows,) / noise (n_rows, P), given together, replace the draws.
        After the call the epoch's draws are in plan.epoch_t / plan.epoch_noise
        (views of the graph's buffers: clone to keep them).  rng="torch" plans
        draw the whole epoch's t, then its noise, from torch's generator before
        the replay (not interleaved per batch as eager steps would).

        One graph per (dataset, n_rows, draws or not) is captured on first use;
        later epochs of the same length copy the new order in and replay."""
        P = self.model.param_dim
        _check_data(data, self.dev, self.L, P)
        order, n = _epoch_order(order, len(data), self.B, drop_last)
        nb = -(-n // self.B)
        if nb >= self.TABLE:
            raise RuntimeError(f"ertdiff: an epoch of {nb} batches does not fit the plan's table of "
                               f"{self.TABLE} Adam steps")
        draw = _check_draws(t, noise, n, P, self.alpha_bar.numel(), "TrainPlan.run_epoch")
        bufs = self._ebufs.get(n)
        if bufs is None:
            bufs = self._ebufs[n] = _EpochBufs(n, self.B, P, self.dev)
        self._sync_step()
        if self.host_step + nb >= self.table_first + self.TABLE:
            self._table_at(self.host_step)
        dev_draw = draw and self.rng == "philox"
        if draw and not dev_draw:
            bufs.t.random_(0, self.T)
            bufs.noise.normal_()
        elif not draw:
            bufs.t.copy_(t)
            bufs.noise.copy_(noise)
        bufs.rows.copy_(order)
        key = ("epoch", n, dev_draw, data.x0.data_ptr(), data.cond.data_ptr(), len(data))
        ent = self._graphs.get(key)
        if ent is None:
            w = self.model.weights_struct()
            with torch.cuda.device(self.dev):
                torch.cuda.synchronize(self.dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    _lib.check(_lib.lib().ertd_train_epoch_dev(
                        ctypes.byref(w), data.x0.data_ptr(), data.cond.data_ptr(), len(data),
                        bufs.rows.data_ptr(), n, bufs.t.data_ptr(), bufs.noise.data_ptr(),
                        self.alpha_bar.data_ptr(), self.B, self.L, self.freq.data_ptr(),
                        _lib.ptr_array(self.grads), _lib.ptr_array(self.exp_avg),
                        _lib.ptr_array(self.exp_avg_sq), self.step_dev.data_ptr(),
                        self.table.data_ptr(), self.table_first, self.TABLE, 1 if dev_draw else 0,
                        self.T, self.seed, bufs.losses.data_ptr(), self.ws.data_ptr(),
                        self.ws.numel(), _lib.stream_of(self.dev)), "train_epoch_dev")
            ent = self._graphs[key] = (g, data)   # the graph addresses the dataset: keep it
        with torch.cuda.device(self.dev):
            ent[0].replay()
        self.host_step += nb
        self._step_base.add_(float(nb))
        for p, gr in zip(self.params, self.grads):
            if p.grad is not gr:
                p.grad = gr
        self.model._packed_key = None
        increment_version(self.params)
        self.epoch_t, self.epoch_noise = bufs.t, bufs.noise
        return bufs.losses.clone()


@torch.no_grad()
def validation_loss(model, x0, cond, T, alpha_bar, *, t=None, noise=None) -> float:
    """Validation pass body (:327-336): forward on q_sample'd inputs, MSE."""
    from .model import q_sample
    B = x0.size(0)
    dev = x0.device
    if t is None:
        t = torch.randint(0, T, (B,), device=dev).long()
    if noise is None:
        noise = torch.randn_like(x0)
    x_noisy = q_sample(x0, t, noise, alpha_bar)
    pred = model(x_noisy, t, cond)
    return F.mse_loss(pred, noise).item()


_MASK64 = (1 << 64) - 1


def _validation_seed(seed: int) -> int:
    """The Philox key of the validation draws: one splitmix64 round of ``seed``,
    never equal to ``seed`` itself (the key of a TrainPlan on the same seed)."""
    z = (int(seed) + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    z ^= z >> 31
    return z if z != (int(seed) & _MASK64) else z ^ 1


class ValidationPlan:
    """The validation pass (:325-338) over rows of a DeviceDataset as one graph
    replay: per batch the train forward (the batch read through the row index),
    eps and the batch's MSELoss; no backward -- parameters, gradients and Adam
    state are not written.

        val = ValidationPlan(model, B, L, T, alpha_bar, seed=seed)
        losses = val.run(data, val_idx)            # device (n_batches,), no host sync
        val.eps, val.t, val.noise                  # the call's predictions and draws

    t ~ U{0..T-1} and noise ~ N(0, 1) are drawn in the head kernel, Philox keyed
    (validation seed, batch position, counter); the plan holds the counter and
    advances it by n_batches per call, so no two batches of any two calls share
    a key, and the validation seed is derived from ``seed`` so that a TrainPlan
    on the same ``seed`` draws a different stream.  The graph addresses the
    parameters: keep them (in-place updates are followed)."""

    def __init__(self, model, B: int, L: int, T: int, alpha_bar, seed=None):
        model._check_supported()
        self.model, self.T = model, int(T)
        self.params = model._params()
        dev = _lib.require_device(alpha_bar, self.params[0])
        self.dev, self.B, self.L = dev, int(B), int(L)
        if self.B < 1 or self.L < 1:
            raise RuntimeError("ertdiff: ValidationPlan needs B >= 1 and L >= 1")
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        self.val_seed = _validation_seed(self.seed)
        self.alpha_bar = _lib.f32c(alpha_bar, "alpha_bar")
        if self.alpha_bar.dim() != 1 or self.alpha_bar.numel() < self.T:
            raise IndexError(f"ertdiff: alpha_bar has {self.alpha_bar.numel()} entries, "
                             f"ValidationPlan needs at least T = {self.T}")
        P = model.param_dim
        self.ws = torch.empty(max(_lib.lib().ertd_workspace_bytes(self.B, self.L, P, 0, _lib.OP_TRAIN),
                                  256), dtype=torch.uint8, device=dev)
        self.freq = timestep_frequencies(_lib.HIDDEN, dev)
        self.ctr = 0           # batches drawn so far (the Philox counter of the next batch)
        self._bufs, self._graphs = {}, {}
        self.eps = self.t = self.noise = None

    def _call(self, data, bufs, n: int, draw: bool):
        w = self.model.weights_struct()
        _lib.check(_lib.lib().ertd_validation_epoch_dev(
            ctypes.byref(w), data.x0.data_ptr(), data.cond.data_ptr(), len(data),
            bufs.rows.data_ptr(), n, bufs.t.data_ptr(), bufs.noise.data_ptr(),
            self.alpha_bar.data_ptr(), self.B, self.L, self.freq.data_ptr(), bufs.ctr.data_ptr(),
            1 if draw else 0, self.T, self.val_seed, bufs.eps.data_ptr(), bufs.losses.data_ptr(),
            self.ws.data_ptr(), self.ws.numel(), _lib.stream_of(self.dev)), "validation_epoch_dev")

    @torch.no_grad()
    def run(self, data, rows, *, t=None, noise=None):
        """Per-batch validation losses (device, (n_batches,)) over data rows
        ``rows`` in the given order, the last batch partial; checks as
        TrainPlan.run_epoch.  t (n_rows,) / noise (n_rows, P) replace the draws."""
        P = self.model.param_dim
        _check_data(data, self.dev, self.L, P)
        rows, n = _epoch_order(rows, len(data), self.B, False)
        nb = -(-n // self.B)
        draw = _check_draws(t, noise, n, P, self.alpha_bar.numel(), "ValidationPlan.run")
        bufs = self._bufs.get(n)
        if bufs is None:
            bufs = self._bufs[n] = _EpochBufs(n, self.B, P, self.dev, with_eps=True)
        if not draw:
            bufs.t.copy_(t)
            bufs.noise.copy_(noise)
        bufs.rows.copy_(rows)
        c0 = self.ctr % (1 << 30)   # int32 on the device
        bufs.ctr.copy_(torch.arange(c0, c0 + nb, dtype=torch.int32, device=self.dev))
        key = (n, draw, data.x0.data_ptr(), data.cond.data_ptr(), len(data))
        ent = self._graphs.get(key)
        if ent is None:
            with torch.cuda.device(self.dev):
                self._call(data, bufs, n, draw)   # once outside any capture: module load
                torch.cuda.synchronize(self.dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._call(data, bufs, n, draw)
            ent = self._graphs[key] = (g, data)
        with torch.cuda.device(self.dev):
            ent[0].replay()
        self.ctr += nb
        self.eps, self.t, self.noise = bufs.eps, bufs.t, bufs.noise
        return bufs.losses.clone()


def _weighted_mean(vals, n_rows: int, B: int) -> float:
    sizes = batch_sizes(n_rows, B)
    if len(vals) != len(sizes):
        raise RuntimeError(f"ertdiff: {len(vals)} losses for {len(sizes)} batches of {n_rows} rows")
    total = 0.0
    for v, b in zip(vals, sizes):
        total += v * b      # running_loss += loss.item() * B (:320)
    return total / n_rows   # / len(dataset) (:322)


def epoch_loss(losses, n_rows: int, B: int) -> float:
    """The reference's epoch figure (:320-322, :336-338) from per-batch losses:
    sum_i loss_i * B_i / n_rows in Python floats; one device-to-host copy."""
    return _weighted_mean(losses.tolist(), n_rows, B)


def fit(model, optimizer, data, train_idx, val_idx, T, alpha_bar, *, num_epochs: int,
        batch_size: int = 32, checkpoint_path=None, generator=None, seed=None):
    """The reference's training loop (:305-356) on a DeviceDataset: per epoch a
    shuffled TrainPlan.run_epoch over train_idx, a ValidationPlan.run over
    val_idx (unshuffled), one host read of both loss vectors, and on a better
    validation loss the reference's checkpoint dict (save_checkpoint, epoch + 1)
    at checkpoint_path.  Returns {"train_history", "val_history",
    "best_val_loss", "best_epoch"} (best_epoch 1-based as in the checkpoint, 0
    if no epoch ran).

    The shuffle is train_idx[torch.randperm(n, generator=generator)] and t /
    noise are the plans' Philox draws from ``seed``: this reproduces neither
    DataLoader's sampler seeding nor the reference's mt19937 torch.randint /
    torch.randn_like draws, so loss curves match the reference statistically,
    not number for number."""
    from .data import save_checkpoint
    train_idx = torch.as_tensor(train_idx)
    val_idx = torch.as_tensor(val_idx)
    L = data.cond.shape[2]
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    plan = TrainPlan(model, optimizer, batch_size, L, T, alpha_bar, seed=seed)
    val = ValidationPlan(model, batch_size, L, T, alpha_bar, seed=seed)
    n_tr, n_va = train_idx.numel(), val_idx.numel()
    train_history, val_history = [], []
    best_val_loss, best_epoch = float("inf"), 0
    gdev = generator.device if generator is not None else "cpu"
    for epoch in range(int(num_epochs)):
        perm = torch.randperm(n_tr, generator=generator, device=gdev)
        tl = plan.run_epoch(data, train_idx[perm.to(train_idx.device)])
        vl = val.run(data, val_idx)
        both = torch.cat([tl, vl]).tolist()
        train_history.append(_weighted_mean(both[:tl.numel()], n_tr, batch_size))
        val_history.append(_weighted_mean(both[tl.numel():], n_va, batch_size))
        if val_history[-1] < best_val_loss:
            best_val_loss, best_epoch = val_history[-1], epoch + 1
            if checkpoint_path is not None:
                save_checkpoint(checkpoint_path, model, optimizer, epoch + 1, best_val_loss,
                                train_history, val_history, model.param_dim)
    return {"train_history": train_history, "val_history": val_history,
            "best_val_loss": best_val_loss, "best_epoch": best_epoch}
