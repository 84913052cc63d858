"""Every C entry that takes a workspace, on the memory a long-running process
hands it: twice with identical inputs --

  clean   inputs as they are, a zero-filled generously sized workspace, zeroed
          outputs (what today's tests and a fresh process's torch.empty give);
  dirty   every input inside NaN bands, every output inside pattern bands and
          prefilled with 0xFF, the workspace 0xFF-filled, fenced, and EXACTLY
          the size its *_ws_bytes / *_workspace_bytes query returned

(tests/dirty_state.py) -- and asserts (a) rc == 0, (b) the dirty outputs are
bitwise the clean ones and finite, (c) every fence is intact, (d) the clean
result is within the neighbouring test's tolerance of its float64 reference.
A skipped zeroing, a pad lane multiplied by a zero weight, a partial buffer
read before it is written, a write past `out` or past ws + ws_bytes, a query
smaller than the launch's scratch: each fails one of these.

Every entry here is deterministic (the suite asserts bitwise reruns), so (b)
holds with no tolerance and no entry needed the reference comparison instead.
Not fenced: the model parameters and packed weights of the reference-model and
U-Net entries (nn.Parameter storage, packed by the library's own pack entry)
and the Adam moments of the train entries; everything else a call is handed is.

Read before the first poisoned run (the words a kernel waits or branches on):
chain.hip's ring / claim / progress / vready / status words are one block
zeroed by launch_zero_words on the stream before the chain (capi.hip,
enqueue_sample; its spins are bounded and report through the status word);
train.hip's fin_cnt arrival counters are zeroed by the step's first kernel
(enc_train_kernel, item 0) and re-armed by the last arriver -- no wait; the
U-Net walk has no device-side wait at all, and its step-counter slot is set by
the sampler's head before any step reads it.  Draws (draw = 1) are formed in registers and
stored: t is never read back from the caller's buffer."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dirty_state as DS
import ertdiff
import solver_ref as SR
from ertdiff import _lib
from ertdiff.schedule import timestep_frequencies
from oracle import ref_numpy as RN
from oracle import ref_torch as RT
from oracle import unet_torch as U
from synth import synth_normal, synth_timesteps, synth_uniform

pytestmark = pytest.mark.gpu

FP32, BF16, BF16X3 = _lib.PREC_FP32, _lib.PREC_BF16, _lib.PREC_BF16X3
PREC = {"fp32": FP32, "bf16": BF16, "bf16x3": BF16X3}
MODES = {"same": 0, "down": 1, "up": 2}
ACTS = {"none": 0, "gn_silu": 1, "gn": 2}
DIRECT, UP, WINO, WINO4 = 0, 1, 2, 3          # ERTD_PACK_*
CONV_TOL = {"fp32": 1e-5, "bf16": 1e-4, "bf16x3": 3e-5}   # test_gpu_unet_ops.py


class Out:
    """An output that the call writes whole: shape and dtype."""

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.dtype = tuple(shape), dtype


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _rel(a, b):
    return RN.rel_l2(a.detach().double().cpu().numpy(), np.asarray(b, dtype=np.float64))


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _batch(B, dev):
    return {"cus/8": _cus(dev) // 8, "cus/4": _cus(dev) // 4}.get(B, B)


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def run_pair(dev, call, inputs, outputs, ws_bytes, finite=True):
    """call(inp, out, ws_ptr, ws_bytes, dirty) -> rc, once clean and once dirty.
    inputs: name -> CPU tensor | None.  outputs: name -> Out (written whole) or
    a CPU tensor (in/out state, copied in).  The call may add further tensors
    to `out` (state it updates in place): they are compared too.  Returns the
    clean outputs and the dirty run's (inp, out, ws) for a follow-up call."""
    runs = {}
    for kind in ("clean", "dirty"):
        dirty = kind == "dirty"
        inp, out = {}, {}
        for k, v in inputs.items():
            inp[k] = None if v is None else (DS.fenced(v, device=dev, name=k) if dirty else v.to(dev))
        for k, v in outputs.items():
            if isinstance(v, Out):
                out[k] = (DS.fenced_empty(v.shape, v.dtype, dev, name=k) if dirty
                          else torch.zeros(v.shape, dtype=v.dtype, device=dev))
            else:
                out[k] = DS.fenced(v, fill="pattern", device=dev, name=k) if dirty else v.to(dev).clone()
        if dirty:
            ws, n = DS.poisoned_ws(ws_bytes, dev), ws_bytes
        else:
            ws = torch.zeros(ws_bytes + 65536, dtype=torch.uint8, device=dev)
            n = ws.numel()
        rc = call(inp, out, _p(ws), n, dirty)
        torch.cuda.synchronize(dev)
        assert rc == 0, f"{kind} call returned {rc}"
        runs[kind] = (inp, out, ws)
    inp, out, ws = runs["dirty"]
    DS.check_fences(*[t for t in list(inp.values()) + list(out.values()) + [ws]
                      if t is not None and hasattr(t, "_fence")])
    for k, v in out.items():
        DS.assert_same_bits(v, runs["clean"][1][k], k, finite=finite)
    return runs["clean"][1], runs["dirty"]


# ---- ertd_conv2d / ertd_conv2d_gn ---------------------------------------------------------------
def _ref_conv(x, w, b, mode, act, gn, bf16):
    """test_gpu_unet_ops.py's reference: torch on the CPU, identical inputs."""
    if act != "none":
        x = x * gn[..., 0][:, :, None, None] + gn[..., 1][:, :, None, None]
        if act == "gn_silu":
            x = F.silu(x)
    if bf16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    ks = w.shape[-1]
    if mode == "up":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w, b, stride=2 if mode == "down" else 1, padding=ks // 2)


def _conv_inputs(Ca, Cb, Cout, H, ks, mode, act, B, seed, epilogue=True):
    Cin = Ca + Cb
    Ho = H // 2 if mode == "down" else (2 * H if mode == "up" else H)
    t = {"x": _rand((B, Ca, H, H), seed), "x2": _rand((B, Cb, H, H), seed + 1) if Cb else None,
         "w": _rand((Cout, Cin, ks, ks), seed + 2, 1.0 / np.sqrt(Cin * ks * ks)),
         "bias": _rand((Cout,), seed + 3, 0.1), "gn": None, "ebias": None, "res": None}
    if act != "none":
        t["gn"] = torch.stack([_rand((B, Cin), seed + 4, 0.3) + 1.0, _rand((B, Cin), seed + 5, 0.2)], -1)
    if epilogue:
        t["ebias"], t["res"] = _rand((B, Cout), seed + 6), _rand((B, Cout, Ho, Ho), seed + 7)
    return t, Ho


def _conv_ref(t, mode, act, bf16=False):
    xin = t["x"] if t["x2"] is None else torch.cat([t["x"], t["x2"]], 1)
    ref = _ref_conv(xin, t["w"], t["bias"], mode, act, t["gn"], bf16)
    if t["ebias"] is not None:
        ref = ref + t["ebias"][:, :, None, None]
    if t["res"] is not None:
        ref = ref + t["res"]
    return ref


def _conv_call(Ca, Cb, Cout, H, ks, mode, act, B, prec, gn_np=0, run=False):
    lib = _lib.lib()

    def call(i, o, ws, n, dirty):
        s = _lib.stream_of(o["out"].device)
        eb = i["ebias"]
        head = (i["x"].data_ptr(), Ca, _p(i["x2"]), Cb, B, H)
        tail = (_p(i["bias"]), Cout, ks, MODES[mode], _p(i["gn"]), ACTS[act], _p(eb),
                0 if eb is None else eb.shape[1], _p(i["res"]), o["out"].data_ptr(), prec, ws, n)
        if run:
            return lib.ertd_conv2d_run(*head, *tail, s)
        if gn_np:
            return lib.ertd_conv2d_gn(*head, i["w"].data_ptr(), *tail, o["gn_parts"].data_ptr(), gn_np, s)
        return lib.ertd_conv2d(*head, i["w"].data_ptr(), *tail, s)
    return call


def _route(Ca, Cb, Cout, H, ks, mode, act, B):
    """(pack kind, GroupNorm partials of the output) as make_dispatch_golden.py queries them."""
    lib = _lib.lib()
    dummy = ctypes.create_string_buffer(64)
    d = _lib.PackDesc()
    a = ctypes.addressof(dummy)
    assert lib.ertd_conv2d_pack_desc(Ca + Cb, Ca, Cout, ks, MODES[mode], FP32, B, H, a, a, ctypes.byref(d)) == 0
    return d.kind, lib.ertd_conv2d_gn_parts(Ca, Cb, Cout, ks, MODES[mode], ACTS[act], FP32, B, H)


# (Ca, Cb, Cout, H, ks, mode, act, B, pack kind, K split (Winograd kinds) | None).  Shapes for 256 CUs;
# the route family is asserted, so a case cannot silently move to another kernel.
CONV_FP32 = [
    (64, 0, 64, 16, 3, "same", "gn_silu", 2, WINO, True),           # F(2x2) with K split
    (16, 8, 64, 16, 3, "same", "gn_silu", 2, WINO, False),          # F(2x2) unsplit on a concat
    (12, 0, 64, 32, 3, "same", "gn_silu", 2, WINO4, False),         # LDS-weight F(4x4)
    (16, 0, 64, 128, 3, "same", "none", 1, WINO4, True),            # LDS-weight F(4x4), K split at 128x128
    (64, 0, 64, 32, 3, "same", "gn_silu", 2, WINO4, False),         # register-weight F(4x4)
    (32, 0, 256, 16, 3, "same", "gn", "cus/8", WINO4, True),        # register-weight F(4x4), K split
    (16, 0, 256, 16, 3, "same", "none", "cus/4", WINO4, False),     # register-weight F(4x4), unsplit at 16x16
    (64, 0, 64, 16, 3, "up", "none", 2, WINO4, False),              # its Upsample route
    (20, 0, 40, 16, 3, "same", "gn_silu", 2, DIRECT, None),         # direct 3x3, ragged channel tiles
    (60, 4, 64, 16, 3, "same", "gn_silu", 2, DIRECT, None),
    (20, 12, 40, 16, 3, "up", "none", 2, UP, None),                 # sub-pixel direct
    (64, 0, 64, 32, 3, "down", "none", 2, DIRECT, None),            # stride 2
    (32, 24, 1, 16, 3, "same", "gn_silu", 3, DIRECT, None),         # Cout = 1
    (1, 0, 64, 16, 3, "same", "none", 2, DIRECT, None),             # Cin = 1
    (96, 32, 128, 32, 1, "same", "none", 3, DIRECT, None),          # 1x1 skip-GEMM
    (128, 64, 64, 64, 1, "same", "none", 2, DIRECT, None),          # 1x1 LDS kernel
    (48, 0, 40, 16, 1, "same", "none", 2, DIRECT, None),            # 1x1 implicit GEMM, ragged
]


@pytest.mark.parametrize("Ca,Cb,Cout,H,ks,mode,act,B,kind,split", CONV_FP32)
def test_conv2d_fp32(Ca, Cb, Cout, H, ks, mode, act, B, kind, split, cuda_dev):
    """ertd_conv2d (ertd_conv2d_gn where the Winograd route emits GroupNorm
    partials) with bias, ebias and res present."""
    B = _batch(B, cuda_dev)
    got_kind, np_ = _route(Ca, Cb, Cout, H, ks, mode, act, B)
    assert got_kind == kind, f"pack kind {got_kind}, expected {kind}"
    if split is not None:                       # a K split emits no partials
        assert (np_ == 0) == split, f"gn_parts {np_} with K split expected {split}"
    np_ = np_ if kind in (WINO, WINO4) else 0   # the partials of the routed Winograd kernels
    t, Ho = _conv_inputs(Ca, Cb, Cout, H, ks, mode, act, B, 100 + Ca + Cout + H)
    outs = {"out": Out(B, Cout, Ho, Ho)}
    if np_:
        outs["gn_parts"] = Out(B, Cout, np_, 2)
    q = _lib.lib().ertd_conv2d_workspace_bytes(Ca + Cb, Cout, ks, FP32, B, H, MODES[mode])
    clean, _ = run_pair(cuda_dev, _conv_call(Ca, Cb, Cout, H, ks, mode, act, B, FP32, np_), t, outs, q)
    err = _rel(clean["out"], _conv_ref(t, mode, act).double().numpy())
    assert err < CONV_TOL["fp32"], err
    if np_:      # {sum, M2} of np equal parts of each (sample, channel) image: combined
        # (Chan et al.) they are the image's sum and M2, whatever pixels a part holds
        y = clean["out"].double().cpu().reshape(B, Cout, -1)
        p = clean["gn_parts"].double().cpu()
        n = y.shape[-1] / np_
        tot = p[..., 0].sum(-1)
        m2 = p[..., 1].sum(-1) + (n * (p[..., 0] / n - (tot / y.shape[-1])[..., None]) ** 2).sum(-1)
        assert _rel(tot, y.sum(-1).numpy()) < 1e-5
        assert _rel(m2, ((y - y.mean(-1, keepdim=True)) ** 2).sum(-1).numpy()) < 1e-5


CONV_BF = [(20, 0, 64, 16, 3, "same", "gn_silu"), (32, 24, 64, 16, 3, "same", "gn_silu"),   # ragged 16-ch group
           (20, 0, 40, 16, 3, "up", "none"), (64, 0, 64, 32, 3, "down", "none"), (96, 32, 64, 16, 1, "same", "none")]


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("Ca,Cb,Cout,H,ks,mode,act", CONV_BF)
def test_conv2d_bf16(Ca, Cb, Cout, H, ks, mode, act, precision, cuda_dev):
    """The bf16 image's pad lanes (Cin % 16 != 0) sit in the workspace: they are
    multiplied by zero weights, and 0 x NaN is NaN."""
    B = 2
    t, Ho = _conv_inputs(Ca, Cb, Cout, H, ks, mode, act, B, 200 + Ca + Cout + H, epilogue=False)
    q = _lib.lib().ertd_conv2d_workspace_bytes(Ca + Cb, Cout, ks, PREC[precision], B, H, MODES[mode])
    clean, _ = run_pair(cuda_dev, _conv_call(Ca, Cb, Cout, H, ks, mode, act, B, PREC[precision]), t,
                        {"out": Out(B, Cout, Ho, Ho)}, q)
    err = _rel(clean["out"], _conv_ref(t, mode, act, precision == "bf16").double().numpy())
    assert err < CONV_TOL[precision], err


@pytest.mark.parametrize("Ca,Cout,H,act,precision", [(64, 64, 16, "gn_silu", "fp32"), (20, 64, 16, "gn_silu", "bf16")])
def test_conv2d_run_after_conv2d(Ca, Cout, H, act, precision, cuda_dev):
    """ertd_conv2d_run on the workspace ertd_conv2d left (the packing at its head
    is the documented carried state: not re-poisoned; the K-split buffer / bf16
    image behind it now hold the first call's leftovers)."""
    B = 2
    t, Ho = _conv_inputs(Ca, 0, Cout, H, 3, "same", act, B, 300 + Ca, epilogue=precision == "fp32")
    q = _lib.lib().ertd_conv2d_workspace_bytes(Ca, Cout, 3, PREC[precision], B, H, 0)
    _, (inp, out, ws) = run_pair(cuda_dev, _conv_call(Ca, 0, Cout, H, 3, "same", act, B, PREC[precision]), t,
                                 {"out": Out(B, Cout, Ho, Ho)}, q)
    out2 = {"out": DS.fenced_empty((B, Cout, Ho, Ho), device=cuda_dev, name="out (run)")}
    rc = _conv_call(Ca, 0, Cout, H, 3, "same", act, B, PREC[precision], run=True)(inp, out2, ws.data_ptr(), q, True)
    torch.cuda.synchronize(cuda_dev)
    assert rc == 0
    DS.check_fences(out2["out"], ws, *[v for v in inp.values() if v is not None])
    DS.assert_same_bits(out2["out"], out["out"], "out (run)")


def test_conv2d_query_suffices_for_every_split(cuda_dev):
    """ertd_conv2d_workspace_bytes sizes with Ca = Cin; the call decides its
    route (and its K-split buffer) from the real Ca.  Every split of Cin, every
    activation: rc 0 on exactly the queried bytes, fences kept, torch <= 1e-5."""
    lib = _lib.lib()
    Cout, H = 64, 16
    for Cin in (64, 72):
        for B in (2, _cus(cuda_dev) // 8):
            q = lib.ertd_conv2d_workspace_bytes(Cin, Cout, 3, FP32, B, H, 0)
            for Ca in (Cin, Cin - 4, Cin - 6, Cin - 8, Cin - 12):
                for act in ("none", "gn_silu", "gn"):
                    t, _ = _conv_inputs(Ca, Cin - Ca, Cout, H, 3, "same", act, B, 400 + Cin + Ca, epilogue=False)
                    inp = {k: None if v is None else DS.fenced(v, device=cuda_dev, name=k) for k, v in t.items()}
                    out = {"out": DS.fenced_empty((B, Cout, H, H), device=cuda_dev, name="out")}
                    ws = DS.poisoned_ws(q, cuda_dev)
                    rc = _conv_call(Ca, Cin - Ca, Cout, H, 3, "same", act, B, FP32)(inp, out, ws.data_ptr(), q, True)
                    torch.cuda.synchronize(cuda_dev)
                    assert rc == 0, (Cin, B, Ca, act, rc)
                    DS.check_fences(out["out"], ws, *[v for v in inp.values() if v is not None])
                    err = _rel(out["out"], _conv_ref(t, "same", act).double().numpy())
                    assert err < 1e-5, (Cin, B, Ca, act, err)


# ---- ertd_conv_input_grad / ertd_conv_wgrad / ertd_conv_wgrad_bias ---------------------------------
INPUT_GRAD = [(64, 64, 64, 3, 0, 2), (192, 64, 32, 3, 0, 2), (64, 1, 32, 3, 0, 2), (1, 32, 32, 3, 0, 2),
              (64, 64, 64, 3, 1, 2), (128, 128, 16, 3, 2, 2), (96, 64, 32, 1, 0, 2),   # test_conv_input_grad_vs_autograd's
              (256, 256, 16, 3, 0, "cus/8")]                                           # the K-split accumulate case


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("Cin,Cout,H,ks,mode,B", INPUT_GRAD)
def test_conv_input_grad(Cin, Cout, H, ks, mode, B, acc, cuda_dev):
    B = _batch(B, cuda_dev)
    g = torch.Generator().manual_seed(Cin + 3 * Cout + H + mode)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    Ho = H // 2 if mode == 1 else (2 * H if mode == 2 else H)
    dy = torch.randn(B, Cout, Ho, Ho, generator=g)
    prev = torch.randn(B, Cin, H, H, generator=g)
    if mode == 2:
        ref = torch.nn.grad.conv2d_input((B, Cin, 2 * H, 2 * H), w.double(), dy.double(), padding=1)
        ref = ref.view(B, Cin, H, 2, H, 2).sum((3, 5))
    else:
        ref = torch.nn.grad.conv2d_input((B, Cin, H, H), w.double(), dy.double(),
                                         stride=2 if mode == 1 else 1, padding=ks // 2)
    if acc:
        ref = ref + prev.double()
    lib = _lib.lib()

    def call(i, o, ws, n, dirty):
        return lib.ertd_conv_input_grad(i["dy"].data_ptr(), B, H, i["w"].data_ptr(), Cout, Cin, ks, mode,
                                        o["dx"].data_ptr(), acc, ws, n, _lib.stream_of(cuda_dev))
    q = lib.ertd_conv_input_grad_ws_bytes(Cin, Cout, B, H, ks, mode)
    clean, _ = run_pair(cuda_dev, call, {"dy": dy, "w": w}, {"dx": prev if acc else Out(B, Cin, H, H)}, q)
    err = _rel(clean["dx"], ref.numpy())
    assert err < 1e-5, err


WGRAD = [  # (Ca, Cb, Cout, H, ks, mode, act, B)
    (64, 0, 64, 16, 3, 0, 0, 3),       # 8-row bands
    (128, 64, 128, 32, 3, 0, 0, 2),    # Winograd wgrad, concat
    (1, 0, 64, 16, 3, 0, 0, 3),
    (32, 0, 1, 32, 3, 0, 0, 2),
    (64, 0, 64, 32, 3, 1, 0, 2),
    (128, 0, 128, 16, 3, 2, 0, 2),
    (96, 32, 64, 32, 1, 0, 0, 2),
    (48, 0, 40, 32, 1, 0, 0, 2),
    (96, 32, 64, 32, 3, 0, 1, 2),      # the fused-activation form
]


@pytest.mark.parametrize("Ca,Cb,Cout,H,ks,mode,act,B", WGRAD)
def test_conv_wgrad(Ca, Cb, Cout, H, ks, mode, act, B, cuda_dev):
    """ertd_conv_wgrad, accumulate 0 then 1 on the same (then used) workspace, and
    ertd_conv_wgrad_bias where ertd_conv_wgrad_bias_ok."""
    g = torch.Generator().manual_seed(Ca * 7 + Cout + H + mode + act)
    Cin = Ca + Cb
    x = torch.randn(B, Cin, H, H, generator=g)
    Ho = H // 2 if mode == 1 else (2 * H if mode == 2 else H)
    dy = torch.randn(B, Cout, Ho, Ho, generator=g)
    ss = None
    a = x.double()
    if act:
        ss = torch.stack([torch.rand(B, Cin, generator=g) + 0.5, torch.randn(B, Cin, generator=g)], -1).contiguous()
        a = F.silu(a * ss[..., 0, None, None].double() + ss[..., 1, None, None].double())
    if mode == 2:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    ref = torch.nn.grad.conv2d_weight(a, (Cout, Cin, ks, ks), dy.double(), stride=2 if mode == 1 else 1,
                                      padding=ks // 2)
    lib = _lib.lib()
    bias_ok = act == 0 and lib.ertd_conv_wgrad_bias_ok(Cin, Cout, B, H, ks, mode) == 1
    ins = {"dy": dy, "xa": x[:, :Ca].contiguous(), "xb": x[:, Ca:].contiguous() if Cb else None, "ss": ss}

    def call(i, o, ws, n, dirty):
        s = _lib.stream_of(cuda_dev)
        args = (i["dy"].data_ptr(), i["xa"].data_ptr(), Ca, _p(i["xb"]), Cb, B, H, Cout, ks, mode, _p(i["ss"]), act)
        for acc in (0, 1):
            rc = lib.ertd_conv_wgrad(*args, o["dw"].data_ptr(), acc, ws, n, s)
            if rc:
                return rc
        if bias_ok:
            return lib.ertd_conv_wgrad_bias(*args, o["dw_b"].data_ptr(), 0, o["db"].data_ptr(), o["db2"].data_ptr(),
                                            ws, n, s)
        return 0
    outs = {"dw": Out(Cout, Cin, ks, ks)}
    if bias_ok:
        outs.update(dw_b=Out(Cout, Cin, ks, ks), db=Out(Cout), db2=Out(Cout))
    q = lib.ertd_conv_wgrad_ws_bytes(Cin, Cout, B, H, ks, mode)
    assert q > 0
    clean, _ = run_pair(cuda_dev, call, ins, outs, q)
    err = _rel(clean["dw"], 2 * ref.numpy())           # written, then accumulated once more
    assert err < 1e-5, err
    if bias_ok:
        assert _rel(clean["dw_b"], ref.numpy()) < 1e-5
        assert _rel(clean["db"], dy.double().sum((0, 2, 3)).numpy()) < 1e-5
        assert torch.equal(clean["db"], clean["db2"])


def test_conv_wgrad_bias_fused_geometry(cuda_dev):
    """ertd_conv_wgrad_bias where it is fused (B * tiles a multiple of 256)."""
    Ca, Cb, Cout, H, B = 64, 0, 64, 32, 4
    lib = _lib.lib()
    assert lib.ertd_conv_wgrad_bias_ok(Ca, Cout, B, H, 3, 0) == 1
    g = torch.Generator().manual_seed(77)
    x, dy = torch.randn(B, Ca, H, H, generator=g), torch.randn(B, Cout, H, H, generator=g)

    def call(i, o, ws, n, dirty):
        return lib.ertd_conv_wgrad_bias(i["dy"].data_ptr(), i["x"].data_ptr(), Ca, None, 0, B, H, Cout, 3, 0, None, 0,
                                        o["dw"].data_ptr(), 0, o["db"].data_ptr(), o["db2"].data_ptr(), ws, n,
                                        _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, call, {"dy": dy, "x": x}, {"dw": Out(Cout, Ca, 3, 3), "db": Out(Cout), "db2": Out(Cout)},
                        lib.ertd_conv_wgrad_ws_bytes(Ca, Cout, B, H, 3, 0))
    ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, Ca, 3, 3), dy.double(), padding=1)
    assert _rel(clean["dw"], ref.numpy()) < 1e-5
    assert _rel(clean["db"], dy.double().sum((0, 2, 3)).numpy()) < 1e-5


# ---- small train operators ------------------------------------------------------------------------
@pytest.mark.parametrize("P", [37, 4096 + 37])
def test_wgrad_gemm(P, cuda_dev):
    M, N, B = 65, 70, 3
    lib = _lib.lib()
    g = torch.Generator().manual_seed(P)
    dY, X = torch.randn(B, M, P, generator=g), torch.randn(B, N, P, generator=g)

    def call(i, o, ws, n, dirty):
        for acc in (0, 1):
            rc = lib.ertd_wgrad_gemm(i["dY"].data_ptr(), i["X"].data_ptr(), M, N, P, B, M * P, N * P,
                                     o["dW"].data_ptr(), acc, ws, n, _lib.stream_of(cuda_dev))
            if rc:
                return rc
        return 0
    clean, _ = run_pair(cuda_dev, call, {"dY": dY, "X": X}, {"dW": Out(M, N)}, lib.ertd_wgrad_ws_bytes(M, N, P, B))
    ref = 2 * torch.einsum("bmp,bnp->mn", dY.double(), X.double())
    assert _rel(clean["dW"], ref.numpy()) < 1e-5


def test_mse_loss(cuda_dev):
    n = 65537
    lib = _lib.lib()
    g = torch.Generator().manual_seed(n)
    e, z = torch.randn(n, generator=g), torch.randn(n, generator=g)

    def call(i, o, ws, nb, dirty):
        return lib.ertd_mse_loss(i["eps"].data_ptr(), i["noise"].data_ptr(), n, o["loss"].data_ptr(),
                                 o["dout"].data_ptr(), ws, nb, _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, call, {"eps": e, "noise": z}, {"loss": Out(1), "dout": Out(n)},
                        lib.ertd_mse_loss_ws_bytes())
    ref = float(((e.double() - z.double()) ** 2).mean())
    assert abs(float(clean["loss"][0]) - ref) <= float(np.spacing(np.float32(ref)))     # <= 1 ulp (test_mse_loss)
    assert torch.equal(clean["dout"].cpu(), (e - z) * torch.tensor(2.0 / n, dtype=torch.float64).float())


@pytest.mark.parametrize("L", [5, 255, 256])
def test_encoder_train_fwd_bwd(L, golden_weights, cuda_dev):
    """fwd then bwd on one workspace (the saved activations are the carried
    state between the two)."""
    B = 3
    lib = _lib.lib()
    W = {k: torch.from_numpy(np.asarray(golden_weights[f"condition_encoder.{k}"]))
         for k in ("0.weight", "0.bias", "2.weight", "2.bias")}
    cond = torch.from_numpy(synth_uniform((B, 14, L), 2000 + L))
    Wr = {k: v.double().requires_grad_(True) for k, v in W.items()}
    a1 = F.relu(F.conv1d(cond.double(), Wr["0.weight"], Wr["0.bias"], stride=2, padding=1))
    a2 = F.relu(F.conv1d(a1, Wr["2.weight"], Wr["2.bias"], stride=2, padding=1))
    gvec = torch.randn(B, 64, generator=torch.Generator().manual_seed(L))
    (a2.mean(2) * gvec.double()).sum().backward()
    gm = (gvec.double() / a2.shape[2]).float()
    packed = torch.zeros(lib.ertd_packed_floats(), device=cuda_dev)
    w0, w2 = W["0.weight"].to(cuda_dev), W["2.weight"].to(cuda_dev)
    assert lib.ertd_encoder_train_pack(w0.data_ptr(), w2.data_ptr(), packed.data_ptr(), _lib.stream_of(cuda_dev)) == 0

    def call(i, o, ws, n, dirty):
        s = _lib.stream_of(cuda_dev)
        rc = lib.ertd_encoder_train_fwd(packed.data_ptr(), i["b1"].data_ptr(), i["b2"].data_ptr(),
                                        i["cond"].data_ptr(), B, L, o["m"].data_ptr(), ws, n, s)
        return rc or lib.ertd_encoder_train_bwd(packed.data_ptr(), i["cond"].data_ptr(), i["g"].data_ptr(), B, L,
                                                o["0.weight"].data_ptr(), o["0.bias"].data_ptr(),
                                                o["2.weight"].data_ptr(), o["2.bias"].data_ptr(), ws, n, s)
    outs = {"m": Out(B, 64)}
    outs.update({k: Out(*v.shape) for k, v in W.items()})
    clean, _ = run_pair(cuda_dev, call, {"b1": W["0.bias"], "b2": W["2.bias"], "cond": cond, "g": gm}, outs,
                        lib.ertd_encoder_train_ws_bytes(B, L))
    assert _rel(clean["m"], a2.mean(2).detach().numpy()) < 2e-6
    for k in W:
        gr = Wr[k].grad.numpy()
        if np.linalg.norm(gr) == 0:
            assert float(clean[k].abs().max()) == 0.0, k
        else:
            assert _rel(clean[k], gr) < 1e-4, k


# ---- the U-Net walk -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unet_case(name, B, L):
    cfg = U.CONFIGS[name]
    x = torch.from_numpy(synth_normal((B, cfg.param_dim), 111))
    cond = torch.from_numpy(synth_uniform((B, 14, L), 112))
    t = torch.tensor([999, 5, 17][:B])
    W = U.init_weights(cfg, 13, affine="random")
    with torch.no_grad():
        ref32 = U.forward(x, t, cond, W, cfg).double().numpy()
        ref16 = U.forward(x, t, cond, W, cfg, bf16=True).double().numpy()
    return cfg, x, cond, t, W, ref32, ref16


def _unet(name, W, dev, precision):
    m = ertdiff.ConditionalUNet.from_config(name, seed=0, precision=precision)
    m.load_state_dict(W)
    return m.to(dev).eval()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("name,B,L", [("U1", 3, 129), ("U3", 2, 257)])
def test_unet_forward(name, B, L, precision, cuda_dev):
    cfg, x, cond, t, W, ref32, ref16 = _unet_case(name, B, L)
    m = _unet(name, W, cuda_dev, precision)
    packed = m.packed_weights(cuda_dev)
    lib = _lib.lib()

    def call(i, o, ws, n, dirty):
        return lib.ertd_unet_forward(ctypes.byref(m.cfg), packed.data_ptr(), i["x"].data_ptr(), i["t"].data_ptr(),
                                     i["cond"].data_ptr(), 14 * L, L, B, o["out"].data_ptr(), o["cemb"].data_ptr(),
                                     ws, n, _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, call, {"x": x, "t": t, "cond": cond},
                        {"out": Out(B, cfg.param_dim), "cemb": Out(B, 128)},
                        lib.ertd_unet_workspace_bytes(ctypes.byref(m.cfg), B, L))
    got = clean["out"].cpu().double().numpy()
    if precision == "bf16":       # test_unet_bf16_forward's budgets
        assert RN.rel_l2(got, ref16) < 1.2e-2 and RN.rel_l2(got, ref32) < 1.6e-2
    else:                         # test_unet_forward_vs_oracle / test_unet_bf16x3_forward
        assert RN.rel_l2(got, ref32) < (1e-5 if precision == "fp32" else 1e-4)
    assert _rel(clean["cemb"], U.condition_embedding(cond, W).double().numpy()) < 1e-5


@pytest.mark.parametrize("plan", [False, True])
@pytest.mark.parametrize("kind", ["ddpm", "solver"])
def test_unet_sample(kind, plan, cuda_dev):
    """ertd_unet_sample / ertd_unet_sample_solver, 3 steps, U1, B = 2, eagerly
    and as a plan (poisoned before plan creation only: the plan's workspace
    between its launches is carried state)."""
    from ertdiff import solver as S
    from ertdiff.unet import _UPrepared
    name, B, L, T = "U1", 2, 129, 3
    cfg = U.CONFIGS[name]
    W = U.init_weights(cfg, 3)
    m = _unet(name, W, cuda_dev, "fp32")
    P = cfg.param_dim
    cond = torch.from_numpy(synth_uniform((B, 14, L), 103))
    noise = torch.from_numpy(synth_normal((T, B, P), 104))
    lib = _lib.lib()
    sched = ertdiff.get_diffusion_schedule(T, device=cuda_dev)
    ab50 = ertdiff.get_diffusion_schedule(50)[2]
    keep = []

    def call(i, o, ws, n, dirty):
        s = _lib.stream_of(cuda_dev)
        handle = ctypes.c_void_p()
        if kind == "ddpm":
            prep = _UPrepared(m, i["cond"], T, *sched, None, 1.0, False)
            keep.append(prep)
            args = prep.args(B, o["x"], i["noise"], 0, 0, T - 1, T, torch.empty(0))[:-2] + (ws, n)
            if not plan:
                return lib.ertd_unet_sample(*args, s)
            rc = lib.ertd_unet_sample_plan_create(*args, ctypes.byref(handle))
        else:
            tab = S._Tables(50, ab50, 3, [49, 20, 0], "dpmpp_2m", 0.0, 1.0, cuda_dev)
            keep.append(tab)

            class _Ws:     # _unet_args reads .data_ptr() / .numel()
                data_ptr = staticmethod(lambda: ws)
                numel = staticmethod(lambda: n)
            args = S._unet_args(m, i["cond"], 14 * L, tab, B, o["x"], o["d_prev"], 0, tab.K, 0.0, i["noise"], 0, 0,
                                _Ws, m.packed_weights(cuda_dev))
            if not plan:
                return lib.ertd_unet_sample_solver(*args, s)
            rc = lib.ertd_unet_sample_solver_plan_create(*args, s, ctypes.byref(handle))
        if rc:
            return rc
        rc = lib.ertd_unet_plan_launch(handle, s)
        torch.cuda.synchronize(cuda_dev)
        return rc or lib.ertd_unet_plan_destroy(handle)
    outs = {"x": noise[0].clone()}
    if kind == "solver":
        outs["d_prev"] = Out(B, P)
    clean, _ = run_pair(cuda_dev, call, {"cond": cond, "noise": noise}, outs,
                        lib.ertd_unet_workspace_bytes(ctypes.byref(m.cfg), B, L))
    if kind == "ddpm":     # test_unet_sampler_vs_oracle
        ref = U.sample(cond, W, cfg, T, noise).double().numpy()
    else:                  # test_gpu_solver.py: the table walk in float64 around the spec
        tab = keep[-1]
        with torch.no_grad():
            model = lambda x, t: U.forward(torch.from_numpy(np.asarray(x)).float(), torch.full((B,), int(t)), cond,
                                           W, cfg).double().numpy()
            ref = SR.table_walk(model, tab.t_cpu.tolist(), tab.coef.cpu().double().numpy(), noise[0].numpy(),
                                noise.numpy())
    err = _rel(clean["x"], ref)
    assert err < 1e-4, err


# ---- the reference model: forward and samplers ------------------------------------------------------
def _status(ws, B, L, n, dev):
    st = ctypes.c_int(-1)
    rc = _lib.lib().ertd_sample_status(ws, B, L, n, ctypes.byref(st), _lib.stream_of(dev))
    return rc, st.value


def test_forward(gpu_model, golden_weights, cuda_dev):
    B, L = 3, 37
    x = torch.from_numpy(synth_normal((B, 29), 1))
    t = torch.tensor([0, 499, 250])
    cond = torch.from_numpy(synth_uniform((B, 14, L), 2))
    W = {k: torch.from_numpy(v) for k, v in golden_weights.items()}
    w, packed = gpu_model.weights_struct(), gpu_model.packed_weights(cuda_dev)
    freq = timestep_frequencies(128, cuda_dev)
    lib = _lib.lib()

    def call(i, o, ws, n, dirty):
        return lib.ertd_forward(ctypes.byref(w), packed.data_ptr(), i["x"].data_ptr(), i["t"].data_ptr(),
                                i["cond"].data_ptr(), B, L, freq.data_ptr(), FP32, o["out"].data_ptr(),
                                o["cemb"].data_ptr(), o["temb"].data_ptr(), ws, n, _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, call, {"x": x, "t": t, "cond": cond},
                        {"out": Out(B, 29), "cemb": Out(B, 128), "temb": Out(B, 128)},
                        lib.ertd_workspace_bytes(B, L, 29, 0, _lib.OP_FORWARD))
    assert _rel(clean["out"], RT.forward(x, t, cond, W).double().numpy()) < 1e-5


@pytest.mark.parametrize("mode", ["hoisted", "faithful", "faithful_steps"])
@pytest.mark.parametrize("B,L,T", [(3, 37, 5), (2, 4694, 3)])
def test_sample(B, L, T, mode, gpu_model, golden_weights, cuda_dev):
    """ertd_sample, then ertd_sample_status on the same workspace: ERTD_OK and 0
    in every mode (the hoisted mode clears the word too)."""
    from ertdiff.sampler import _Prepared
    cond = torch.from_numpy(synth_uniform((B, 14, L), 20 + L))
    noise = torch.from_numpy(synth_normal((T, B, 29), 21 + L))
    W = {k: torch.from_numpy(v) for k, v in golden_weights.items()}
    sched = ertdiff.get_diffusion_schedule(T, device=cuda_dev)
    lib = _lib.lib()
    keep, status = [], {}

    def call(i, o, ws, n, dirty):
        prep = _Prepared(gpu_model, i["cond"], T, *sched, None, 1.0, "fp32", False)
        keep.append(prep)
        args = prep.args(B, o["x"], i["noise"], 0, 0, mode, T - 1, T, torch.empty(0))[:-2] + (ws, n)
        rc = lib.ertd_sample(*args, _lib.stream_of(cuda_dev))
        if rc == 0:
            status[dirty] = _status(ws, B, L, T, cuda_dev)
        return rc
    clean, _ = run_pair(cuda_dev, call, {"cond": cond, "noise": noise}, {"x": noise[0].clone()},
                        lib.ertd_workspace_bytes(B, L, 29, T, _lib.OP_SAMPLE))
    assert status[False] == (0, 0) and status[True] == (0, 0), status
    assert _rel(clean["x"], RT.sample(cond, W, T, noise).double().numpy()) < 1e-4


def test_sample_conditions(gpu_model, golden_weights, cuda_dev):
    from ertdiff.sampler import _Conditions, _Prepared
    n_cond, n_samples, L, T = 2, 3, 37, 4
    B = n_cond * n_samples
    cond = torch.from_numpy(synth_uniform((n_cond, 14, L), 31))
    noise = torch.from_numpy(synth_normal((T, B, 29), 32))
    W = {k: torch.from_numpy(v) for k, v in golden_weights.items()}
    sched = ertdiff.get_diffusion_schedule(T, device=cuda_dev)
    lib = _lib.lib()
    keep = []
    for mode in ("hoisted", "faithful"):
        def call(i, o, ws, n, dirty):
            prep = _Prepared(gpu_model, i["cond"], T, *sched, None, 1.0, "fp32", False)
            geo = _Conditions(prep, n_samples, 0, None)
            keep.append(prep)
            args = geo.args(prep, o["x"], i["noise"], 0, mode, T - 1, T, torch.empty(0))[:-2] + (ws, n)
            return lib.ertd_sample_conditions(*args, _lib.stream_of(cuda_dev))
        clean, _ = run_pair(cuda_dev, call, {"cond": cond, "noise": noise}, {"x": noise[0].clone()},
                            lib.ertd_workspace_bytes(B, L, 29, T, _lib.OP_SAMPLE))
        # member j = realisation j // n_cond of condition j % n_cond
        ref = RT.sample(cond.repeat(n_samples, 1, 1), W, T, noise).double().numpy()
        assert _rel(clean["x"], ref) < 1e-4, mode


def test_sample_solver(gpu_model, golden_weights, cuda_dev):
    from ertdiff import solver as S
    B, L, T, TS = 3, 37, 50, [49, 20, 0]
    cond = torch.from_numpy(synth_uniform((B, 14, L), 41))
    noise = torch.from_numpy(synth_normal((len(TS), B, 29), 42))
    ab = ertdiff.get_diffusion_schedule(T)[2]
    tab = S._Tables(T, ab, 3, TS, "dpmpp_2m", 0.0, 1.0, cuda_dev)
    w, packed = gpu_model.weights_struct(), gpu_model.packed_weights(cuda_dev)
    freq = timestep_frequencies(128, cuda_dev)
    lib = _lib.lib()

    def call(i, o, ws, n, dirty):
        return lib.ertd_sample_solver(ctypes.byref(w), packed.data_ptr(), i["cond"].data_ptr(), 14 * L, B, L, tab.K,
                                      0, tab.K, tab.timesteps.data_ptr(), tab.coef.data_ptr(), 0.0, freq.data_ptr(),
                                      i["noise"].data_ptr(), 0, 0, _lib.MODE_HOISTED, FP32, o["x"].data_ptr(),
                                      o["d_prev"].data_ptr(), ws, n, _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, call, {"cond": cond, "noise": noise}, {"x": noise[0].clone(), "d_prev": Out(B, 29)},
                        lib.ertd_workspace_bytes(B, L, 29, tab.K, _lib.OP_SAMPLE))
    W64 = {k: torch.from_numpy(v).double() for k, v in golden_weights.items()}
    cemb = RT.encoder(cond.double(), W64)

    def model(x, t):          # test_gpu_solver.py's float64 model
        xt = torch.from_numpy(np.asarray(x))
        te = F.relu(F.linear(RT.timestep_embedding(torch.full((B,), int(t), dtype=torch.long), 128).double(),
                             W64["time_embed.0.weight"], W64["time_embed.0.bias"]))
        h = F.relu(F.linear(torch.cat([xt, te, cemb], dim=1), W64["mlp.0.weight"], W64["mlp.0.bias"]))
        return F.linear(h, W64["mlp.2.weight"], W64["mlp.2.bias"]).numpy()
    ref = SR.sample(model, ab.numpy(), TS, noise[0].numpy(), "dpmpp_2m", 0.0, 1.0, noise.numpy())
    assert SR.rel_l2(clean["x"].cpu().numpy(), ref) <= 1e-4


# ---- the reference model: train entries -------------------------------------------------------------
def _fresh_model(golden_weights, dev):
    m = ertdiff.ConditionalDiffusionModel(29, 128)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_weights.items()})
    return m.to(dev).train()


HP = (1e-4, 0.9, 0.999, 1e-8)


def _adam_table(n, dev):
    host = torch.zeros(n * 6, dtype=torch.float32)
    assert _lib.lib().ertd_adam_table(1, n, *HP, host.data_ptr()) == 0
    return host.to(dev)


@pytest.mark.parametrize("B,L", [(3, 37), (2, 1)])
@pytest.mark.parametrize("entry", ["step", "step_dev", "steps_dev", "epoch_dev", "validation_epoch_dev"])
def test_train_entries(entry, B, L, golden_weights, cuda_dev):
    """Fresh parameters and Adam state per call; losses, gradients, the drawn
    t / noise, parameters and both Adam moments compared bitwise.  The epoch
    entries run 7 rows (batches of B, the last partial)."""
    T, P, nrows = 500, 29, 7
    lib = _lib.lib()
    epoch = entry.endswith("epoch_dev")
    n = nrows if epoch else B
    nb = -(-n // B) if epoch else 1
    x0 = torch.from_numpy(synth_normal((n, P), 300 + L))
    cond = torch.from_numpy(synth_uniform((n, 14, L), 303 + L))
    t = torch.from_numpy(synth_timesteps(n, T, 301 + L)).long()
    noise = torch.from_numpy(synth_normal((n, P), 302 + L))
    rows = torch.tensor([3, 0, 6, 1, 5, 2, 4], dtype=torch.int32)
    ab = ertdiff.get_diffusion_schedule(T, device=cuda_dev)[2].contiguous()
    freq = timestep_frequencies(128, cuda_dev)
    table = _adam_table(16, cuda_dev)
    draw = entry in ("steps_dev", "epoch_dev")
    from ertdiff.model import STATE_KEYS
    shapes = [tuple(golden_weights[k].shape) for k in STATE_KEYS]

    def call(i, o, ws, nbytes, dirty):
        s = _lib.stream_of(cuda_dev)
        m = _fresh_model(golden_weights, cuda_dev)
        params = m._params()
        w = m.weights_struct()
        grads = [o[f"grad{k}"] for k in range(12)] if entry != "validation_epoch_dev" else []
        ea =[torch.zeros_like(p) for p in params]
        es = [torch.zeros_like(p) for p in params]
        step_dev = torch.zeros(1, dtype=torch.int32, device=cuda_dev)
        tt, nz = (o["t"], o["noise"]) if draw else (i["t"], i["noise"])
        G, EA, ES = _lib.ptr_array(grads), _lib.ptr_array(ea), _lib.ptr_array(es)
        if entry == "step":
            rc = lib.ertd_train_step(ctypes.byref(w), None, i["x0"].data_ptr(), tt.data_ptr(), nz.data_ptr(),
                                     i["cond"].data_ptr(), ab.data_ptr(), B, L, freq.data_ptr(), G, EA, ES, 1, *HP,
                                     o["loss"].data_ptr(), ws, nbytes, s)
        elif entry == "step_dev":
            rc = lib.ertd_train_step_dev(ctypes.byref(w), i["x0"].data_ptr(), tt.data_ptr(), nz.data_ptr(),
                                         i["cond"].data_ptr(), ab.data_ptr(), B, L, freq.data_ptr(), G, EA, ES,
                                         step_dev.data_ptr(), table.data_ptr(), 1, 16, 0, T, 1234,
                                         o["loss"].data_ptr(), ws, nbytes, s)
        elif entry == "steps_dev":
            rc = lib.ertd_train_steps_dev(ctypes.byref(w), i["x0"].data_ptr(), tt.data_ptr(), nz.data_ptr(),
                                          i["cond"].data_ptr(), ab.data_ptr(), B, L, freq.data_ptr(), G, EA, ES,
                                          step_dev.data_ptr(), table.data_ptr(), 1, 16, 1, T, 1234, 3,
                                          o["loss"].data_ptr(), ws, nbytes, s)
        elif entry == "epoch_dev":
            rc = lib.ertd_train_epoch_dev(ctypes.byref(w), i["x0"].data_ptr(), i["cond"].data_ptr(), nrows,
                                          i["rows"].data_ptr(), nrows, tt.data_ptr(), nz.data_ptr(), ab.data_ptr(),
                                          B, L, freq.data_ptr(), G, EA, ES, step_dev.data_ptr(), table.data_ptr(),
                                          1, 16, 1, T, 1234, o["loss"].data_ptr(), ws, nbytes, s)
        else:
            rc = lib.ertd_validation_epoch_dev(ctypes.byref(w), i["x0"].data_ptr(), i["cond"].data_ptr(), nrows,
                                               i["rows"].data_ptr(), nrows, tt.data_ptr(), nz.data_ptr(),
                                               ab.data_ptr(), B, L, freq.data_ptr(), None, 0, T, 1234,
                                               o["eps"].data_ptr(), o["loss"].data_ptr(), ws, nbytes, s)
        torch.cuda.synchronize(cuda_dev)
        if entry != "validation_epoch_dev":
            for k in range(12):
                o[f"param{k}"], o[f"exp_avg{k}"], o[f"exp_avg_sq{k}"] = params[k].detach(), ea[k], es[k]
            o["step_dev"] = step_dev
        return rc
    ins = {"x0": x0, "cond": cond, "rows": rows if epoch else None}
    outs = {"loss": Out(nb)}
    if draw:
        outs.update(t=Out(n, dtype=torch.int64), noise=Out(n, P))
    else:
        ins.update(t=t, noise=noise)
    if entry == "validation_epoch_dev":
        outs["eps"] = Out(n, P)
    else:
        outs.update({f"grad{k}": Out(*shapes[k]) for k in range(12)})
    clean, _ = run_pair(cuda_dev, call, ins, outs, lib.ertd_workspace_bytes(B, L, P, 0, _lib.OP_TRAIN))
    if entry in ("step", "step_dev"):     # test_grads_vs_fp64_backward
        a = ab.cpu().double()[t].numpy()[:, None]      # x = q_sample(x0, t, noise) in float64
        xn = np.sqrt(a) * x0.double().numpy() + np.sqrt(1 - a) * noise.double().numpy()
        f = RN.forward_full(xn, t.numpy(), cond.numpy(), golden_weights)
        ref_loss, g = RN.backward(f, noise.numpy(), golden_weights)
        assert abs(float(clean["loss"][0]) - ref_loss) < 1e-5 * ref_loss
        for k, name in enumerate(STATE_KEYS):
            if np.linalg.norm(g[name]) == 0:
                assert float(clean[f"grad{k}"].abs().max()) == 0.0, name
            else:
                assert _rel(clean[f"grad{k}"], g[name]) < 1e-4, name
    elif entry == "validation_epoch_dev":
        # eps = model(q_sample(x0[rows], t, noise), t, cond[rows]); per-batch MSE (float64)
        r, a = rows.long(), ab.cpu().double()[t]
        xn = (a.sqrt()[:, None] * x0[r].double() + (1 - a).sqrt()[:, None] * noise.double()).float()
        W = {k: torch.from_numpy(v) for k, v in golden_weights.items()}
        eps = RT.forward(xn, t, cond[r], W).double()
        assert _rel(clean["eps"], eps.numpy()) < 1e-5
        for b in range(nb):
            sl = slice(b * B, min((b + 1) * B, nrows))
            ref = float(((eps[sl] - noise[sl].double()) ** 2).mean())
            assert abs(float(clean["loss"][b]) - ref) < 1e-5 * ref, b
    else:
        assert int(clean["step_dev"][0]) == (3 if entry == "steps_dev" else nb)
        assert int(clean["t"].min()) >= 0 and int(clean["t"].max()) < T


# ---- sort, Wasserstein, MinMax ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tiles", [1, 5])
def test_rows_sort_and_wasserstein(tiles, dtype, cuda_dev):
    lib = _lib.lib()
    code = _lib_dtype(dtype)
    M = tiles * lib.ertd_rows_sort_tile(code) + 7
    nrow = 2
    g = torch.Generator().manual_seed(M)
    u = torch.randn(nrow, M, generator=g, dtype=torch.float64).to(dtype)
    v = (torch.randn(M, generator=g, dtype=torch.float64) * 1.3 + 0.2).to(dtype)

    def sort(i, o, ws, n, dirty):
        return lib.ertd_rows_sort(i["u"].data_ptr(), code, nrow, M, M, o["sorted"].data_ptr(), ws, n,
                                  _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, sort, {"u": u}, {"sorted": Out(nrow, M, dtype=dtype)},
                        lib.ertd_rows_sort_ws_bytes(code, nrow, M))
    assert torch.equal(clean["sorted"].cpu(), torch.sort(u, dim=1).values)

    def w1(i, o, ws, n, dirty):
        return lib.ertd_wasserstein(i["u"].data_ptr(), code, nrow, M, M, i["v"].data_ptr(), M, o["w1"].data_ptr(),
                                    ws, n, _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, w1, {"u": u, "v": v}, {"w1": Out(nrow, dtype=torch.float64)},
                        lib.ertd_wasserstein_ws_bytes(code, nrow, M, M))
    # equal sizes: W1 = mean |sorted u - sorted v| (float64); the device adds scipy's terms
    # in another order: <= (Mu + Mv) eps relative
    vs = torch.sort(v.double()).values
    ref = (torch.sort(u.double(), dim=1).values - vs).abs().mean(1)
    assert torch.allclose(clean["w1"].cpu(), ref, rtol=2 * M * 2.2e-16, atol=0)


def _lib_dtype(dtype):
    return 0 if dtype == torch.float32 else 1     # ERTD_F32 / ERTD_F64


def test_minmax_partial_fit(cuda_dev):
    n, Fd = 300, 14
    lib = _lib.lib()
    X = torch.randn(n, Fd, generator=torch.Generator().manual_seed(5), dtype=torch.float64)

    def call(i, o, ws, nb, dirty):
        return lib.ertd_minmax_partial_fit(i["X"].data_ptr(), n, Fd, Fd, o["min"].data_ptr(), o["max"].data_ptr(), 0,
                                           ws, nb, _lib.stream_of(cuda_dev))
    clean, _ = run_pair(cuda_dev, call, {"X": X}, {"min": Out(Fd, dtype=torch.float64), "max": Out(Fd, dtype=torch.float64)},
                        lib.ertd_minmax_ws_bytes(n, Fd))
    assert torch.equal(clean["min"].cpu(), X.min(0).values) and torch.equal(clean["max"].cpu(), X.max(0).values)


# ---- too small is refused cleanly ---------------------------------------------------------------------
def test_workspace_one_byte_short_is_refused(gpu_model, cuda_dev):
    """ws_bytes = query - 1 where the query is tight: ERTD_ENOSPC, nothing
    launched -- the 0xFF-prefilled output is untouched.  (Read first: every one
    of these entries compares its layout with ws_bytes before its first launch
    -- conv2d_impl, ertd_conv_input_grad, the U-Net walk's dry pass,
    enqueue_sample, ertd_minmax_partial_fit.)"""
    from ertdiff.sampler import _Prepared
    lib = _lib.lib()
    dev = cuda_dev
    s = _lib.stream_of(dev)

    def untouched(t):
        torch.cuda.synchronize(dev)
        return bool((t.reshape(-1).view(torch.uint8) == 0xFF).all())

    def refused(rc, out, what):
        assert rc == _lib.ERTD_ENOSPC, (what, rc)
        assert untouched(out), what
        DS.check_fences(out)

    # conv2d fp32 with a K split; conv2d bf16 3x3 gn_silu
    for (Ca, Cout, H, B, act, prec) in ((64, 64, 16, 2, "gn_silu", FP32), (32, 64, 16, 2, "gn_silu", BF16)):
        t, Ho = _conv_inputs(Ca, 0, Cout, H, 3, "same", act, B, 900, epilogue=False)
        inp = {k: None if v is None else v.to(dev) for k, v in t.items()}
        out = {"out": DS.fenced_empty((B, Cout, Ho, Ho), device=dev, name="out")}
        q = lib.ertd_conv2d_workspace_bytes(Ca, Cout, 3, prec, B, H, 0)
        ws = DS.poisoned_ws(q, dev)
        refused(_conv_call(Ca, 0, Cout, H, 3, "same", act, B, prec)(inp, out, ws.data_ptr(), q - 1, True),
                out["out"], f"conv2d prec {prec}")
    # conv_input_grad
    Cin, Cout, H, B = 64, 64, 32, 2
    q = lib.ertd_conv_input_grad_ws_bytes(Cin, Cout, B, H, 3, 0)
    ws, dx = DS.poisoned_ws(q, dev), DS.fenced_empty((B, Cin, H, H), device=dev, name="dx")
    dy, w = torch.zeros(B, Cout, H, H, device=dev), torch.zeros(Cout, Cin, 3, 3, device=dev)
    refused(lib.ertd_conv_input_grad(dy.data_ptr(), B, H, w.data_ptr(), Cout, Cin, 3, 0, dx.data_ptr(), 0,
                                     ws.data_ptr(), q - 1, s), dx, "conv_input_grad")
    # unet_forward
    m = ertdiff.ConditionalUNet.from_config("U1", seed=0).to(dev).eval()
    B, L, P = 2, 65, m.param_dim
    q = lib.ertd_unet_workspace_bytes(ctypes.byref(m.cfg), B, L)
    ws, out = DS.poisoned_ws(q, dev), DS.fenced_empty((B, P), device=dev, name="eps")
    x, tt, cond = torch.zeros(B, P, device=dev), torch.zeros(B, dtype=torch.int64, device=dev), \
        torch.zeros(B, 14, L, device=dev)
    refused(lib.ertd_unet_forward(ctypes.byref(m.cfg), m.packed_weights(dev).data_ptr(), x.data_ptr(), tt.data_ptr(),
                                  cond.data_ptr(), 14 * L, L, B, out.data_ptr(), None, ws.data_ptr(), q - 1, s),
            out, "unet_forward")
    # sample
    B, L, T = 3, 37, 5
    sched = ertdiff.get_diffusion_schedule(T, device=dev)
    prep = _Prepared(gpu_model, torch.zeros(B, 14, L, device=dev), T, *sched, None, 1.0, "fp32", False)
    q = lib.ertd_workspace_bytes(B, L, 29, T, _lib.OP_SAMPLE)
    ws, x = DS.poisoned_ws(q, dev), DS.fenced_empty((B, 29), device=dev, name="x")
    for mode in ("hoisted", "faithful", "faithful_steps"):
        args = prep.args(B, x, None, 0, 0, mode, T - 1, T, torch.empty(0))[:-2] + (ws.data_ptr(), q - 1)
        refused(lib.ertd_sample(*args, s), x, f"sample {mode}")
    # minmax_partial_fit
    n, Fd = 300, 14
    q = lib.ertd_minmax_ws_bytes(n, Fd)
    ws = DS.poisoned_ws(q, dev)
    X = torch.zeros(n, Fd, dtype=torch.float64, device=dev)
    mn, mx = (DS.fenced_empty((Fd,), torch.float64, dev, name=k) for k in ("min", "max"))
    rc = lib.ertd_minmax_partial_fit(X.data_ptr(), n, Fd, Fd, mn.data_ptr(), mx.data_ptr(), 0, ws.data_ptr(), q - 1, s)
    refused(rc, mn, "minmax_partial_fit")
    assert untouched(mx)
