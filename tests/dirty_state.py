"""Control over the state a call inherits: fenced tensors, poisoned workspaces
and a poisoning allocator.

The library allocates nothing: every entry works in caller-owned memory, and
its contract (include/ertdiff.h, "Workspace contract") is that the contents of
a workspace or an output on entry are arbitrary, that nothing is read before
the call writes it, and that nothing outside [ws, ws + ws_bytes) or outside the
outputs is written.  torch.empty very often hands out zeros, which hides a
skipped zeroing, an unwritten pad lane multiplied by a zero weight, or a partial
buffer read before it is written.  The tools here take that luck away:

  fenced(t)            a copy of t inside a larger allocation with a band of
                       guard_bytes on each side (inputs: NaN bands, so a read
                       one element outside shows in the result);
  fenced_empty(...)    an output inside such an allocation: pattern bands,
                       interior prefilled with 0xFF bytes;
  poisoned_ws(n)       a workspace of EXACTLY n bytes, 0xFF inside (fp32 / bf16
                       NaN, 0xFFFFFFFF counters, -1 integers), pattern bands;
  check_fences(...)    every band byte for byte intact, else the tensor's name
                       and the first changed offset;
  sentinel_empty(...)  an fp32 output followed by 4096 words 0x7FC0DEAD in the
                       same allocation (a work item too many writes there);
  check_sentinel(...)  every one of those words intact;
  dirty_allocator()    for its duration torch.empty / torch.empty_like fill
                       every CUDA tensor they return with 0xFF bytes.

Every band lies inside memory this module allocated: nothing here reads or
writes outside an allocation.  Importing needs no GPU."""
from __future__ import annotations

import contextlib

import torch

GUARD_BYTES = 4096   # a multiple of every alignment an entry assumes (16 B vector loads, 256 B slots)
NAN_BYTE = 0xFF      # 0xFF.. is a NaN in fp64 / fp32 / fp16 / bf16
PATTERN_BYTE = 0xA5  # neither 0x00 nor 0xFF: fp32 0xA5A5A5A5 = -2.9e-16, int32 -1515870811
POISON_BYTE = 0xFF
_REAL_EMPTY = torch.empty


class _Fence:
    __slots__ = ("raw", "guard", "nbytes", "byte", "name")

    def __init__(self, raw, guard, nbytes, byte, name):
        self.raw, self.guard, self.nbytes, self.byte, self.name = raw, guard, nbytes, byte, name


def _band_byte(fill, dtype) -> int:
    if isinstance(fill, int):
        if not 0 <= fill <= 255:
            raise ValueError("fill byte out of range")
        return fill
    if fill == "nan":   # integer inputs have no NaN: the fixed pattern byte
        return NAN_BYTE if (dtype.is_floating_point or dtype.is_complex) else PATTERN_BYTE
    if fill == "pattern":
        return PATTERN_BYTE
    raise ValueError(f"fill must be 'nan', 'pattern' or a byte, got {fill!r}")


def _carve(shape, dtype, device, guard_bytes, band, interior, name):
    guard_bytes = int(guard_bytes)
    if guard_bytes <= 0 or guard_bytes % 16:
        raise ValueError("guard_bytes must be a positive multiple of 16")
    n = 1
    for s in shape:
        n *= int(s)
    itemsize = torch.empty((), dtype=dtype).element_size()
    nbytes = n * itemsize
    raw = torch.full((2 * guard_bytes + nbytes,), band, dtype=torch.uint8, device=device)
    inner = raw[guard_bytes:guard_bytes + nbytes]
    if interior is not None and interior != band:
        inner.fill_(interior)
    view = inner.view(dtype).view(tuple(int(s) for s in shape)) if nbytes else \
        torch.empty(tuple(int(s) for s in shape), dtype=dtype, device=device)
    view._fence = _Fence(raw, guard_bytes, nbytes, band, name or "tensor")
    return view


def fenced(t: torch.Tensor, guard_bytes: int = GUARD_BYTES, fill="nan", name=None, device=None):
    """A contiguous copy of ``t`` (moved to ``device`` if given) inside a larger
    allocation with a band of ``guard_bytes`` bytes on each side.  fill="nan":
    the bands hold NaN (for an integer ``t`` the pattern byte) -- an input;
    fill="pattern": the pattern byte -- an output or workspace that carries
    values in; an int: that byte (0: the benign neighbours of today's tests)."""
    device = t.device if device is None else torch.device(device)
    out = _carve(t.shape, t.dtype, device, guard_bytes, _band_byte(fill, t.dtype), None, name)
    if t.numel():
        out.copy_(t)
    return out


def fenced_empty(shape, dtype=torch.float32, device="cpu", guard_bytes: int = GUARD_BYTES,
                 interior: int = POISON_BYTE, name=None):
    """An output: pattern bands, every interior byte ``interior`` (0xFF)."""
    if isinstance(shape, int):
        shape = (shape,)
    return _carve(tuple(shape), dtype, torch.device(device), guard_bytes, PATTERN_BYTE, interior, name)


def poisoned_ws(nbytes: int, device="cpu", guard_bytes: int = GUARD_BYTES, name="ws"):
    """A workspace of exactly ``nbytes`` bytes (the value the entry's
    *_ws_bytes / *_workspace_bytes query returned), all 0xFF, fenced."""
    return fenced_empty((int(nbytes),), torch.uint8, device, guard_bytes, POISON_BYTE, name)


SENTINEL_WORD = 0x7FC0DEAD   # a quiet fp32 NaN no arithmetic produces
SENTINEL_WORDS = 4096


class _Tail:
    __slots__ = ("raw", "numel", "word", "name")

    def __init__(self, raw, numel, word, name):
        self.raw, self.numel, self.word, self.name = raw, numel, word, name


def sentinel_empty(shape, device="cpu", words: int = SENTINEL_WORDS, word: int = SENTINEL_WORD, name=None):
    """An fp32 output whose last element is followed, in the same allocation,
    by ``words`` 32-bit words ``word``: an entry that runs one work item too
    many writes there.  Interior prefilled with 0xFF bytes (NaN)."""
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    if not 0 <= word < 2 ** 31:
        raise ValueError("word must fit a non-negative int32")
    raw = torch.full((n + int(words),), -1, dtype=torch.int32, device=torch.device(device))
    raw[n:] = word
    view = raw[:n].view(torch.float32).view(shape)
    view._tail = _Tail(raw, n, word, name or "tensor")
    return view


def check_sentinel(*tensors):
    """Assert that every word behind each sentinel_empty tensor still holds its value."""
    for t in tensors:
        f = getattr(t, "_tail", None)
        if f is None:
            raise TypeError("check_sentinel: not a tensor made by sentinel_empty")
        bad = (f.raw[f.numel:] != f.word).nonzero()
        if bad.numel():
            i = int(bad[0])
            raise AssertionError(f"{f.name}: write past the end, first changed word {i} behind a "
                                 f"{f.numel}-element tensor (0x{int(f.raw[f.numel + i]) & 0xFFFFFFFF:08x}, "
                                 f"sentinel 0x{f.word:08x}), {bad.numel()} words changed")


def _first_changed(band: torch.Tensor, byte: int):
    bad = (band != byte).nonzero()
    return None if bad.numel() == 0 else int(bad[0])


def check_fences(*tensors):
    """Assert that both bands of every fenced tensor still hold their byte.
    Offsets in the message are bytes relative to the tensor: negative = before
    its first byte, >= nbytes = past its last."""
    for t in tensors:
        if t is None:
            continue
        f = getattr(t, "_fence", None)
        if f is None:
            raise TypeError("check_fences: not a tensor made by fenced / fenced_empty / poisoned_ws")
        lead = f.raw[:f.guard]
        trail = f.raw[f.guard + f.nbytes:]
        i = _first_changed(trail, f.byte)
        if i is not None:
            raise AssertionError(f"{f.name}: write past the end, first changed byte at offset "
                                 f"{f.nbytes + i} of a {f.nbytes}-byte tensor "
                                 f"(0x{int(trail[i]):02x}, fence 0x{f.byte:02x})")
        i = _first_changed(lead, f.byte)
        if i is not None:
            raise AssertionError(f"{f.name}: write before the start, first changed byte at offset "
                                 f"{i - f.guard} (0x{int(lead[i]):02x}, fence 0x{f.byte:02x})")


def _bytes(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def bitwise_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape, dtype and bytes (NaNs compare by their bits)."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bytes(a).cpu(), _bytes(b).cpu()))


def assert_same_bits(dirty: torch.Tensor, clean: torch.Tensor, name: str = "output", finite: bool = True):
    """The clean-vs-dirty comparison: the call on poisoned memory gave, bit for
    bit, what the call on zero-filled memory gave, and (floats) all finite."""
    assert dirty.shape == clean.shape and dirty.dtype == clean.dtype, \
        f"{name}: {tuple(dirty.shape)} {dirty.dtype} vs {tuple(clean.shape)} {clean.dtype}"
    if finite and dirty.dtype.is_floating_point:
        bad = (~torch.isfinite(dirty)).reshape(-1).nonzero()
        assert bad.numel() == 0, (f"{name}: {bad.numel()} non-finite values on dirty memory, first at "
                                  f"flat index {int(bad[0])}")
    da, ca = _bytes(dirty).cpu(), _bytes(clean).cpu()
    if not torch.equal(da, ca):
        i = int((da != ca).nonzero()[0]) // max(dirty.element_size(), 1)
        raise AssertionError(f"{name}: dirty and clean calls differ, first at flat index {i}: "
                             f"{dirty.reshape(-1)[i].item()!r} vs {clean.reshape(-1)[i].item()!r}")


def _poison(t: torch.Tensor, devices) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type not in devices or t.numel() == 0:
        return t
    if t.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return t   # a fill inside a capture would become a node of the graph
    st = t.untyped_storage()
    _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),)).fill_(POISON_BYTE)
    return t


@contextlib.contextmanager
def dirty_allocator(monkeypatch=None, devices=("cuda",)):
    """While active, torch.empty and torch.empty_like fill every tensor they
    return on ``devices`` (default: CUDA only; CPU tensors are left alone) with
    0xFF bytes, except while the current stream is capturing.  This poisons the
    torch.empty workspaces and outputs inside ertdiff/*.py without editing
    them.  With a pytest ``monkeypatch`` the patch is undone by it as well."""
    real_empty, real_empty_like = torch.empty, torch.empty_like
    devices = tuple(devices)

    def empty(*args, **kwargs):
        return _poison(real_empty(*args, **kwargs), devices)

    def empty_like(*args, **kwargs):
        return _poison(real_empty_like(*args, **kwargs), devices)

    if monkeypatch is not None:
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", empty)
            m.setattr(torch, "empty_like", empty_like)
            yield
        return
    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like
