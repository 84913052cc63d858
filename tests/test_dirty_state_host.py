"""tests/dirty_state.py catches what it is for -- shown on the CPU with tiny
stand-in "entries" written in torch, each with the call shape of a library
entry (inputs, output, caller-owned workspace) and each misbehaving in exactly
one way.  The GPU tests (test_gpu_dirty_entries.py, test_gpu_dirty_api.py) run
the same clean-vs-dirty protocol on the real entries; this file is the proof
that the protocol can fail."""
import pytest
import torch

import dirty_state as DS

N = 37


def _past(t, before=0, after=0):
    """``t`` widened by elements before / after it -- inside its allocation
    (the fences), which is where a kernel's off-by-one lands."""
    return torch.as_strided(t, (t.numel() + before + after,), (1,), t.storage_offset() - before)


def entry_good(x, out, ws):
    w = ws.view(torch.float32)
    w[:N] = x * 2.0            # writes its scratch, then reads it
    out[:] = w[:N] + 1.0


def entry_reads_ws_first(x, out, ws):
    w = ws.view(torch.float32)
    out[:] = x * 2.0 + 1.0 + w[0]    # w[0] "is zero between calls"
    w[:N] = x


def entry_leaves_hole(x, out, ws):
    w = ws.view(torch.float32)
    w[:N] = x * 2.0
    out[:N - 1] = w[:N - 1] + 1.0    # the last element is never written


def entry_writes_past_out(x, out, ws):
    entry_good(x, out, ws)
    _past(out, after=1)[N] = 7.0     # one element past the output


def entry_writes_past_ws(x, out, ws):
    entry_good(x, out, ws)
    _past(ws, after=1)[ws.numel()] = 1   # one byte past ws + ws_bytes


def entry_reads_before_input(x, out, ws):
    w = ws.view(torch.float32)
    w[:N] = x * 2.0
    out[:] = w[:N] + 1.0
    out[0] += _past(x, before=1)[0]  # folds x[-1] into the first sum


def _protocol(entry):
    """The protocol of the GPU tests: a clean call (zero neighbours, zero
    workspace, zero output) and a dirty call (NaN input bands, exactly sized
    0xFF workspace, 0xFF output) on identical inputs; bitwise equality, finite
    values, intact fences."""
    x = torch.linspace(-1.0, 1.0, N)
    xc = DS.fenced(x, fill=0, name="x")
    outc = DS.fenced_empty((N,), interior=0, name="out")
    wsc = DS.fenced_empty((4 * N + 256,), torch.uint8, interior=0, name="ws")
    entry(xc, outc, wsc)
    xd = DS.fenced(x, name="x")
    outd = DS.fenced_empty((N,), name="out")
    wsd = DS.poisoned_ws(4 * N)
    entry(xd, outd, wsd)
    DS.assert_same_bits(outd, outc, "out")
    DS.check_fences(xd, outd, wsd)
    assert torch.equal(outc, x * 2.0 + 1.0)


def test_well_behaved_entry_passes():
    _protocol(entry_good)


@pytest.mark.parametrize("entry,what", [
    (entry_reads_ws_first, "out: .*non-finite"),
    (entry_leaves_hole, "out: .*non-finite values on dirty memory, first at flat index 36"),
    (entry_writes_past_out, "out: write past the end, first changed byte at offset 148 of a 148-byte"),
    (entry_writes_past_ws, "ws: write past the end, first changed byte at offset 148 of a 148-byte"),
    (entry_reads_before_input, "out: .*non-finite values on dirty memory, first at flat index 0"),
])
def test_each_defect_is_caught(entry, what):
    with pytest.raises(AssertionError, match=what):
        _protocol(entry)


def test_defects_pass_on_zero_memory():
    """The same stand-ins on today's kind of memory (zeros everywhere): the
    read-before-write, the hole and the stray read all go unnoticed -- which is
    the gap."""
    x = torch.linspace(-1.0, 1.0, N)
    for entry in (entry_reads_ws_first, entry_leaves_hole, entry_reads_before_input):
        xc = DS.fenced(x, fill=0)
        out = DS.fenced_empty((N,), interior=0)
        entry(xc, out, DS.fenced_empty((4 * N,), torch.uint8, interior=0))
        ref = x * 2.0 + 1.0
        if entry is entry_leaves_hole:
            ref[-1] = 0.0
        assert torch.equal(out, ref)


def test_bitwise_mismatch_is_reported_with_index():
    a = torch.arange(8.0)
    b = a.clone()
    b[5] = -0.0 + 5.0000005
    with pytest.raises(AssertionError, match="first at flat index 5"):
        DS.assert_same_bits(b, a)
    assert DS.bitwise_equal(a, a.clone())
    assert not DS.bitwise_equal(torch.tensor([0.0]), torch.tensor([-0.0]))   # bits, not values
    nan = torch.full((3,), float("nan"))
    assert DS.bitwise_equal(nan, nan.clone())
    with pytest.raises(AssertionError, match="non-finite"):
        DS.assert_same_bits(nan, nan.clone())


def test_fence_layout_and_bands():
    x = torch.arange(10, dtype=torch.float32)
    f = DS.fenced(x)
    assert torch.equal(f, x) and f.is_contiguous()
    assert f.data_ptr() % 16 == 0
    assert torch.isnan(_past(f, before=1)[0]) and torch.isnan(_past(f, after=1)[10])
    i = DS.fenced(torch.arange(5, dtype=torch.int32))
    assert int(_past(i, before=1)[0]) == int.from_bytes(bytes([DS.PATTERN_BYTE] * 4), "little", signed=True)
    o = DS.fenced_empty((2, 3), torch.float32)
    assert bool(torch.isnan(o).all())
    assert DS.PATTERN_BYTE not in (0x00, 0xFF)
    w = DS.poisoned_ws(1001)
    assert w.numel() == 1001 and w.dtype == torch.uint8 and bool((w == 0xFF).all())
    assert bool((w.view(torch.int8) == -1).all())
    assert bool(torch.isnan(DS.poisoned_ws(8).view(torch.bfloat16)).all())
    DS.check_fences(f, i, o, w, None)
    # a write before the start is named with a negative offset
    _past(o.view(-1), before=2)[0] = 1.0
    with pytest.raises(AssertionError, match=r"write before the start, first changed byte at offset -8"):
        DS.check_fences(o)
    with pytest.raises(TypeError):
        DS.check_fences(torch.zeros(3))
    z = DS.fenced(torch.zeros(0))
    assert z.numel() == 0
    DS.check_fences(z)


def test_dirty_allocator(monkeypatch):
    real_empty, real_like = torch.empty, torch.empty_like
    with DS.dirty_allocator(monkeypatch):
        assert torch.empty is not real_empty
        c = torch.empty(64)     # CPU tensors are left alone by default
        assert c.device.type == "cpu"
    assert torch.empty is real_empty and torch.empty_like is real_like
    # the mechanism itself, pointed at the CPU so that it runs here
    with DS.dirty_allocator(devices=("cpu",)):
        a = torch.empty(5, 7)
        b = torch.empty_like(torch.zeros(3, dtype=torch.int32))
        s = torch.empty((), dtype=torch.float32)
        h = torch.empty(6, dtype=torch.bfloat16)
        e = torch.empty(0)
        z = torch.zeros(4)
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(s)) and bool(torch.isnan(h).all())
    assert bool((b == -1).all()) and e.numel() == 0 and bool((z == 0).all())
    assert torch.empty is real_empty and torch.empty_like is real_like
    with pytest.raises(ZeroDivisionError):
        with DS.dirty_allocator(devices=("cpu",)):
            1 / 0
    assert torch.empty is real_empty and torch.empty_like is real_like


def test_sentinel_tail_catches_one_word_past_the_end():
    out = DS.sentinel_empty((3, 5), name="out")
    assert out.shape == (3, 5) and out.dtype == torch.float32 and bool(torch.isnan(out).all())
    tail = out._tail.raw[out.numel():]
    assert tail.numel() == DS.SENTINEL_WORDS and bool((tail == DS.SENTINEL_WORD).all())
    out.fill_(1.0)                       # writes inside the tensor leave the tail alone
    DS.check_sentinel(out)
    out._tail.raw[out.numel() + 7] = 0   # one word behind the last element
    with pytest.raises(AssertionError, match="out: write past the end, first changed word 7"):
        DS.check_sentinel(out)
    with pytest.raises(TypeError):
        DS.check_sentinel(torch.zeros(2))
