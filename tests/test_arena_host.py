"""The guard-band harness (tests/_arena.py) bites: small Python stand-ins for a kernel, on CPU tensors.  Every mutant below is
what a wrong kernel does to memory; each must be reported, and with a message that names the case, the operand, the side and
the byte offset.  A correct stand-in passes.  This is the evidence that a case of tests/test_gpu_arena.py fails if a kernel strays."""
import re

import pytest

torch = pytest.importorskip("torch")

import _arena                                        # noqa: E402
from _arena import Case, In, InOut, Out, Scratch     # noqa: E402

B, N = 3, 1000              # three batch elements of 1000 floats


def _around(t, first, count):
    """`count` elements of t's storage from element `first` of t on (negative: in front of it), or None where the storage
    ends — a plain allocation has nothing around it, as the neighbours of a real one are nobody's business."""
    flat = t.reshape(-1)
    off = flat.storage_offset() + first
    room = flat.untyped_storage().nbytes() // flat.element_size()
    if off < 0 or off + count > room:
        return None
    return torch.as_strided(flat, (count,), (1,), off)


def _good(b):
    b["ws"][:8] = 1
    b["y"].copy_(b["x"] * 2.0 + b["w"][0])
    return 0


def _operands():
    g = torch.Generator().manual_seed(1)
    return [In("x", torch.randn(B, N, generator=g), batch=B), In("w", torch.randn(4, generator=g)),
            Out("y", (B, N), torch.float32, batch=B), Scratch("ws", 100)]


def _mutant(after):
    def call(b):
        _good(b)
        after(b)
        return 0
    return call


def _poke(t, first, count=1):
    v = _around(t, first, count)
    if v is not None:
        v.fill_(7)


def _read_before_input(b):
    v = _around(b["x"], -1, 1)
    b["y"].reshape(-1)[0] += (v[0] if v is not None else 0.0)


MUTANTS = [
    ("one element past the output", lambda b: _poke(b["y"], B * N), r"operand 'y' \(out\): back pad changed .* offset \+%d " % (4 * B * N)),
    ("one element before the output", lambda b: _poke(b["y"], -1), r"operand 'y' \(out\): front pad changed .* offset -4 "),
    ("one batch element past the output", lambda b: _poke(b["y"], B * N, N), r"operand 'y' \(out\): back pad changed .* offset \+%d " % (4 * B * N)),
    ("reads the element before its input", _read_before_input, r"input pads \+1024.0\]: operand 'y' \(out\) differs from the run on plain allocations.* offset \+[0-3] "),
    ("modifies its input", lambda b: b["x"].reshape(-1)[5].fill_(9.0), r"operand 'x' \(in\) was modified.* offset \+2[0-3] "),
    ("writes past its scratch", lambda b: _poke(b["ws"], 100), r"operand 'ws' \(scratch\): back pad changed .* offset \+100 "),
    ("writes into the pad behind a read-only operand", lambda b: _poke(b["w"], 4), r"operand 'w' \(in\): back pad changed .* offset \+1[6-9] "),     # 7.0f = 00 00 E0 40: its low bytes equal the 0.0 fill
]


def test_a_correct_stand_in_passes():
    got = _arena.run(Case("good", _good, _operands()))
    ops = {o.name: o for o in _operands()}
    assert torch.equal(got["y"], ops["x"].data * 2.0 + ops["w"].data[0])


@pytest.mark.parametrize("name,after,message", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_is_reported_and_named(name, after, message):
    with pytest.raises(_arena.ArenaError) as e:
        _arena.run(Case("mutant: " + name, _mutant(after), _operands()))
    text = str(e.value)
    assert text.startswith("mutant: " + name + " ["), text
    assert re.search(message, text), text


def test_a_bad_return_code_is_reported():
    with pytest.raises(_arena.ArenaError, match=r"failing \[plain allocations\]: return code -3"):
        _arena.run(Case("failing", lambda b: -3, _operands()))
    calls = []

    def fails_in_an_arena(b):
        calls.append(1)
        _good(b)
        return 0 if len(calls) < 3 else -1
    with pytest.raises(_arena.ArenaError, match=r"late \[arenas, input pads \+1024.0\]: return code -1"):
        _arena.run(Case("late", fails_in_an_arena, _operands()))


def test_an_output_nobody_wrote_is_reported():
    with pytest.raises(_arena.ArenaError, match=r"idle \[plain allocations\]: operand 'y' \(out\) was never written"):
        _arena.run(Case("idle", lambda b: 0, _operands()))


def test_aliased_operand_and_integer_fills():
    """inout: checked against the plain run, its pads hold the poison of the run like an input's (the call reads it) and are
    checked like any pad; integer inputs get the byte fills."""
    k = torch.arange(50, dtype=torch.int32)

    def good(b):
        b["acc"] += b["k"].to(torch.float32)
        return 0
    _arena.run(Case("aliased", good, [In("k", k), InOut("acc", torch.ones(50))]))

    def reads_pad(b):
        good(b)
        v = _around(b["k"], 50, 1)
        b["acc"][0] += float(v[0]) if v is not None else 0.0
        return 0
    with pytest.raises(_arena.ArenaError, match=r"input pads \+1024.0/0x7F\]: operand 'acc' \(inout\) differs"):
        _arena.run(Case("aliased, reads k's pad", reads_pad, [In("k", k), InOut("acc", torch.ones(50))]))

    def reads_its_own_pad(b):                 # a halo load outside the aliased operand itself
        good(b)
        v = _around(b["acc"], -1, 1)
        b["acc"][0] += (v[0] if v is not None else 0.0)
        return 0
    with pytest.raises(_arena.ArenaError, match=r"input pads \+1024.0/0x7F\]: operand 'acc' \(inout\) differs"):
        _arena.run(Case("aliased, reads its own pad", reads_its_own_pad, [In("k", k), InOut("acc", torch.ones(50))]))

    def writes_behind(b):
        good(b)
        _poke(b["acc"], 50)
        return 0
    with pytest.raises(_arena.ArenaError, match=r"operand 'acc' \(inout\): back pad changed \(fill \+0.0\).* offset \+20[0-3] "):
        _arena.run(Case("aliased, writes behind itself", writes_behind, [In("k", k), InOut("acc", torch.ones(50))]))


def test_layout_of_an_arena():
    """The pads are at least 1 MiB and at least one batch element, the data starts on a multiple of 256 bytes, and scratch is
    exactly the bytes asked for."""
    big = In("x", torch.zeros(2, 300000), batch=2)                   # one batch element = 1.2 MB > 1 MiB
    a = _arena.Arena(big, "cpu", _arena._pattern(torch.float32, 1, "cpu"))
    assert a.start >= 1200000 and a.raw.numel() - a.end >= 1200000
    assert a.view().data_ptr() % 256 == 0 and a.view().shape == (2, 300000)
    assert float(a.front().view(torch.float32).min()) == 1024.0 == float(a.back().view(torch.float32).max())
    s = _arena.Arena(Scratch("ws", 1001), "cpu", torch.tensor([_arena.CANARY], dtype=torch.uint8))
    assert s.view().numel() == 1001 and s.start >= (1 << 20) and int(s.raw[s.end]) == _arena.CANARY == int(s.raw[s.start - 1])
    assert bool(torch.isnan(s.extent()[:1000].view(torch.float32)).all())


def test_empty_calls_must_touch_nothing():
    ops = [In("x", torch.zeros(1, 8)), Out("y", (1, 8))]
    _arena.run_noop(Case("noop", lambda b: 0, ops))
    with pytest.raises(_arena.ArenaError, match=r"touches \[empty call\]: operand 'y' was touched.* offset \+0 "):
        _arena.run_noop(Case("touches", lambda b: int(b["y"].zero_().sum()), ops))
    with pytest.raises(_arena.ArenaError, match=r"refuses \[empty call\]: return code -1"):
        _arena.run_noop(Case("refuses", lambda b: -1, ops))
