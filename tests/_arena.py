"""Guard-band harness: every operand of a C-ABI call is a typed view into the middle of a larger byte tensor (its arena),
so a kernel that reads or writes outside its buffers is caught instead of going unnoticed (or faulting).

    case = Case("name", call, [In("x", x, batch=B), Out("y", shape, torch.float32, batch=B), Scratch("ws", nbytes)])
    run(case, device)

`call(bufs)` receives a dict name -> tensor and returns the entry point's return code.  run() makes the call once on plain
allocations and once per pad fill on arenas, and asserts

  1. every out / inout extent of an arena run equals the plain run, byte for byte,
  2. the pads of every out / scratch operand still hold the canary byte 0xA5,
  3. the pads of every in / inout operand still hold their fill (an aliased operand is read too: a halo load outside it must
     change the result between two fills),
  4. every in extent still holds what went in,
  5. the return code is 0,
  6. every out operand was written at all (a call that does nothing agrees with itself).

The pads of what a call reads hold a FINITE poison (0.0, +1024.0, -1024.0 as the operand's float type; the bytes 0x00, 0x7F, 0x80 for integer
operands): a NaN would be swallowed by a ReLU compiled with -fno-honor-nans, a stray value that meets a zero weight must stay
harmless, and 1024 is exact and far above every tolerance, so a read of a pad changes the output between two fills.
Scratch is exactly the bytes asked for, NaN inside.  Plain Python on torch tensors: works on CPU and on the GPU; all
comparisons run on the tensors' device.
"""
import torch

CANARY = 0xA5
ALIGN = 256                      # what any HIP allocator returns; the header promises no more
MIN_PAD = 1 << 20
FLOAT_FILLS = (0.0, 1024.0, -1024.0)
BYTE_FILLS = (0x00, 0x7F, 0x80)


class ArenaError(AssertionError):
    pass


def _up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Operand(object):
    """name; role in {"in", "out", "inout", "scratch"}; data (in / inout) or shape + dtype (out) or nbytes (scratch);
    batch = number of batch elements the operand holds: the pads are at least one of them (and at least 1 MiB), so a store that
    is off by a whole cube still lands in a pad.  None: the operand has no batch axis (weights, scratch)."""

    def __init__(self, name, role, data=None, shape=None, dtype=None, batch=None):
        assert role in ("in", "out", "inout", "scratch")
        self.name, self.role = name, role
        if data is not None:
            data = data.contiguous()
            shape, dtype = tuple(data.shape), data.dtype
        self.data, self.shape, self.dtype = data, tuple(int(s) for s in shape), dtype
        self.nbytes = _numel(self.shape) * _itemsize(dtype)
        self.pad = _up(max(MIN_PAD, self.nbytes // max(1, int(batch)) if batch else 0))


def In(name, data, batch=None):
    return Operand(name, "in", data=data, batch=batch)


def InOut(name, data, batch=None):
    return Operand(name, "inout", data=data, batch=batch)


def Out(name, shape, dtype=torch.float32, batch=None):
    return Operand(name, "out", shape=shape, dtype=dtype, batch=batch)


def Scratch(name, nbytes):
    return Operand(name, "scratch", shape=(int(nbytes),), dtype=torch.uint8)


class Case(object):
    def __init__(self, name, call, operands):
        self.name, self.call, self.operands = name, call, list(operands)
        assert len({o.name for o in self.operands}) == len(self.operands), "operand names must differ"

    def __repr__(self):
        return self.name


def _pattern(dtype, fill_index, device):
    """The bytes of one element of the pad fill number `fill_index` for an in operand of type dtype."""
    if dtype.is_floating_point:
        return torch.tensor([FLOAT_FILLS[fill_index]], dtype=dtype).view(torch.uint8).to(device)
    return torch.full((_itemsize(dtype),), BYTE_FILLS[fill_index], dtype=torch.uint8).to(device)


def _fill_name(dtype, fill_index):
    return ("%+.1f" % FLOAT_FILLS[fill_index]) if dtype.is_floating_point else ("0x%02X" % BYTE_FILLS[fill_index])


def _nan_fill(buf):
    """float32 NaN in every whole word of a byte tensor (0xFF in what is left): NaN as any float type's word too."""
    buf.fill_(0xFF)


class Arena(object):
    """One operand inside its arena: front pad | extent | back pad, the extent 256-byte aligned."""

    def __init__(self, op, device, pattern):
        self.op = op
        item = _itemsize(op.dtype)
        total = op.pad + ALIGN + _up(op.nbytes) + op.pad
        self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        self.start = _up(base + op.pad) - base
        self.end = self.start + op.nbytes
        assert (base + self.start) % ALIGN == 0 and self.start >= op.pad and total - self.end >= op.pad
        assert self.start % item == 0
        back = (total - self.end) // len(pattern) * len(pattern)       # whole elements of the fill
        self.stop = self.end + back
        self.pattern = pattern
        self.front().view(-1, len(pattern)).copy_(pattern.expand(self.start // len(pattern), len(pattern)))
        self.back().view(-1, len(pattern)).copy_(pattern.expand(back // len(pattern), len(pattern)))
        ext = self.extent()
        if op.role in ("in", "inout"):
            ext.copy_(op.data.reshape(-1).view(torch.uint8).to(device))
        elif op.role == "out":
            ext.fill_(CANARY)
        else:
            _nan_fill(ext)

    def front(self):
        return self.raw[:self.start]

    def back(self):
        return self.raw[self.end:self.stop]

    def extent(self):
        return self.raw[self.start:self.end]

    def view(self):
        return self.extent().view(self.op.dtype).view(self.op.shape)


def _first_diff(a, b):
    return int((a != b).nonzero()[0, 0])


def _check_pad(case, arena, what, run_name):
    for side, pad in (("front", arena.front()), ("back", arena.back())):
        n = len(arena.pattern)
        want = arena.pattern.expand(pad.numel() // n, n)
        if torch.equal(pad.view(-1, n), want):
            continue
        at = _first_diff(pad.view(-1, n), want.contiguous()) * n
        at += int((pad[at:at + n] != arena.pattern).nonzero()[0, 0])
        rel = at - pad.numel() if side == "front" else arena.op.nbytes + at
        raise ArenaError("%s [%s]: operand '%s' (%s): %s pad changed (%s), first changed byte at offset %+d relative to the "
                         "extent of %d bytes" % (case.name, run_name, arena.op.name, arena.op.role, side, what, rel, arena.op.nbytes))


def _plain(op, device):
    if op.role in ("in", "inout"):
        return op.data.to(device).clone()
    t = torch.empty(max(op.nbytes, 0), dtype=torch.uint8, device=device)
    if op.role == "out":
        t.fill_(CANARY)
        return t.view(op.dtype).view(op.shape)
    _nan_fill(t)
    return t


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def run(case, device="cpu", fills=(0, 1, 2)):
    """The checked call.  Returns the plain run's buffers (name -> tensor) so a caller may go on to compare them with a reference."""
    plain = {op.name: _plain(op, device) for op in case.operands}
    rc = case.call(plain)
    _sync(device)
    if rc != 0:
        raise ArenaError("%s [plain allocations]: return code %r" % (case.name, rc))
    for op in case.operands:                  # a call that quietly did nothing would agree with itself in every run
        if op.role == "out" and op.nbytes and bool((plain[op.name].reshape(-1).view(torch.uint8) == CANARY).all()):
            raise ArenaError("%s [plain allocations]: operand '%s' (out) was never written: it still holds the canary" % (case.name, op.name))
    canary = torch.full((1,), CANARY, dtype=torch.uint8, device=device)
    for fi in fills:
        arenas = {}
        for op in case.operands:
            pat = _pattern(op.dtype, fi, device) if op.role in ("in", "inout") else canary      # whatever the call READS
            arenas[op.name] = Arena(op, device, pat)
        run_name = "arenas, input pads " + "/".join(sorted({_fill_name(op.dtype, fi) for op in case.operands if op.role in ("in", "inout")}) or ["-"])
        rc = case.call({k: a.view() for k, a in arenas.items()})
        _sync(device)
        if rc != 0:
            raise ArenaError("%s [%s]: return code %r" % (case.name, run_name, rc))
        for op in case.operands:
            a = arenas[op.name]
            _check_pad(case, a, "fill %s" % _fill_name(op.dtype, fi) if op.role in ("in", "inout") else "canary 0x%02X" % CANARY, run_name)
            if op.role == "in":
                want = op.data.reshape(-1).view(torch.uint8).to(device)
                if not torch.equal(a.extent(), want):
                    raise ArenaError("%s [%s]: operand '%s' (in) was modified, first changed byte at offset %+d relative to the extent"
                                     % (case.name, run_name, op.name, _first_diff(a.extent(), want)))
            elif op.role in ("out", "inout"):
                want = plain[op.name].reshape(-1).view(torch.uint8)
                if not torch.equal(a.extent(), want):
                    raise ArenaError("%s [%s]: operand '%s' (%s) differs from the run on plain allocations, first differing byte at "
                                     "offset %+d relative to the extent (a result that depends on memory outside the operands)"
                                     % (case.name, run_name, op.name, op.role, _first_diff(a.extent(), want)))
    return plain


def run_noop(case, device="cpu"):
    """An empty call (B = 0 / n = 0 / rows = 0): every operand, whatever its role, is an arena that holds the canary in pads
    AND extent; the call must return 0 and change none of it."""
    canary = torch.full((1,), CANARY, dtype=torch.uint8, device=device)
    arenas = {}
    for op in case.operands:
        a = arenas[op.name] = Arena(op, device, canary)
        a.extent().fill_(CANARY)
    rc = case.call({k: a.view() for k, a in arenas.items()})
    _sync(device)
    if rc != 0:
        raise ArenaError("%s [empty call]: return code %r" % (case.name, rc))
    for op in case.operands:
        a = arenas[op.name]
        _check_pad(case, a, "canary 0x%02X" % CANARY, "empty call")
        if not bool((a.extent() == CANARY).all()):
            raise ArenaError("%s [empty call]: operand '%s' was touched, first changed byte at offset %+d relative to the extent"
                             % (case.name, op.name, _first_diff(a.extent(), torch.full_like(a.extent(), CANARY))))
