"""Every entry point against the memory it was handed: the guarded arena and the embedded check (tests only; no GPU import here, CPU
tensors work too).

tests/poison.py puts hostile values INSIDE a batch, in a clip's neighbours.  This file puts them AROUND the tensors of a call: before
the first clip, after the last, between strided rows, behind the scratch and inside every output and scratch byte before the call.  A
result that changes with the fill has read memory it was not handed (a halo or a tile tail multiplied by a 0 / 1 mask: 0 * NaN), or
returns a cell nobody wrote, or read a scratch word before writing it.  A guard word that changes is a write past an output or past the
declared scratch size.  The reference is the call itself on plain tensors: bit equality, no tolerance.

An Arena is one flat int32 buffer holding a fill; a placement is a view into it with GUARD untouched elements on either side.
embedded_check runs a call once on plain tensors and once per fill with every input and output a placement; prefilled does the same for
the Python layer, which allocates inside the library, by standing in for its two allocators."""
import contextlib
import math

import numpy as np
import torch

from tests import poison as P

# Guard on each side of a placement, in elements (never fewer than GUARD 4-byte words).  More than the largest tile any kernel owns,
# 256 frames x 512 channels = 1 << 17 elements: a whole tile of overhang in either direction still lands inside the arena.
GUARD = 1 << 18
FILLS = ("Z", "N", "I", "B")
NAN_WORD = 0x7FC0BEEF  # the quiet NaN the stream tests use as SENTINEL; as int32 a far out-of-range 2143338223
_ALLOCATOR_ALIGN = 512  # what the caching allocator guarantees: prefilled's stand-ins keep it


def _word(value):
    return int(np.array([value], dtype=np.float32).view(np.int32)[0])


def fill_words(fill):
    """The two int32 words a fill alternates (even word, odd word): Z zero bytes, the baseline; N every word 0x7FC0BEEF, a NaN as fp32,
    the same NaN pattern twice as fp64 (which reads as 2.35e307: finite, overflowing at the first product) and a far out-of-range int32; I +inf / -inf; B +-3e38, finite on entry and overflowing inside a kernel."""
    return {"Z": (0, 0), "N": (NAN_WORD, NAN_WORD), "I": (_word(np.inf), _word(-np.inf)), "B": (_word(P.BIG), _word(-P.BIG))}[fill]


class Touched(AssertionError):
    """A word outside every placement's own elements no longer holds the fill."""


class Differs(AssertionError):
    """An output embedded in a fill is not bit for bit the output of the plain call."""


class Placement:
    def __init__(self, name, start, shape, dtype, strides):
        self.name, self.start, self.shape, self.dtype, self.strides = name, start, tuple(shape), dtype, tuple(strides)  # start in bytes


class Arena:
    """Arena(fill, device, words): a flat int32 buffer of `words` words holding `fill`; place() hands out views of it."""

    def __init__(self, fill, device="cpu", words=8 * GUARD):
        even, odd = fill_words(fill)
        self.fill, self.device = fill, torch.device(device)
        words = -(-int(words) // 2) * 2
        self._pair = torch.tensor(np.array([even, odd], dtype=np.int64).astype(np.int32))
        self._pair = self._pair.to(self.device)
        self.buf = self._pair.repeat(words // 2)
        self.used = 0  # bytes handed out so far, guards included
        self.placements = []

    @staticmethod
    def words_for(specs, align=16):
        """Words an arena needs for placements of these (shape, dtype, stride0 or None) specs."""
        total = 0
        for shape, dtype, stride0 in specs:
            item = _item(dtype)
            total += 2 * GUARD * max(item, 4) + _span(shape, stride0) * item + 2 * max(align, 16) + 16
        return total // 4 + 8

    def room(self, nbytes, itemsize=1, align=16):
        start = self.used + GUARD * max(itemsize, 4) + align
        return start + itemsize + nbytes + GUARD * max(itemsize, 4) <= self.buf.numel() * 4

    def place(self, shape, dtype=torch.float32, stride0=None, offset=0, align=16, name=None):
        """A view of `shape` and `dtype` that starts GUARD elements after the previous placement's end (or the arena's start), on an
        `align`-byte boundary shifted by `offset` elements, with GUARD more elements behind it.  stride0: elements between the
        slices of axis 0 (default: dense); the gap belongs to the guard.  The view's own elements still hold the fill."""
        shape = tuple(int(s) for s in shape)
        item = _item(dtype)
        guard = GUARD * max(item, 4)
        inner = int(math.prod(shape[1:])) if len(shape) > 1 else 1
        stride0 = inner if stride0 is None else int(stride0)
        assert stride0 >= inner and align % item == 0 and align % 4 == 0
        base = self.buf.data_ptr()
        start = -(-(base + self.used + guard) // align) * align - base + int(offset) * item
        span = _span(shape, stride0) * item
        end = start + span
        assert end + guard <= self.buf.numel() * 4, f"arena of {self.buf.numel()} words is full"
        self.used = end
        strides = [1] * len(shape)
        for d in range(len(shape) - 2, -1, -1):
            strides[d] = strides[d + 1] * shape[d + 1]
        if shape:
            strides[0] = stride0
        p = Placement(name or f"placement {len(self.placements)}", start, shape, dtype, strides)
        self.placements.append(p)
        return self._view(self.buf, p)

    def _view(self, buf, p):
        item = _item(p.dtype)
        span = _span(p.shape, p.strides[0] if p.shape else 1) * item
        flat = buf.view(torch.uint8)[p.start:p.start + span].view(p.dtype)
        return flat.as_strided(p.shape, p.strides) if span else flat.reshape(p.shape)

    def put(self, t, stride0=None, offset=0, align=16, name=None):
        """A placement holding a copy of `t`."""
        v = self.place(t.shape, t.dtype, stride0, offset, align, name)
        v.copy_(t)
        return v

    def intact(self, what=""):
        """Raises Touched unless every word outside the placements' own elements — guards and stride gaps alike — still holds the fill;
        names the placement nearest the damage and the first and last changed offset, in its elements, relative to its start."""
        expected = self._pair.repeat(self.buf.numel() // 2)
        own = torch.zeros(self.buf.numel() * 4, dtype=torch.uint8, device=self.device)
        for p in self.placements:
            if math.prod(p.shape):
                _mark(own, p, _item(p.dtype))
        bad = (self.buf.view(torch.uint8) != expected.view(torch.uint8)) & (own == 0)
        if not bool(bad.any()):
            return True
        where = torch.nonzero(bad).reshape(-1)
        first, last = int(where[0]), int(where[-1])
        near = min(self.placements, key=lambda p: min(abs(first - p.start), abs(first - self._end(p)))) if self.placements else None
        if near is None:
            raise Touched(f"{what} fill {self.fill}: {where.numel()} bytes changed, the first at byte {first}; the arena has no placement")
        item = _item(near.dtype)
        lo, hi = (first - near.start) / item, (last - near.start) / item
        size = _span(near.shape, near.strides[0] if near.shape else 1)
        side = "before it" if first < near.start else ("behind it" if first >= self._end(near) else "in a stride gap")
        raise Touched(f"{what} fill {self.fill}: {where.numel()} bytes outside every placement changed; nearest is {near.name} "
                      f"{near.shape} (spans {size} elements): first changed offset {lo:g}, last {hi:g} elements from its start ({side})")

    def _end(self, p):
        return p.start + _span(p.shape, p.strides[0] if p.shape else 1) * _item(p.dtype)


def _item(dtype):
    return torch.tensor([], dtype=dtype).element_size()


def _span(shape, stride0):
    """Elements from a placement's first to one past its last (stride gaps inside included, none behind the last slice)."""
    shape = tuple(shape)
    if not shape:
        return 1
    if math.prod(shape) == 0:
        return 0
    inner = int(math.prod(shape[1:])) if len(shape) > 1 else 1
    stride0 = inner if stride0 is None else int(stride0)
    return (shape[0] - 1) * stride0 + inner


def _mark(own, p, item):
    span = _span(p.shape, p.strides[0] if p.shape else 1)
    cells = own[p.start:p.start + span * item].view(-1, item)  # [element][byte]
    cells.as_strided(p.shape + (item,), tuple(s * item for s in p.strides) + (1,)).fill_(1)


def _plain(shape, dtype, stride0, device):
    """A tensor of its own, zeroed, with the row stride asked for (a call is told its strides: the plain run keeps them)"""
    shape = tuple(int(n) for n in shape)
    if stride0 is None or not shape:
        return torch.zeros(shape, dtype=dtype, device=device)
    inner = [int(math.prod(shape[d + 1:])) for d in range(1, len(shape))]
    return torch.zeros(max(_span(shape, stride0), 1), dtype=dtype, device=device).as_strided(shape, [int(stride0)] + inner)


def _tensors(result):
    outs = P._as_outputs(result)
    flat = []
    for name, v in outs:
        if isinstance(v, torch.Tensor):
            flat.append((name, v))
        else:
            flat += [(f"{name}[{i}]", t) for i, t in enumerate(v)]
    return flat


def same_bits(ref, got, what):
    """Raises Differs unless every tensor of `got` is, bit for bit (NaN == NaN, -0 != +0), the tensor of `ref` with the same name."""
    a, b = _tensors(ref), _tensors(got)
    assert a, f"{what}: the call returned no tensor"
    assert [n for n, _ in a] == [n for n, _ in b], f"{what}: the runs' outputs differ in kind"
    for (name, x), (_, y) in zip(a, b):
        if x.shape != y.shape or x.dtype != y.dtype:
            raise Differs(f"{what} {name}: {tuple(y.shape)} {y.dtype} where the plain call gave {tuple(x.shape)} {x.dtype}")
        bx, by = P._bits(x), P._bits(y)
        if not np.array_equal(bx, by):
            diff = np.argwhere(np.atleast_1d(bx != by))
            raise Differs(f"{what} {name}: {len(diff)} of {bx.size} words differ from the plain call, the first at {tuple(int(i) for i in diff[0])}, "
                          f"the last at {tuple(int(i) for i in diff[-1])}{'' if P._finite(y) else '; the result is not finite'}")


def embedded_check(call, inputs, out_specs, what="", fills=FILLS, device=None):
    """call(*inputs, *outputs) writes its outputs and returns None, or returns the tensors to compare (views of the outputs, or more).

    inputs: tensors, or dicts {"t": tensor, "stride0": .., "offset": .., "inout": bool}; inout: the call also writes this placement (an
    in-place call), so it counts as an output and is compared.  out_specs: (shape, dtype) or dicts {"shape", "dtype", "stride0",
    "offset", "scratch": bool}; scratch: placed, filled and guarded like an output but not compared.  Runs the call once on plain tensors (of their own, with the same row strides, outputs zeroed): the reference is the entry point itself.  Then once per
    fill with every input copied into a placement of that fill's arena and every output a placement still holding the fill; every output
    must be bit for bit the reference's (where a stride leaves gaps: its own elements) and the arena intact()."""
    ins = [i if isinstance(i, dict) else {"t": i} for i in inputs]
    outs = [o if isinstance(o, dict) else {"shape": o[0], "dtype": o[1]} for o in out_specs]
    device = device or ins[0]["t"].device

    def collect(args_in, args_out, returned):
        res = {f"out{k}": o for k, (o, spec) in enumerate(zip(args_out, outs)) if not spec.get("scratch")}
        res.update({f"inout{k}": a for k, (a, i) in enumerate(zip(args_in, ins)) if i.get("inout")})
        if returned is not None:
            res["returned"] = returned
        return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}

    plain_in = [_plain(i["t"].shape, i["t"].dtype, i.get("stride0"), device).copy_(i["t"]) for i in ins]
    plain_out = [_plain(o["shape"], o["dtype"], o.get("stride0"), device) for o in outs]
    ref = collect(plain_in, plain_out, call(*plain_in, *plain_out))
    specs = [(i["t"].shape, i["t"].dtype, i.get("stride0")) for i in ins] + [(o["shape"], o["dtype"], o.get("stride0")) for o in outs]
    for fill in fills:
        arena = Arena(fill, device, Arena.words_for(specs))
        a_in = [arena.put(i["t"], i.get("stride0"), i.get("offset", 0), name=f"input {k}") for k, i in enumerate(ins)]
        a_out = [arena.place(o["shape"], o["dtype"], o.get("stride0"), o.get("offset", 0), name=f"output {k}") for k, o in enumerate(outs)]
        got = collect(a_in, a_out, call(*a_in, *a_out))
        same_bits(ref, got, f"{what} fill {fill}")
        arena.intact(f"{what}")
    return ref


class Prefilled:
    """What prefilled() yields: the arenas its stand-ins allocated from, and view() for the call's own inputs."""

    def __init__(self, fill, words):
        self.fill, self.words, self.arenas = fill, words, []

    def _arena(self, device, nbytes, item, align):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        for a in self.arenas:
            if a.device == device and a.room(nbytes, item, align):
                return a
        need = (2 * GUARD * max(item, 4) + nbytes + 2 * align) // 4 + 64
        self.arenas.append(Arena(self.fill, device, max(self.words, need)))
        return self.arenas[-1]

    def alloc(self, shape, dtype, device, name):
        item = _item(dtype)
        a = self._arena(device, int(math.prod(shape)) * item, item, _ALLOCATOR_ALIGN)
        return a.place(shape, dtype, align=_ALLOCATOR_ALIGN, name=name)  # holds the fill; exactly these bytes, a guard behind them

    def view(self, t, stride0=None, offset=0):
        """An input of the call: a copy of `t` in an arena of the same fill."""
        item = t.element_size()
        a = self._arena(t.device, _span(t.shape, stride0) * item + 16 + item, item, 16)
        return a.put(t, stride0, offset, name=f"input {tuple(t.shape)}")

    def intact(self, what=""):
        for a in self.arenas:
            a.intact(what)


@contextlib.contextmanager
def prefilled(fill, monkeypatch, words=16 * GUARD):
    """For the Python-layer entry points, which allocate inside the library: l3ac_amd._metric.scratch (mel_scratch resolves it at call
    time, so the one patch covers both) and torch.empty for CUDA allocations return placements of arenas holding `fill`.  A scratch
    placement is exactly the requested number of bytes with a guard behind it.  Everything is restored on the way out."""
    from l3ac_amd import _metric
    state = Prefilled(fill, words)
    real_empty, real_scratch = torch.empty, _metric.scratch
    sizing = []  # non-empty while the real scratch() runs only to tell us the size it would allocate

    def empty(*size, **kw):
        device = kw.get("device")
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        if sizing:
            sizing.append(tuple(int(n) for n in shape))
            return real_empty(0, dtype=dtype)
        if device is None or torch.device(device).type != "cuda" or kw.get("out") is not None or kw.get("pin_memory"):
            return real_empty(*size, **kw)
        shape = tuple(int(n) for n in shape)
        return state.alloc(shape, dtype, device, f"torch.empty({shape}, {dtype})")

    def scratch(dev, need, extra_scratch=0, rows=0, row_floats=0):
        sizing.append("asked")
        try:
            real_scratch(dev, need, extra_scratch, rows, row_floats)
            (nbytes,), = sizing[1:]
        finally:
            sizing.clear()
        return state.alloc((nbytes,), torch.uint8, dev, f"scratch of {nbytes} bytes")

    with monkeypatch.context() as m:  # (undone in the context's own finally, whatever the block raises)
        m.setattr(torch, "empty", empty)
        m.setattr(_metric, "scratch", scratch)
        yield state
