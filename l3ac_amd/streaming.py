"""Streaming sessions: live audio in, the chunker's bits out.

Geometry first, as pure functions of host integers (no tensors, no GPU): a stream of frames arrives in pushes of any size and is cut
with a step of ``step`` frames and a look-back of ``lookback`` frames.  Chunk k covers ``[max(0, k * step - lookback),
min(n', (k + 1) * step))`` and emits what lies at or after ``k * step``; ``n'`` is the stream's length rounded up to ``round_to``
(audio: the hop, the zero padding of ``Network.preprocess``).  For ``lookback < step`` that is ``ChunkData``'s / ``l3ac_chunk_plan``'s
geometry; for ``lookback >= step`` — a short step with the attention's whole window behind it, which the offline chunker refuses — the
look-back grows over the first ``ceil(lookback / step)`` chunks until it is full.

Then the sessions, ``StreamEncoder`` / ``StreamDecoder`` (``L3AC.stream_encoder`` / ``L3AC.stream_decoder``): the state carried
between pushes lives in one device buffer per session, moved by the kernels of csrc/kernels/stream.hip; every chunk runs as a row of
the ragged calls, so its bits are those of ``encode_audio`` / ``decode_audio`` on that chunk alone.

Last, streaming sample-rate conversion: its geometry (``resample_advance``) and ``StreamResampler``
(``l3ac_amd.stream_resampler``), whose carried state is each stream's last inputs; one launch of csrc/kernels/resample_stream.hip per push.
The bookkeeping of streaming IIR filtering (``filter_advance``) is here too; its session, ``StreamFilter``, is in
filtering.py.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _capi
from ._rows import (check_codec_input, contiguous_rows, decode_rows, encode_rows, end_flags, int_list, refuse_grn_exact, row_stride, validated,
                    window_args)
from .resampling import _resample_bank


# ---- 1. geometry -------------------------------------------------------------------------------------------------------------
class StreamState(NamedTuple):
    """What one stream holds between pushes: ``context`` frames of look-back followed directly by ``pending`` frames that have not
    completed a chunk yet (``held = context + pending`` frames, one contiguous piece of the stream), and the frames seen so far."""
    context: int = 0
    pending: int = 0
    seen: int = 0

    @property
    def held(self) -> int:
        return self.context + self.pending


class StreamRow(NamedTuple):
    """One completed chunk.  (start, frames, prefix, pad) are ``l3ac_chunk_desc``'s fields: the chunk's first frame in its stream,
    its frames (look-back and zero padding included), the look-back frames its emission drops, the zero frames at its end.  The row is
    ``state[0:held] ++ new[off:off + take] ++ zeros(pad)``; afterwards the stream keeps the row's last ``keep`` real frames."""
    start: int
    frames: int
    prefix: int
    pad: int
    held: int
    off: int
    take: int
    keep: int


def check_geometry(step: int, lookback: int, round_to: int = 1) -> None:
    if round_to < 1 or step < round_to or step % round_to or lookback < 0 or lookback % round_to:
        raise ValueError(f"a step of {step} and a look-back of {lookback} frames must be whole multiples of {round_to}, the step at least one")


def advance(state: StreamState, new_frames: int, end: bool, step: int, lookback: int, round_to: int = 1) -> Tuple[List[StreamRow], StreamState]:
    """One push of ``new_frames`` frames onto a stream in ``state``: the chunks it completes, in order, and the state afterwards.
    ``end``: the stream ends with this push; what is pending is flushed as its last chunk, padded with zeros to a multiple of
    ``round_to``, and the state afterwards is a fresh stream's."""
    check_geometry(step, lookback, round_to)
    if new_frames < 0:
        raise ValueError(f"{new_frames} new frames")
    context, pending, seen = state
    rows: List[StreamRow] = []
    off = 0
    while pending + (new_frames - off) >= step:
        take = step - pending
        frames = context + step
        keep = min(lookback, frames)
        rows.append(StreamRow(seen - pending - context, frames, context, 0, context + pending, off, take, keep))
        seen += take
        off += take
        context, pending = keep, 0
    rest = new_frames - off
    if not end:
        return rows, StreamState(context, pending + rest, seen + rest)
    if pending + rest > 0:
        pad = -(pending + rest) % round_to
        rows.append(StreamRow(seen - pending - context, context + pending + rest + pad, context, pad, context + pending, off, rest, 0))
    return rows, StreamState()


def leftover(rows: Sequence[StreamRow], after: StreamState, new_frames: int) -> Optional[Tuple[int, int, int]]:
    """(held, off, take) of the append that follows a push's last chunk: ``new[off:off + take]`` goes behind the ``held`` frames the
    stream holds by then; None when the push leaves nothing over (always when it ended the stream)."""
    off = sum(r.take for r in rows)
    take = new_frames - off
    if take <= 0 or after.held == 0:
        return None
    return after.held - take, off, take


def emitted(seen: int, ended: bool, step: int, round_to: int = 1) -> int:
    """Frames' worth of output (in units of ``round_to`` frames: tokens) a stream has emitted after ``seen`` frames."""
    return -(-seen // round_to) if ended else seen // step * (step // round_to)


def round4(n: int) -> int:
    return -(-n // 4) * 4


# ---- 1b. streaming sample-rate conversion: geometry ----------------------------------------------------------
class ResampleGeometry(NamedTuple):
    """``resample``'s plan for a rate pair: up / down = target / orig reduced, half_len = 10 max(up, down), K taps per output.  Output m reads
    inputs ``i(m) - (K - 1) .. i(m)``, ``i(m) = (m * down + half_len) // up``, with the taps of phase ``(m * down + half_len) % up``."""
    up: int
    down: int
    half_len: int
    K: int

    def newest(self, m: int) -> int:
        return (m * self.down + self.half_len) // self.up

    def length(self, n_in: int) -> int:
        """``resample_length``: ceil(n_in * up / down)."""
        return -(-n_in * self.up // self.down)


def resample_geometry(orig_sr: int, target_sr: int) -> ResampleGeometry:
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if orig_sr < 1 or target_sr < 1:
        raise ValueError(f"resample: rates must be positive (got {orig_sr} -> {target_sr})")
    g = math.gcd(orig_sr, target_sr)
    up, down = target_sr // g, orig_sr // g
    half_len = 10 * max(up, down)
    return ResampleGeometry(up, down, half_len, -(-(2 * half_len + 1) // up))


class ResampleState(NamedTuple):
    """What one converted stream is between pushes: its last ``held`` inputs are on the device; ``seen`` inputs received, ``emitted`` outputs
    produced so far (Python ints: they never reach the device)."""
    held: int = 0
    seen: int = 0
    emitted: int = 0


class ResamplePush(NamedTuple):
    """One stream's share of one push, l3ac_resample_stream_desc's fields: the stream's input is ``state[0:held] ++ new[0:take] ++ zeros``,
    output j of the push has ``q = q0 + j * down`` (newest input at row position ``q // up``, phase ``q % up``), ``count`` outputs are
    emitted, and the stream keeps the last ``keep`` of its held + take inputs."""
    q0: int
    count: int
    held: int
    take: int
    keep: int


def resample_advance(state: ResampleState, new_frames: int, end: bool, geo: ResampleGeometry) -> Tuple[ResamplePush, ResampleState]:
    """One push of ``new_frames`` inputs onto a stream in ``state``.  Not ended: the outputs whose newest input exists by now are emitted
    (they lag the input by half_len / up input samples).  ``end``: inputs past the end count as zeros, as in ``resample``; the outputs up to
    ``ceil(seen * up / down)`` are emitted and the state afterwards is a fresh stream's.  Equal rates pass the inputs through at once."""
    if new_frames < 0:
        raise ValueError(f"{new_frames} new frames")
    up, down, half_len, K = geo
    held, seen, done = state
    now = seen + new_frames
    q0 = done * down + half_len - (seen - held) * up
    if up == down:
        count, keep = new_frames, 0
    elif end:
        count, keep = geo.length(now) - done, 0
    else:
        upto = max(0, -(-(now * up - half_len) // down))
        count = upto - done
        keep = now - max(0, geo.newest(upto) - (K - 1))
    push = ResamplePush(q0, count, held, new_frames, keep)
    return push, (ResampleState() if end else ResampleState(keep, now, done + count))


# ---- 1c. streaming IIR filtering: bookkeeping ------------------------------------------------------------------
FILTER_SEGMENT = 256  # l3ac_sosfilt_segment(): the segment of the parallel recursion, anchored at a stream's first sample


class FilterState(NamedTuple):
    """What one filtered stream is between pushes on the host: ``k`` samples into its current segment (its position modulo the segment;
    the start pair of that segment and both running states are on the device) and ``seen`` samples received so far."""
    k: int = 0
    seen: int = 0


class FilterPush(NamedTuple):
    """One stream's share of one push, l3ac_sosfilt_stream_desc's fields: the stream's current segment has had ``k`` samples, the push
    brings ``take`` more and emits ``count`` = ``take`` outputs; ``end``: the slot is at rest afterwards; ``fresh``: the stream has
    received nothing yet, so the push starts from rest and reads nothing of what the slot holds on the device (``reset`` relies on it)."""
    k: int
    take: int
    count: int
    end: bool
    fresh: bool


def filter_advance(state: FilterState, new_frames: int, end: bool, segment: int = FILTER_SEGMENT) -> Tuple[FilterPush, FilterState]:
    """One push of ``new_frames`` samples onto a stream in ``state``: as many outputs as inputs, at once (no latency, nothing to flush).
    ``end`` only returns the slot to rest."""
    if new_frames < 0:
        raise ValueError(f"{new_frames} new frames")
    k, seen = state
    push = FilterPush(k, new_frames, new_frames, bool(end), seen == 0)
    return push, (FilterState() if end else FilterState((k + new_frames) % segment, seen + new_frames))


# ---- 2. sessions -------------------------------------------------------------------------------------------------------------
class _Streams:
    """What all six sessions share: the per-stream host state and the parsing of a push's ``lengths`` / ``end``."""
    _fresh = None  # the state of a fresh stream

    def __init__(self, streams: int):
        if isinstance(streams, bool) or int(streams) != streams or int(streams) < 1:
            raise ValueError(f"streams must be a positive integer, got {streams!r}")
        self.streams = int(streams)
        self._states = [self._fresh] * self.streams

    @property
    def states(self) -> list:
        """The streams' host state (a copy), one tuple of the session's state type each (``StreamState``, ``ResampleState``,
        ``wire.PackState`` / ``UnpackState``): what the stream holds on the device and what it has seen and emitted since it began."""
        return list(self._states)

    def reset(self, streams=None) -> None:
        """Make the given streams (an index, a sequence of them; absent: all) fresh: what they hold is dropped, nothing is emitted."""
        which = range(self.streams) if streams is None else [streams] if isinstance(streams, int) else list(streams)
        which = [int(i) for i in which]
        bad = [i for i in which if not 0 <= i < self.streams]
        if bad:
            raise ValueError(f"stream {bad[0]} of {self.streams}")
        for i in which:
            self._states[i] = self._fresh

    def _lengths(self, lengths, n: int, what: str) -> List[int]:
        return [n] * self.streams if lengths is None else int_list(lengths, self.streams, 0, n, what, f"{self.streams} streams")

    def _ends(self, end) -> List[bool]:
        return end_flags(end, self.streams)


class _CarrySession(_Streams):
    """The sessions of one launch per push (StreamResampler, wire.StreamPacker / StreamUnpacker, filtering.StreamFilter): the carried state lives on the device of
    the first push, in two buffers read and written alternately.  A push cannot be captured: ``_phase`` names the host value that moves."""
    _what = "session"
    _elements = "elements"
    _phase = ""

    def __init__(self, streams: int):
        super().__init__(streams)
        self._lib = _capi.load_library()
        self._device = None
        self._bufs = None  # allocated at the first push

    def _check_device(self, t: torch.Tensor, what: str) -> None:
        if not t.is_cuda:
            raise RuntimeError(f"{self._what}: {what} is on {t.device}: l3ac_amd has no CPU path")
        if self._device is not None and t.device != self._device:
            raise RuntimeError(f"{self._what}: {what} is on {t.device} but the session's state is on {self._device}")
        if t.shape[1] >= 2 ** 31:
            raise ValueError(f"{self._what}: a push of {t.shape[1]} {self._elements}")
        with torch.cuda.device(t.device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._what}: a push cannot be captured into a graph: {self._phase} is a host value that "
                                   "advances with every push")

    def _take(self, new: torch.Tensor, what: str, dtype, lengths, lengths_what: str, end, advance, *geometry):
        """The host half of a push of (S, n) ``new``: every check, then ``advance(state, lengths[i], end[i], *geometry)`` per stream ->
        (new as ``dtype`` with unit-stride rows, the plan [(push, state afterwards)], the outputs per stream, their maximum)."""
        lens = self._lengths(lengths, new.shape[1], lengths_what)
        ends = self._ends(end)
        self._check_device(new, what)
        plan = [advance(st, m, e, *geometry) for st, m, e in zip(self._states, lens, ends)]
        total = [p.count for p, _ in plan]
        return contiguous_rows(new.to(dtype)), plan, total, max(total)

    def _buffers(self, dev, shape, dtype):
        """(read, written) pointers of the two state buffers, zeroed on ``dev`` at the first push; ``shape`` None: a session without any."""
        if self._device is None:
            self._device = dev
            self._bufs = shape and [torch.zeros(shape, dtype=dtype, device=dev) for _ in range(2)]
        return (self._bufs[0].data_ptr(), self._bufs[1].data_ptr()) if self._bufs else (None, None)

    def _commit(self, plan) -> None:
        """After the launch: what was written is what the next push reads, and every stream is in its state afterwards."""
        if self._bufs:
            self._bufs.reverse()
        self._states = [after for _, after in plan]


class _PushPlan(NamedTuple):
    rows: list       # (slot, round, StreamRow), in row order of the whole push: shortest first
    groups: list     # lists of indices into rows: one ragged call each
    appends: list    # (slot, held, off, take)
    after: list      # StreamState per slot
    rounds: int


def _stream_window(hop: int, process_window, prefix_tokens):
    """``window_args``' geometry for a session: a step of at least one hop and any look-back, at, above or below it."""
    if int(process_window) != process_window or int(process_window) < hop:
        raise ValueError(f"process_window ({process_window} samples) must be at least one hop ({hop} samples)")
    if int(prefix_tokens) != prefix_tokens or int(prefix_tokens) < 0:
        raise ValueError(f"prefix_tokens must be a non-negative integer, got {prefix_tokens!r}")
    return int(process_window) // hop * hop, int(prefix_tokens) * hop


class _Session(_Streams):
    """What StreamEncoder and StreamDecoder share: the per-stream host state, the device state buffer and the kernels that move it."""
    _what = "stream"
    _fresh = StreamState()

    def __init__(self, codec, streams: int, process_window: int, prefix_tokens: Optional[int], chunks_per_call: Optional[int], in_tokens: bool):
        super().__init__(streams)
        hop = codec.network.mc.hop_length
        chunk_len, self.prefix_tokens, self.chunks_per_call = window_args(codec.network.mc, codec.config.sample_rate, process_window,
                                                                          prefix_tokens, chunks_per_call, _stream_window)
        self.codec = codec
        self.hop = hop
        self.step_tokens = chunk_len // hop
        unit = 1 if in_tokens else hop  # frames per token on the input side
        self.round_to = unit
        self.step = self.step_tokens * unit
        self.lookback = self.prefix_tokens * unit
        check_geometry(self.step, self.lookback, self.round_to)
        self.state_frames = round4(self.lookback + self.step)
        self._ctx = codec.network.context()  # raises when the network is not on a GPU
        self._device = codec.network.device
        self._lib = _capi.load_library()
        self._buf, self._c = None, 0  # [streams][state_frames][c], allocated at the first push (a decoder learns c there)

    # ---- host side ------------------------------------------------------------------------------------------------------
    def _check_network(self, t, what: str) -> None:
        check_codec_input(self.codec.network, self._ctx, t, what, self._what)
        refuse_grn_exact(self.codec.network, self._what, self._offline)

    def _plan(self, lens: List[int], ends: List[bool]) -> _PushPlan:
        per, after, appends = [], [], []
        for i in range(self.streams):
            rows, st = advance(self._states[i], lens[i], ends[i], self.step, self.lookback, self.round_to)
            tail = leftover(rows, st, lens[i])
            if tail is not None:
                appends.append((i,) + tail)
            per.append(rows)
            after.append(st)
        flat = [(i, j, r) for i, rows in enumerate(per) for j, r in enumerate(rows)]
        flat.sort(key=lambda e: e[2].frames)  # shortest first (stable), as encode_long groups its chunks
        groups = [list(range(k0, min(k0 + self.chunks_per_call, len(flat)))) for k0 in range(0, len(flat), self.chunks_per_call)]
        return _PushPlan(flat, groups, appends, after, max([len(rows) for rows in per] + [0]))

    def _steady(self, lens: List[int], ends: List[bool]) -> Optional[str]:
        """None when this push is steady (capturable), else the condition it breaks."""
        for i, st in enumerate(self._states):
            if st.context != self.lookback:
                return f"stream {i}'s look-back is not full ({st.context} of {self.lookback} frames)"
            if st.pending:
                return f"stream {i} has {st.pending} frames pending"
            if lens[i] != self.step:
                return f"lengths[{i}] = {lens[i]} is not the step ({self.step})"
            if ends[i]:
                return f"stream {i} ends with this push"
        return None

    def _check_capture(self, lens, ends) -> None:
        if torch.cuda.is_current_stream_capturing():
            why = self._steady(lens, ends)
            if why is None and self._buf is None:
                why = "the session has not run yet"
            if why is not None:
                raise RuntimeError(f"{self._what}: only a steady push can be captured into a graph (every look-back full, nothing pending, "
                                   f"every length the step, no end), but {why}; run the pushes up to the steady state outside stream capture")

    # ---- device side ----------------------------------------------------------------------------------------------------
    def _state_buffer(self, like, c: int):
        if self._buf is None or self._buf.dtype != like.dtype or self._c != c:
            self._buf = torch.zeros((self.streams, self.state_frames * c), dtype=like.dtype, device=self._device)
            self._c = c
        return self._buf

    def _desc(self, entries):
        return (_capi.StreamDesc * len(entries))(*entries)

    def _move(self, plan: _PushPlan, new, new_stride: int, c: int, stream):
        """gather / carry round by round, then append: the rows tensors of the plan's groups (group order), state updated."""
        lib, buf = self._lib, self._buf
        rows_t = []
        where = {}  # index into plan.rows -> (group, row in group)
        for g, group in enumerate(plan.groups):
            longest = max(plan.rows[k][2].frames for k in group)
            width = round4(longest) if c == 1 and self.round_to > 1 else longest  # audio rows: stride rounded to 4, as encode_long's
            shape = (len(group), width) if c == 1 else (len(group), width, c)
            rows_t.append(torch.empty(shape, dtype=new.dtype, device=self._device))
            for k_in, k in enumerate(group):
                where[k] = (g, k_in)
        new_ptr = new.data_ptr() if new.numel() else None
        new_frames = new.shape[1]
        for rnd in range(plan.rounds):
            for g, group in enumerate(plan.groups):
                entries = [_capi.StreamDesc(slot, where[k][1], r.held, r.take, r.off, r.pad, r.keep, r.prefix, 0, 0)
                           for k in group for slot, j, r in [plan.rows[k]] if j == rnd]
                if not entries:
                    continue
                desc = self._desc(entries)
                rt = rows_t[g]
                _capi.check(lib.l3ac_stream_gather(buf.data_ptr(), self.streams, self.state_frames, new_ptr, new_frames, new_stride, c, desc,
                                                   len(desc), rt.data_ptr(), rt.shape[0], rt.stride(0) // c, stream))
                if any(e.keep for e in entries):
                    _capi.check(lib.l3ac_stream_carry(rt.data_ptr(), rt.shape[0], rt.stride(0) // c, c, desc, len(desc), buf.data_ptr(),
                                                      self.streams, self.state_frames, stream))
        if plan.appends:
            desc = self._desc([_capi.StreamDesc(slot, 0, held, take, off, 0, 0, 0, 0, 0) for slot, held, off, take in plan.appends])
            _capi.check(lib.l3ac_stream_append(new_ptr, new_frames, new_stride, c, desc, len(desc), buf.data_ptr(), self.streams,
                                               self.state_frames, stream))
        return rows_t

    def _emit_plan(self, plan: _PushPlan, scale_num: int, scale_den: int):
        """Per group the emit descriptors in output frames (input frames * scale_num / scale_den), the per-stream output counts and the
        widest of them.  A stream's last chunk of the push zeroes its output row up to the width; a stream that emits nothing gets a
        descriptor of zeros only (in the first group's launch)."""
        sc = lambda v: v * scale_num // scale_den
        total = [0] * self.streams
        for slot, j, r in plan.rows:
            total[slot] += sc(r.frames - r.prefix)
        width = max(total)
        pos = [0] * self.streams
        out = [[None] * len(group) for group in plan.groups]
        order = sorted(range(len(plan.rows)), key=lambda k: (plan.rows[k][0], plan.rows[k][1]))  # each stream's chunks in time order
        where = {k: (g, k_in) for g, group in enumerate(plan.groups) for k_in, k in enumerate(group)}
        for k in order:
            slot, j, r = plan.rows[k]
            n = sc(r.frames - r.prefix)
            last = pos[slot] + n == total[slot]
            g, k_in = where[k]
            out[g][k_in] = _capi.StreamDesc(slot, k_in, sc(r.frames), 0, 0, 0, 0, sc(r.prefix), width - total[slot] if last else 0, pos[slot])
            pos[slot] += n
        if width and out:
            out[0] += [_capi.StreamDesc(slot, 0, 0, 0, 0, 0, 0, 0, width, 0) for slot in range(self.streams) if total[slot] == 0]
        return [self._desc(e) for e in out], total, width

    def _emit(self, src, desc, dst, stream) -> None:
        c = dst.shape[2] if dst.dim() == 3 else 1
        _capi.check(self._lib.l3ac_stream_emit(src.data_ptr(), src.shape[0], src.stride(0) // c, c, desc, len(desc), dst.data_ptr(),
                                               dst.shape[0], dst.stride(0) // c, dst.shape[1], stream))


class StreamEncoder(_Session):
    """``codec.stream_encoder(streams=S, process_window=16000, prefix_tokens=None)``: S concurrent live streams; see ``push``."""
    _what = "stream_encoder"
    _offline = "extract_unit"

    def __init__(self, codec, streams: int, process_window: int = 16000, prefix_tokens: Optional[int] = None,
                 chunks_per_call: Optional[int] = None):
        super().__init__(codec, streams, process_window, prefix_tokens, chunks_per_call, in_tokens=False)

    def push(self, audio, lengths=None, end=None, validate: bool = False):
        """New samples of every stream -> the tokens of the windows they complete.

        ``audio`` (S, n) fp32 CUDA at the codec's rate, n >= 0: row i holds stream i's new samples, ``lengths[i]`` in 0..n of them
        (absent: n; 0: the stream brings nothing this call; samples at or after ``lengths[i]`` are ignored, whatever they hold).
        ``end``: a bool or S bools; a stream that ends flushes what is pending as its last chunk, zero-padded to a whole hop, and its
        slot starts fresh for the next stream.  Returns ``encode_audio(..., lengths=)``'s shapes: ``q (S, T_out, C)``,
        ``{"indices": (S, T_out) int32, "level_indices": (S, T_out, D), "lengths": int32 on the CPU}``; ``lengths`` holds the tokens
        emitted per stream by this call, rows are zero after them, ``T_out`` is their maximum and may be 0.

        However a stream's samples are split over pushes, and whatever the other streams do, the concatenation of what it emits is,
        chunk by chunk, ``encode_audio`` of chunk ``[max(0, k * CL - P), (k + 1) * CL)`` alone with the look-back tokens dropped, bit
        for bit (CL = ``process_window`` in whole hops, P = ``prefix_tokens`` hops): for P < CL, ``encode_long``'s row.  After t
        samples ``floor(t / CL) * CL / hop`` tokens have been emitted, after ``end`` ``ceil(t / hop)``.
        There is no ``sample_rate=``: converting a live stream needs the filter's own carried state, which ``l3ac_amd.stream_resampler``
        keeps: push its output (``y, n = rs.push(packet, ...)``; ``enc.push(y, lengths=n, end=...)``) for
        ``encode_long(..., sample_rate=)``'s bits (``StreamResampler``).
        A steady push (every look-back full, nothing pending, every length CL, no end) can be captured into a graph after
        ``context().reserve(S, P + CL)`` and one eager steady push; under stream capture any other push raises RuntimeError.
        ``validate``: as encode_audio."""
        if not isinstance(audio, torch.Tensor) or audio.dim() != 2 or audio.shape[0] != self.streams:
            raise ValueError(f"audio must be a ({self.streams}, samples) tensor, got {tuple(getattr(audio, 'shape', ()))}")
        lens = self._lengths(lengths, audio.shape[1], "lengths")
        ends = self._ends(end)
        self._check_network(audio, "audio")
        self._check_capture(lens, ends)
        mc, hop, dev = self.codec.network.mc, self.hop, self._device
        plan = self._plan(lens, ends)
        new = contiguous_rows(audio.to(torch.float32))
        descs, total, width = self._emit_plan(plan, 1, hop)
        q_feature = torch.empty((self.streams, width, mc.feature_dim), dtype=torch.float32, device=dev)
        indices = torch.empty((self.streams, width), dtype=torch.int32, device=dev)
        level_indices = torch.empty((self.streams, width, len(mc.levels)), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), validated(self._ctx, "stream_encoder.push", validate):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._state_buffer(new, 1)
            rows_t = self._move(plan, new, row_stride(new), 1, stream)
            self._states = plan.after
            for group, rows, desc in zip(plan.groups, rows_t, descs):
                samples = [plan.rows[k][2].frames for k in group]
                longest = max(samples)
                # rows of one length (every steady push): the plain call, the same bits
                q, idx, li = encode_rows(self._ctx, rows, len(group), longest, rows.stride(0), None if min(samples) == longest else samples, stream)
                self._emit(q, desc, q_feature, stream)
                self._emit(idx, desc, indices, stream)
                self._emit(li, desc, level_indices, stream)
        return q_feature, {"indices": indices, "level_indices": level_indices, "lengths": torch.tensor(total, dtype=torch.int32)}


class StreamDecoder(_Session):
    """``codec.stream_decoder(streams=S, process_window=16000, prefix_tokens=None)``: the decoding side of S live streams; see ``push``."""
    _what = "stream_decoder"
    _offline = "decode_unit"

    def __init__(self, codec, streams: int, process_window: int = 16000, prefix_tokens: Optional[int] = None,
                 chunks_per_call: Optional[int] = None):
        super().__init__(codec, streams, process_window, prefix_tokens, chunks_per_call, in_tokens=True)

    def push(self, audio_feature=None, indices=None, lengths=None, end=None, validate: bool = False):
        """New tokens of every stream — int indices (S, m) or features (S, m, C), ``lengths`` in tokens (0..m) — -> ``(wave, n_tok)``:
        ``wave (S, T_out * hop)`` fp32, zero after each stream's own samples, and ``n_tok`` (int32, CPU): tokens' worth of audio emitted
        per stream by this call.  ``end`` as in ``StreamEncoder.push``.

        The step is ``process_window // hop`` tokens, as in ``decode_long``.  The concatenation of what a stream emits is, chunk by
        chunk, ``decode_audio`` of tokens ``[max(0, k * cl - P), (k + 1) * cl)`` alone with its first look-back samples dropped, bit
        for bit; for P < cl, ``decode_long``'s row.  The feature form and the index form agree; a session keeps the form of its first
        push (another form is accepted once no stream holds anything).  Out-of-range indices are clamped and counted as in
        ``decode_long``: a token inside a look-back counts each time it is decoded, and ``validate=True`` raises — after the push has
        taken effect — reporting occurrences.  A flush whose row is too short for the first EnhanceBlock raises ``decode_audio``'s
        ValueError before any device work, the session unchanged.  No ``sample_rate=``: push ``wave`` with ``lengths=n_tok * hop`` into a
        ``l3ac_amd.stream_resampler(S, config.sample_rate, rate)`` for ``decode_long(..., sample_rate=rate)``'s bits
        (``StreamResampler``).  Steady pushes are capturable as in ``StreamEncoder.push``."""
        src = audio_feature if audio_feature is not None else indices
        if src is None:
            raise ValueError("stream_decoder.push needs audio_feature or indices")
        mc, hop, dev = self.codec.network.mc, self.hop, self._device
        if not isinstance(src, torch.Tensor):
            raise ValueError("stream_decoder.push needs a tensor")
        if audio_feature is not None:
            if src.dim() != 3 or src.shape[-1] != mc.feature_dim or src.shape[0] != self.streams:
                raise ValueError(f"audio_feature must be ({self.streams}, tokens, {mc.feature_dim}), got {tuple(src.shape)}")
        elif src.dim() != 2 or src.shape[0] != self.streams or src.dtype.is_floating_point:
            raise ValueError(f"indices must be an integer ({self.streams}, tokens) tensor, got {src.dtype} {tuple(src.shape)}")
        c = mc.feature_dim if audio_feature is not None else 1
        lens = self._lengths(lengths, src.shape[1], "lengths (tokens)")
        ends = self._ends(end)
        self._check_network(src, "decode input")
        self._check_capture(lens, ends)
        dtype = torch.float32 if audio_feature is not None else torch.int32
        if self._buf is not None and (self._buf.dtype != dtype or self._c != c) and any(st.held for st in self._states):
            raise ValueError("stream_decoder.push: this session holds " + ("features" if self._c > 1 else "indices") +
                             "; the other form is accepted once no stream holds anything (end or reset)")
        plan = self._plan(lens, ends)
        if plan.rows and min(r.frames for _, _, r in plan.rows) * mc.en_coder_compress_rate < 2:
            # reference behaviour, as decode_audio: the first EnhanceBlock's InstanceNorm1d raises on a single frame
            raise ValueError(f"Expected more than 1 spatial element when training, got input size torch.Size([{self.streams}, 4, 1])")
        new = src.to(dtype)
        if not new.is_contiguous() and new.numel():
            new = new.contiguous()
        descs, total, width = self._emit_plan(plan, hop, 1)
        wave = torch.empty((self.streams, width), dtype=torch.float32, device=dev)
        bad_indices = None if audio_feature is not None else lambda bad: (
            f"{bad} index occurrences in the chunk rows (a token in a look-back counts each time it is decoded) "
            f"lie outside [0, {mc.codebook_size}): corrupted token stream")
        with torch.cuda.device(dev), validated(self._ctx, "stream_decoder.push", validate, bad_indices):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._state_buffer(new, c)
            rows_t = self._move(plan, new, max(new.shape[1], 1), c, stream)
            self._states = plan.after
            for group, rows, desc in zip(plan.groups, rows_t, descs):
                toks = [plan.rows[k][2].frames for k in group]
                longest = max(toks)
                # rows of one length: the plain call, the same bits
                out = decode_rows(self._ctx, rows, audio_feature is not None, len(group), longest, None if min(toks) == longest else toks, stream)
                self._emit(out, desc, wave, stream)
        return wave, torch.tensor([n // hop for n in total], dtype=torch.int32)


# ---- 3. streaming sample-rate conversion: the session -------------------------------------------------------------
class StreamResampler(_CarrySession):
    """``l3ac_amd.stream_resampler(streams, orig_sr, target_sr)``: S concurrent live streams converted from ``orig_sr`` to ``target_sr``
    packet by packet, with ``resample``'s bits; see ``push``.  Needs no codec and no context, as ``resample`` needs none.  In front of a
    ``stream_encoder``, or behind a ``stream_decoder``, it makes a live stream at another rate give ``encode_long(..., sample_rate=)``'s /
    ``decode_long(..., sample_rate=)``'s bits::

        rs  = l3ac.stream_resampler(S, 48000, codec.config.sample_rate)
        enc = codec.stream_encoder(streams=S, process_window=16000)
        y, n = rs.push(packet_48k, lengths=new_samples, end=finished)
        q_feature, indices = enc.push(y, lengths=n, end=finished)        # encode_long(..., sample_rate=48000)'s bits
        # decoding side
        wave, n_tok = dec.push(indices=..., lengths=..., end=finished)
        out, n_out = rs_out.push(wave, lengths=n_tok * hop, end=finished)  # decode_long(..., sample_rate=44100)'s bits
    """

    _what = "stream_resampler"
    _fresh = ResampleState()
    _elements = "samples"
    _phase = "the position of every stream in the filter's phase cycle"

    def __init__(self, streams: int, orig_sr: int, target_sr: int):
        super().__init__(streams)
        if isinstance(orig_sr, bool) or isinstance(target_sr, bool) or int(orig_sr) != orig_sr or int(target_sr) != target_sr:
            raise ValueError(f"rates must be integers, got {orig_sr!r} -> {target_sr!r}")
        self.orig_sr, self.target_sr = int(orig_sr), int(target_sr)
        if not (0 < self.orig_sr < 2 ** 31 and 0 < self.target_sr < 2 ** 31):
            raise ValueError(f"resample: rates must be positive 32-bit integers (got {self.orig_sr} -> {self.target_sr})")
        state = self._lib.l3ac_resample_stream_state(self.orig_sr, self.target_sr)
        if state < 0:  # resample_length's error: a reduced max(up, down) above 1024
            raise ValueError(self._lib.l3ac_last_error().decode())
        self.geometry = resample_geometry(self.orig_sr, self.target_sr)
        self.state_frames = int(state)
        assert self.state_frames == round4(self.geometry.K - 1)
        self._bank = None

    @property
    def delay(self) -> float:
        """How far the output lags the input, in input samples: half_len / up (0 at equal rates).  ``end`` flushes it."""
        geo = self.geometry
        return 0.0 if geo.up == geo.down else geo.half_len / geo.up

    @torch.no_grad()
    def push(self, audio, lengths=None, end=None):
        """New samples of every stream at ``orig_sr`` -> ``(y, lengths_out)``: the samples at ``target_sr`` they complete.

        ``audio`` (S, n) fp32 CUDA, n >= 0: row i holds stream i's new samples, ``lengths[i]`` in 0..n of them (absent: n; samples at or
        after ``lengths[i]`` are ignored, whatever they hold).  ``end``: a bool or S bools; a stream that ends emits the rest of its
        outputs, the samples after its end counting as zeros, and its slot starts fresh.  ``y`` is (S, T_out) fp32, zero after each
        stream's own outputs; ``lengths_out`` (int32, CPU) holds the outputs per stream, ``T_out`` is their maximum and may be 0.

        For finite input, however a stream's samples are split over pushes and whatever the other streams do, the concatenation of what
        stream i emits is ``resample(x_i[None, :], orig_sr, target_sr)[0]`` bit for bit; ``resample_length(orig_sr, target_sr, N)`` samples
        have been emitted once a stream of N samples has ended.  Before that an output is emitted as soon as its newest input has
        arrived: the output lags the input by ``delay`` input samples.  Equal rates pass the samples through at once, bit for bit.
        Non-finite samples INSIDE a stream are outside the guarantee (the offline kernel multiplies a few more of them by zero taps).
        One kernel launch per push, no host synchronisation; every count is a host integer.  Errors are raised before any device work and
        leave the session unchanged.  A push under stream capture raises RuntimeError: the host position advances with every push, so
        a captured push would replay one position for ever."""
        if not isinstance(audio, torch.Tensor) or audio.dim() != 2 or audio.shape[0] != self.streams:
            raise ValueError(f"audio must be a ({self.streams}, samples) tensor, got {tuple(getattr(audio, 'shape', ()))}")
        new, plan, total, width = self._take(audio, "audio", torch.float32, lengths, "lengths", end, resample_advance, self.geometry)
        dev, n = new.device, new.shape[1]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if self._device is None:
                self._bank = _resample_bank(dev, self.orig_sr, self.target_sr)
            # equal rates: a copy, with no state to carry
            src, dst = self._buffers(dev, None if self.geometry.up == self.geometry.down else (self.streams, self.state_frames), torch.float32)
            y = torch.empty((self.streams, width), dtype=torch.float32, device=dev)
            desc = (_capi.ResampleStreamDesc * self.streams)(*[_capi.ResampleStreamDesc(i, p.held, p.take, p.count, p.keep, p.q0)
                                                                for i, (p, _) in enumerate(plan)])
            _capi.check(self._lib.l3ac_resample_stream(
                src, dst, self.streams, self.state_frames, new.data_ptr() if n else None, n, row_stride(new), self.orig_sr, self.target_sr,
                None if self._bank is None else self._bank.data_ptr(), desc, self.streams, y.data_ptr() if width else None, width,
                max(width, 1), stream))
            self._commit(plan)
        return y, torch.tensor(total, dtype=torch.int32)
