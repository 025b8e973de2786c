"""The token wire format for live streams: ragged packing, byte sessions and the frame header.

The format is ``pack_indices``', stated per byte: token t of a stream occupies bits ``[t * bits, (t + 1) * bits)`` of a little-endian bit
stream, byte k of the stream is bits ``[8k, 8k + 8)``, and a stream of n tokens is ``packed_bytes(n, bits) = ceil(n * bits / 8)`` bytes, its
last byte zero-padded: the first ``packed_bytes(n, bits)`` bytes of ``pack_indices``' row for the same tokens (the rest of that row is zero).

Geometry first, as pure functions of host integers (no tensors, no GPU), written as ``resample_advance`` is: ``pack_advance`` /
``unpack_advance``.  Then the sessions, ``StreamPacker`` / ``StreamUnpacker`` (``l3ac_amd.stream_packer`` / ``stream_unpacker``): the state
carried between pushes is one uint32 per stream, the bits that have not filled a byte (completed a token) yet, in two device buffers read
and written alternately; one launch of csrc/kernels/bitpack_stream.hip per push.  The ragged forms of ``pack_indices`` / ``unpack_indices``
go through the same two kernels with no held state and every row ended.  Last, the frame header of ``L3AC.compress`` / ``decompress``.
"""
from __future__ import annotations

import struct
from typing import List, NamedTuple, Tuple

import torch

from . import _capi
from .streaming import _Session, _check_streams, round4


# ---- 1. geometry -----------------------------------------------------------------------------------------------------------------------
def _check_bits(bits, lo: int = 1) -> int:
    if isinstance(bits, bool) or int(bits) != bits or not lo <= int(bits) <= 32:
        raise ValueError(f"bits must be an integer in {lo}..32, got {bits!r}")
    return int(bits)


def packed_bytes(n_tok: int, bits: int) -> int:
    """Bytes of a stream of ``n_tok`` tokens: ceil(n_tok * bits / 8) (l3ac_packed_bytes)."""
    bits = _check_bits(bits)
    if int(n_tok) != n_tok or n_tok < 0:
        raise ValueError(f"{n_tok!r} tokens")
    return -(-int(n_tok) * bits // 8)


class PackState(NamedTuple):
    """What one packed stream is between pushes: ``held_bits`` (0..7) bits that have not filled a byte yet are on the device;
    ``tokens_seen`` tokens received and ``bytes_emitted`` bytes produced so far (Python ints: they never reach the device)."""
    held_bits: int = 0
    tokens_seen: int = 0
    bytes_emitted: int = 0


class PackPush(NamedTuple):
    """One stream's share of one packing push, l3ac_pack_stream_desc's fields: the stream's bit string is its ``held`` pending bits
    followed by ``take`` tokens; its first ``count`` bytes are emitted and its last ``keep`` bits stay pending."""
    held: int
    take: int
    count: int
    keep: int


class UnpackState(NamedTuple):
    """What one unpacked stream is between pushes: ``held_bits`` (0..bits-1) bits that have not completed a token yet are on the device;
    ``bytes_seen`` bytes received and ``tokens_emitted`` tokens produced so far (Python ints: they never reach the device)."""
    held_bits: int = 0
    bytes_seen: int = 0
    tokens_emitted: int = 0


class UnpackPush(NamedTuple):
    """One stream's share of one unpacking push, l3ac_unpack_stream_desc's fields: ``held`` pending bits followed by ``take`` bytes;
    ``count`` tokens are emitted and the last ``keep`` bits stay pending."""
    held: int
    take: int
    count: int
    keep: int


def pack_advance(state: PackState, new_tokens: int, end: bool, bits: int) -> Tuple[PackPush, PackState]:
    """One push of ``new_tokens`` tokens onto a stream in ``state``.  Not ended: the whole bytes of held + new bits are emitted, the
    remainder stays pending.  ``end``: the last byte is emitted zero-padded and the state afterwards is a fresh stream's."""
    bits = _check_bits(bits)
    if new_tokens < 0:
        raise ValueError(f"{new_tokens} new tokens")
    held, seen, done = state
    total = held + new_tokens * bits
    count, keep = (-(-total // 8), 0) if end else divmod(total, 8)
    push = PackPush(held, new_tokens, count, keep)
    return push, (PackState() if end else PackState(keep, seen + new_tokens, done + count))


def unpack_advance(state: UnpackState, new_bytes: int, end: bool, bits: int) -> Tuple[UnpackPush, UnpackState]:
    """One push of ``new_bytes`` bytes onto a stream in ``state``: the whole tokens of held + new bits are emitted, the remainder stays
    pending.  ``end``: the remainder (a stream's byte padding) is dropped and the state afterwards is a fresh stream's."""
    bits = _check_bits(bits)
    if new_bytes < 0:
        raise ValueError(f"{new_bytes} new bytes")
    held, seen, done = state
    count, keep = divmod(held + 8 * new_bytes, bits)
    push = UnpackPush(held, new_bytes, count, 0 if end else keep)
    return push, (UnpackState() if end else UnpackState(keep, seen + new_bytes, done + count))


# ---- 2. sessions -----------------------------------------------------------------------------------------------------------------------
class _WireSession:
    """What StreamPacker and StreamUnpacker share: the per-stream host state and the two device state buffers."""
    _what = "wire session"
    _fresh = None  # the state of a fresh stream

    def __init__(self, streams: int, bits: int):
        self.streams = _check_streams(streams)
        # 8..32: fewer than 8 padding bits can then never hold a token, so a stream's end is unambiguous
        self.bits = _check_bits(bits, lo=8)
        self._lib = _capi.load_library()
        self._states = [self._fresh] * self.streams
        self._device = None
        self._bufs = None  # two [streams] uint32 buffers, read and written alternately: allocated at the first push

    _lengths = _Session._lengths
    _ends = _Session._ends

    @property
    def states(self) -> list:
        """The streams' host state (a copy): bits pending on the device, elements seen and emitted since the stream began."""
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

    def _check_device(self, t: torch.Tensor, what: str):
        if not t.is_cuda:
            raise RuntimeError(f"{self._what}: {what} is on {t.device}: l3ac_amd has no CPU path")
        if self._device is not None and t.device != self._device:
            raise RuntimeError(f"{self._what}: {what} is on {t.device} but the session's state is on {self._device}")
        if t.shape[1] >= 2 ** 31:
            raise ValueError(f"{self._what}: a push of {t.shape[1]} elements")
        with torch.cuda.device(t.device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._what}: a push cannot be captured into a graph: the bit phase of every stream is a host value that "
                                   "advances with every push")

    def _buffers(self, dev):
        if self._device is None:
            self._device, self._bufs = dev, [torch.zeros((self.streams,), dtype=torch.int32, device=dev) for _ in range(2)]
        return self._bufs[0].data_ptr(), self._bufs[1].data_ptr()


class StreamPacker(_WireSession):
    """``l3ac_amd.stream_packer(streams, bits)``: the tokens of S concurrent live streams -> the bytes of the wire, push by push, with
    ``pack_indices``' bits; see ``push``.  Needs no codec and no context, as ``pack_indices`` needs none.  It composes with the codec's
    sessions (``end`` travels along the chain)::

        enc, dec = codec.stream_encoder(streams=S), codec.stream_decoder(streams=S)
        packer, unpacker = l3ac.stream_packer(S, bits), l3ac.stream_unpacker(S, bits)      # bits = l3ac.bits_per_token(codec.network.mc)
        _, tok = enc.push(audio, lengths=new_samples, end=finished)
        wire, n_bytes = packer.push(tok["indices"], lengths=tok["lengths"], end=finished)   # wire[i, :n_bytes[i]] goes out
        idx, n_tok = unpacker.push(wire, lengths=n_bytes, end=finished)
        wave, n = dec.push(indices=idx, lengths=n_tok, end=finished)
    """
    _what = "stream_packer"
    _fresh = PackState()

    @torch.no_grad()
    def push(self, indices, lengths=None, end=None):
        """New tokens of every stream -> ``(packed, lengths_out)``: the bytes they complete.

        ``indices`` (S, n) integer CUDA, n >= 0: row i holds stream i's new tokens, ``lengths[i]`` in 0..n of them (absent: n; tokens at or
        after ``lengths[i]`` are ignored, whatever they hold).  Bits of an index above ``bits`` are dropped.  ``end``: a bool or S bools; a
        stream that ends emits its last byte zero-padded and its slot starts fresh.  ``packed`` is uint8 (S, n_bytes), zero after each
        stream's own bytes (rows are 4-byte aligned: a row stride rounded up to a multiple of 4); ``lengths_out`` (int32, CPU) holds the
        bytes per stream, ``n_bytes`` is their maximum and may be 0.

        However a stream's tokens are split over pushes and whatever the other streams do, the concatenation of what stream i emits is
        ``pack_indices(tokens_i[None, :], bits)[0, :packed_bytes(n_i, bits)]`` once the stream of n_i tokens has ended; before that,
        ``floor(tokens * bits / 8)`` bytes have been emitted.  One kernel launch per push, no host synchronisation; every count is a host
        integer.  Errors are raised before any device work and leave the session unchanged.  A push under stream capture raises
        RuntimeError: the bit phase advances with every push, so a captured push would replay one phase for ever."""
        if not isinstance(indices, torch.Tensor) or indices.dim() != 2 or indices.shape[0] != self.streams or indices.dtype.is_floating_point \
                or indices.dtype.is_complex or indices.dtype == torch.bool:
            raise ValueError(f"indices must be an integer ({self.streams}, tokens) tensor, got {getattr(indices, 'dtype', type(indices))} "
                             f"{tuple(getattr(indices, 'shape', ()))}")
        n = indices.shape[1]
        lens = self._lengths(lengths, n, "lengths")
        ends = self._ends(end)
        self._check_device(indices, "indices")
        dev = indices.device
        plan = [pack_advance(st, m, e, self.bits) for st, m, e in zip(self._states, lens, ends)]
        total = [p.count for p, _ in plan]
        width = max(total)
        new = indices.to(torch.int32)
        if new.stride(-1) != 1 and new.numel():
            new = new.contiguous()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            src, dst = self._buffers(dev)
            out = torch.empty((self.streams, round4(width)), dtype=torch.uint8, device=dev)
            desc = (_capi.PackStreamDesc * self.streams)(*[_capi.PackStreamDesc(i, *p) for i, (p, _) in enumerate(plan)])
            _capi.check(self._lib.l3ac_pack_stream(
                src, dst, self.streams, new.data_ptr() if new.numel() else None, n, new.stride(0) if self.streams > 1 and n else max(n, 1),
                self.bits, desc, self.streams, out.data_ptr() if width else None, width, out.shape[1], stream))
            self._bufs.reverse()
            self._states = [after for _, after in plan]
        return out[:, :width], torch.tensor(total, dtype=torch.int32)


class StreamUnpacker(_WireSession):
    """``l3ac_amd.stream_unpacker(streams, bits)``: the receiving side of ``StreamPacker``: any run of bytes of S concurrent streams in,
    the tokens they complete out, with ``unpack_indices``' bits; see ``push``."""
    _what = "stream_unpacker"
    _fresh = UnpackState()

    @torch.no_grad()
    def push(self, packed, lengths=None, end=None):
        """New bytes of every stream -> ``(indices, lengths_out)``: the tokens they complete.

        ``packed`` (S, n) uint8 CUDA, n >= 0, rows at any byte alignment: row i holds stream i's new bytes, ``lengths[i]`` in 0..n of them
        (absent: n; bytes at or after ``lengths[i]`` are ignored, whatever they hold).  ``end``: a bool or S bools; a stream that ends drops
        the bits that are left (its byte padding) and its slot starts fresh.  ``indices`` is int32 (S, n_tok), zero after each stream's own
        tokens; ``lengths_out`` (int32, CPU) holds the tokens per stream, ``n_tok`` is their maximum and may be 0.

        However a stream's bytes are split over pushes and whatever the other streams do, the concatenation of what stream i emits is
        ``unpack_indices`` of the whole stream: ``floor(8 * N / bits)`` tokens for N bytes.  A stream of n tokens must be fed its
        ``packed_bytes(n, bits)`` bytes: fed ``pack_indices``' word-padded row instead, it can yield trailing zero tokens (up to 31 padding
        bits can hold one).  One kernel launch per push, no host synchronisation; errors are raised before any device work and leave the
        session unchanged; a push under stream capture raises RuntimeError, as ``StreamPacker.push``."""
        if not isinstance(packed, torch.Tensor) or packed.dim() != 2 or packed.shape[0] != self.streams or packed.dtype != torch.uint8:
            raise ValueError(f"packed must be a uint8 ({self.streams}, bytes) tensor, got {getattr(packed, 'dtype', type(packed))} "
                             f"{tuple(getattr(packed, 'shape', ()))}")
        n = packed.shape[1]
        lens = self._lengths(lengths, n, "lengths (bytes)")
        ends = self._ends(end)
        self._check_device(packed, "packed")
        dev = packed.device
        plan = [unpack_advance(st, m, e, self.bits) for st, m, e in zip(self._states, lens, ends)]
        total = [p.count for p, _ in plan]
        width = max(total)
        new = packed if packed.stride(-1) == 1 or not packed.numel() else packed.contiguous()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            src, dst = self._buffers(dev)
            out = torch.empty((self.streams, width), dtype=torch.int32, device=dev)
            desc = (_capi.UnpackStreamDesc * self.streams)(*[_capi.UnpackStreamDesc(i, *p) for i, (p, _) in enumerate(plan)])
            _capi.check(self._lib.l3ac_unpack_stream(
                src, dst, self.streams, new.data_ptr() if new.numel() else None, n, new.stride(0) if self.streams > 1 and n else max(n, 1),
                self.bits, desc, self.streams, out.data_ptr() if width else None, width, max(width, 1), stream))
            self._bufs.reverse()
            self._states = [after for _, after in plan]
        return out, torch.tensor(total, dtype=torch.int32)


# ---- 3. the ragged forms of pack_indices / unpack_indices ------------------------------------------------------------------------------
def token_lengths(lengths, batch: int, limit: int, what: str = "lengths") -> List[int]:
    """``lengths=`` of pack_indices / unpack_indices as B Python ints in 0..limit: ``ragged_lengths``' checks, but a row may be empty."""
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().reshape(-1).tolist()
    try:
        seq = list(lengths)
        vals = [int(v) for v in seq]
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a sequence of {batch} ints") from None
    if any(float(v) != int(v) for v in seq):
        raise ValueError(f"{what} must be integers")
    if len(vals) != batch:
        raise ValueError(f"{what}: {len(vals)} entries for a batch of {batch}")
    bad = [v for v in vals if not 0 <= v <= limit]
    if bad:
        raise ValueError(f"{what}: {bad[0]} outside [0, {limit}]")
    return vals


def pack_ragged(idx: torch.Tensor, bits: int, lens: List[int]):
    """int32 (B, T_tok) contiguous CUDA, row i holding ``lens[i]`` tokens -> (uint8 (B, 4 * ceil(T_tok * bits / 32)), bytes per row int32
    CPU): every row a stream of its own, ended, with no held state (one l3ac_pack_stream call)."""
    b, n_tok = idx.shape
    row_bytes = 4 * (-(-n_tok * bits // 32))
    nbytes = [packed_bytes(n, bits) for n in lens]
    out = torch.empty((b, row_bytes), dtype=torch.uint8, device=idx.device)
    desc = (_capi.PackStreamDesc * b)(*[_capi.PackStreamDesc(i, 0, n, k, 0) for i, (n, k) in enumerate(zip(lens, nbytes))])
    with torch.cuda.device(idx.device):
        _capi.check(_capi.load_library().l3ac_pack_stream(None, None, b, idx.data_ptr(), n_tok, n_tok, bits, desc, b, out.data_ptr(), row_bytes,
                                                          row_bytes, torch.cuda.current_stream(idx.device).cuda_stream))
    return out, torch.tensor(nbytes, dtype=torch.int32)


def unpack_ragged(packed: torch.Tensor, n_tok: int, bits: int, lens: List[int]) -> torch.Tensor:
    """uint8 (B, row_bytes) contiguous CUDA, row i holding the ``packed_bytes(lens[i], bits)`` bytes of ``lens[i]`` tokens -> int32
    (B, n_tok), zero after each row's own tokens (one l3ac_unpack_stream call; bytes after a row's own are never read)."""
    b, row_bytes = packed.shape
    out = torch.empty((b, n_tok), dtype=torch.int32, device=packed.device)
    desc = (_capi.UnpackStreamDesc * b)(*[_capi.UnpackStreamDesc(i, 0, packed_bytes(n, bits), n, 0) for i, n in enumerate(lens)])
    with torch.cuda.device(packed.device):
        _capi.check(_capi.load_library().l3ac_unpack_stream(None, None, b, packed.data_ptr(), row_bytes, row_bytes, bits, desc, b, out.data_ptr(),
                                                            n_tok, n_tok, torch.cuda.current_stream(packed.device).cuda_stream))
    return out


# ---- 4. frames: audio -> bytes -> audio ------------------------------------------------------------------------------------------------
FRAME_MAGIC = b"L3AC"
FRAME_VERSION = 1
_HEADER = struct.Struct("<4sBBHIIII")  # magic, version, bits, hop, codebook size, sample rate, token count, sample count
FRAME_HEADER_BYTES = _HEADER.size
assert FRAME_HEADER_BYTES == 24


class Frame(NamedTuple):
    """A parsed frame: its token count, its sample count at the codec's rate and its payload, ``packed_bytes(n_tok, bits)`` bytes."""
    n_tok: int
    n_samples: int
    payload: bytes


def _mc_bits(mc) -> int:
    return max(1, (mc.codebook_size - 1).bit_length())  # bits_per_token


def frame_header(mc, sample_rate: int, n_tok: int, n_samples: int) -> bytes:
    """The 24-byte little-endian header of one recording's frame: ``b"L3AC"``, u8 format version (1), u8 bits per token, u16 hop,
    u32 codebook size, u32 codec sample rate, u32 token count, u32 sample count at the codec's rate.  ``mc``: the codec's ModelConfig."""
    return _HEADER.pack(FRAME_MAGIC, FRAME_VERSION, _mc_bits(mc), mc.hop_length, mc.codebook_size, int(sample_rate), int(n_tok), int(n_samples))


def parse_frame(blob, mc, sample_rate: int) -> Frame:
    """Check one frame against the codec it is to be decoded by (``mc``: its ModelConfig, ``sample_rate``: its rate); raises ValueError
    naming the field that is wrong.  Host only."""
    try:
        blob = bytes(blob)
    except TypeError:
        raise ValueError(f"frame: a bytes-like object is needed, got {type(blob).__name__}") from None
    if len(blob) < FRAME_HEADER_BYTES:
        raise ValueError(f"frame: {len(blob)} bytes are shorter than the header ({FRAME_HEADER_BYTES} bytes)")
    magic, version, bits, hop, codebook, rate, n_tok, n_samples = _HEADER.unpack_from(blob)
    if magic != FRAME_MAGIC:
        raise ValueError(f"frame: bad magic {magic!r}, not {FRAME_MAGIC!r}")
    if version != FRAME_VERSION:
        raise ValueError(f"frame: unknown format version {version} (this package reads version {FRAME_VERSION})")
    if bits != _mc_bits(mc):
        raise ValueError(f"frame: {bits} bits per token, but this codec's tokens have {_mc_bits(mc)} bits")
    if hop != mc.hop_length:
        raise ValueError(f"frame: a hop of {hop} samples, but this codec's hop is {mc.hop_length}")
    if codebook != mc.codebook_size:
        raise ValueError(f"frame: a codebook size of {codebook}, but this codec's codebook size is {mc.codebook_size}")
    if rate != int(sample_rate):
        raise ValueError(f"frame: a sample rate of {rate} Hz, but this codec's sample rate is {int(sample_rate)} Hz")
    if n_tok < 1 or n_tok != -(-n_samples // hop):
        raise ValueError(f"frame: a token count of {n_tok} does not go with a sample count of {n_samples} at a hop of {hop}")
    payload = blob[FRAME_HEADER_BYTES:]
    if len(payload) != packed_bytes(n_tok, bits):
        raise ValueError(f"frame: a payload of {len(payload)} bytes, but {n_tok} tokens of {bits} bits are {packed_bytes(n_tok, bits)} bytes")
    return Frame(n_tok, n_samples, payload)
