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
from ._rows import int_list, row_stride
from .streaming import _CarrySession, round4


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
class _WireSession(_CarrySession):
    """What StreamPacker and StreamUnpacker share: ``bits``, and one uint32 of pending bits per stream as the carried state."""
    _what = "wire session"
    _phase = "the bit phase of every stream"

    def __init__(self, streams: int, bits: int):
        super().__init__(streams)
        # 8..32: fewer than 8 padding bits can then never hold a token, so a stream's end is unambiguous
        self.bits = _check_bits(bits, lo=8)


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
        new, plan, total, width = self._take(indices, "indices", torch.int32, lengths, "lengths", end, pack_advance, self.bits)
        dev, n = new.device, new.shape[1]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            src, dst = self._buffers(dev, (self.streams,), torch.int32)
            out = torch.empty((self.streams, round4(width)), dtype=torch.uint8, device=dev)
            desc = (_capi.PackStreamDesc * self.streams)(*[_capi.PackStreamDesc(i, *p) for i, (p, _) in enumerate(plan)])
            _capi.check(self._lib.l3ac_pack_stream(src, dst, self.streams, new.data_ptr() if n else None, n, row_stride(new), self.bits, desc,
                                                   self.streams, out.data_ptr() if width else None, width, out.shape[1], stream))
            self._commit(plan)
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
        new, plan, total, width = self._take(packed, "packed", torch.uint8, lengths, "lengths (bytes)", end, unpack_advance, self.bits)
        dev, n = new.device, new.shape[1]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            src, dst = self._buffers(dev, (self.streams,), torch.int32)
            out = torch.empty((self.streams, width), dtype=torch.int32, device=dev)
            desc = (_capi.UnpackStreamDesc * self.streams)(*[_capi.UnpackStreamDesc(i, *p) for i, (p, _) in enumerate(plan)])
            _capi.check(self._lib.l3ac_unpack_stream(src, dst, self.streams, new.data_ptr() if n else None, n, row_stride(new), self.bits, desc,
                                                     self.streams, out.data_ptr() if width else None, width, max(width, 1), stream))
            self._commit(plan)
        return out, torch.tensor(total, dtype=torch.int32)


# ---- 3. pack_indices / unpack_indices, plain and ragged --------------------------------------------------------------------------------
def token_lengths(lengths, batch: int, limit: int, what: str = "lengths") -> List[int]:
    """``lengths=`` of pack_indices / unpack_indices as B Python ints in 0..limit: ``ragged_lengths``' checks, but a row may be empty."""
    return int_list(lengths, batch, 0, limit, what, f"a batch of {batch}")


def pack_indices(indices: torch.Tensor, bits: int, lengths=None):
    """int indices (B, T_tok) on the GPU -> little-endian bit stream, one row of whole 32-bit words per clip, as
    uint8 (B, 4 * ceil(T_tok * bits / 32)).  The reference has no wire format (it keeps int32 tensors).
    ``lengths`` (B token counts in 0..T_tok; a sequence, an array or a tensor, checked as ``ragged_lengths`` checks but a row may be
    empty): the ragged form, ``(packed, nbytes)``: row i is the stream of its first ``lengths[i]`` tokens alone, ``nbytes[i] =
    packed_bytes(lengths[i], bits)`` bytes (int32, CPU) followed by zeros; tokens at or after ``lengths[i]`` are ignored, whatever they
    hold (``encode_audio(..., lengths=)`` and ``encode_long`` return such rows)."""
    if not indices.is_cuda or indices.dim() != 2:
        raise ValueError("indices must be a (batch, tokens) CUDA tensor")
    if lengths is not None:
        lens = token_lengths(lengths, indices.shape[0], indices.shape[1])
        if not 1 <= int(bits) <= 32 or int(bits) != bits or indices.shape[0] == 0 or indices.shape[1] == 0:
            raise ValueError(f"pack_indices: {tuple(indices.shape)} indices of {bits!r} bits")
        bits = int(bits)
    idx = indices.to(torch.int32).contiguous()
    b, n_tok = idx.shape
    words = -(-n_tok * bits // 32)
    lib = _capi.load_library()
    with torch.cuda.device(idx.device):
        stream = torch.cuda.current_stream(idx.device).cuda_stream
        if lengths is None:
            out = torch.empty((b, words), dtype=torch.int32, device=idx.device)
            _capi.check(lib.l3ac_pack_indices(idx.data_ptr(), b, n_tok, bits, out.data_ptr(), words, stream))
            return out.view(torch.uint8)
        # every row a stream of its own, ended, with no held state: one l3ac_pack_stream call
        nbytes = [packed_bytes(n, bits) for n in lens]
        out = torch.empty((b, 4 * words), dtype=torch.uint8, device=idx.device)
        desc = (_capi.PackStreamDesc * b)(*[_capi.PackStreamDesc(i, 0, n, k, 0) for i, (n, k) in enumerate(zip(lens, nbytes))])
        _capi.check(lib.l3ac_pack_stream(None, None, b, idx.data_ptr(), n_tok, n_tok, bits, desc, b, out.data_ptr(), 4 * words, 4 * words, stream))
    return out, torch.tensor(nbytes, dtype=torch.int32)


def unpack_indices(packed: torch.Tensor, n_tok: int, bits: int, lengths=None) -> torch.Tensor:
    """Inverse of `pack_indices`: uint8 (B, 4 * words) -> int32 (B, n_tok).  ``lengths`` (B token counts in 0..n_tok): the ragged form:
    row i is zero after its own ``lengths[i]`` tokens, and bytes beyond its ``packed_bytes(lengths[i], bits)`` are never read."""
    if not packed.is_cuda or packed.dim() != 2 or packed.dtype != torch.uint8 or packed.shape[1] % 4:
        raise ValueError("packed must be a (batch, 4 * words) uint8 CUDA tensor")
    words = packed.shape[1] // 4
    if words * 32 < n_tok * bits:
        raise ValueError("packed stream too short for n_tok tokens")
    if lengths is not None:
        lens = token_lengths(lengths, packed.shape[0], n_tok)
        if not 1 <= int(bits) <= 32 or int(bits) != bits or packed.shape[0] == 0 or n_tok < 1:
            raise ValueError(f"unpack_indices: {packed.shape[0]} rows of {n_tok} tokens of {bits!r} bits")
        n_tok, bits = int(n_tok), int(bits)
    src = packed.contiguous()
    b, row_bytes = src.shape
    out = torch.empty((b, n_tok), dtype=torch.int32, device=src.device)
    lib = _capi.load_library()
    with torch.cuda.device(src.device):
        stream = torch.cuda.current_stream(src.device).cuda_stream
        if lengths is None:
            _capi.check(lib.l3ac_unpack_indices(src.view(torch.int32).data_ptr(), b, n_tok, bits, words, out.data_ptr(), stream))
        else:  # every row a stream of its own, ended, with no held state: one l3ac_unpack_stream call
            desc = (_capi.UnpackStreamDesc * b)(*[_capi.UnpackStreamDesc(i, 0, packed_bytes(n, bits), n, 0) for i, n in enumerate(lens)])
            _capi.check(lib.l3ac_unpack_stream(None, None, b, src.data_ptr(), row_bytes, row_bytes, bits, desc, b, out.data_ptr(), n_tok, n_tok, stream))
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


def bits_per_token(mc) -> int:
    """ceil(log2(codebook size)): 17 at 1kbps (117 649 codes), 18 at 3kbps (250 047)."""
    return max(1, (mc.codebook_size - 1).bit_length())


def frame_header(mc, sample_rate: int, n_tok: int, n_samples: int) -> bytes:
    """The 24-byte little-endian header of one recording's frame: ``b"L3AC"``, u8 format version (1), u8 bits per token, u16 hop,
    u32 codebook size, u32 codec sample rate, u32 token count, u32 sample count at the codec's rate.  ``mc``: the codec's ModelConfig."""
    return _HEADER.pack(FRAME_MAGIC, FRAME_VERSION, bits_per_token(mc), mc.hop_length, mc.codebook_size, int(sample_rate), int(n_tok), int(n_samples))


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
    if bits != bits_per_token(mc):
        raise ValueError(f"frame: {bits} bits per token, but this codec's tokens have {bits_per_token(mc)} bits")
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
