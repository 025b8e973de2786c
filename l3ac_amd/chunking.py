"""Long-audio chunking: the split / merge bookkeeping of the reference's ``ChunkData`` (l3ac/codec.py:159-188) and the
chunk plan of the corrected long-audio path (``L3AC.extract_unit`` / ``L3AC.decode_unit`` in this package).

The reference's ``extract_unit`` / ``decode_unit`` (codec.py:124-156) cut a clip into windows that overlap their predecessor
by ONE hop, run ``Codec.compress`` on each — which skips ``en_encoder`` / ``en_decoder`` entirely — and glue the pieces with
``ChunkData``.  Here the same bookkeeping is kept (same class, same ``data`` / ``chunk_data`` semantics, along ``dim`` —
default 0, the reference's: a waveform ``(T,)``, indices ``(T_tok,)`` or token features ``(T_tok, C)`` are all cut along their
first dimension), but every chunk goes through
the full path (encoder -> en_encoder -> quantizer, en_decoder -> decoder) and the overlap is a parameter whose default is the
local attention's look-back (one window of tokens), since the transformer — not the one-hop conv halo — is what carries
context across a cut.

Last, the chunks of a whole batch of recordings as rows of ragged calls (``L3AC.encode_long`` / ``decode_long``):
``chunk_plan`` and the device movers ``_chunk_cut`` / ``_chunk_merge``.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch

from . import _capi


class ChunkData:
    """reference l3ac/codec.py:159-188, generalised from dim 0 to a chosen dim.  Either ``original_data`` (to be cut:
    chunk i > 0 is ``data[i*chunk_len - prefix_len : (i+1)*chunk_len]``, chunk 0 has no prefix) or ``chunk_data`` (to be merged:
    every chunk after the first drops its first ``prefix_len`` elements)."""

    def __init__(self, chunk_len: int, prefix_len: int, original_data: Optional[torch.Tensor] = None,
                 chunk_data: Optional[Sequence[torch.Tensor]] = None, dim: int = 0):
        assert chunk_len > prefix_len
        self.chunk_len = chunk_len
        self.prefix_len = prefix_len
        self.dim = dim
        self._original_data = original_data
        self._chunk_data = None if chunk_data is None else list(chunk_data)

    @property
    def data(self) -> torch.Tensor:
        if self._original_data is not None:
            return self._original_data
        parts = [self._chunk_data[0]]
        for x in self._chunk_data[1:]:
            parts.append(x.narrow(self.dim, self.prefix_len, x.shape[self.dim] - self.prefix_len))
        return torch.cat(parts, dim=self.dim)

    @property
    def chunk_data(self) -> List[torch.Tensor]:
        if self._chunk_data is not None:
            return self._chunk_data
        n = self._original_data.shape[self.dim]
        chunks = []
        for i in range(0, n, self.chunk_len):
            start = 0 if i == 0 else i - self.prefix_len
            stop = min(n, i + self.chunk_len)
            chunks.append(self._original_data.narrow(self.dim, start, stop - start))
        return chunks


def plan(hop: int, process_window: int, prefix_tokens: int):
    """(chunk_len, prefix_len) in samples: the window rounded down to whole hops (codec.py:135), the overlap in whole hops."""
    chunk_len = process_window // hop * hop
    prefix_len = prefix_tokens * hop
    if chunk_len <= prefix_len:
        raise ValueError(f"process_window ({process_window} samples) must exceed the overlap ({prefix_len} samples)")
    return chunk_len, prefix_len


def chunk_plan(frames, chunk_len: int, prefix_len: int, round_to: int = 1):
    """The chunks of a batch of recordings of ``frames[i]`` frames each, as a ctypes array of ``_capi.ChunkDesc`` (rec, row, start,
    frames, prefix, pad, last): ``ChunkData``'s geometry, computed by the library (l3ac_chunk_plan, host only; DESIGN.md section
    3.8).  Rows are numbered recording after recording.  Raises ValueError on bad arguments."""
    lib = _capi.load_library()
    vals = [int(v) for v in frames]
    host = (ctypes.c_int64 * max(len(vals), 1))(*vals)
    n = lib.l3ac_chunk_plan(host, len(vals), int(chunk_len), int(prefix_len), int(round_to), None, 0)
    if n < 0:
        raise ValueError(lib.l3ac_last_error().decode())
    desc = (_capi.ChunkDesc * n)()
    if lib.l3ac_chunk_plan(host, len(vals), int(chunk_len), int(prefix_len), int(round_to), desc, n) != n:
        raise ValueError(lib.l3ac_last_error().decode())
    return desc


def _chunk_groups(desc, chunks_per_call: int):
    """A plan's chunks as the groups of at most `chunks_per_call` chunk numbers that run in one ragged call each, shortest first: a
    ragged call computes the grid of its longest row, so every recording's short chunks (its first has no prefix, its last is what is
    left) share calls of their own size (3.5 % of a call).  The bits do not depend on the grouping."""
    order = sorted(range(len(desc)), key=lambda k: desc[k].frames)  # (stable)
    return [order[k0:k0 + chunks_per_call] for k0 in range(0, len(order), chunks_per_call)]


def _group_desc(desc, group, scale: int = 1):
    """The descriptors of one group with rows renumbered 0 .. len(group) - 1 (the rows of that group's call)."""
    out = (_capi.ChunkDesc * len(group))()
    for k, j in enumerate(group):
        d = desc[j]
        out[k] = _capi.ChunkDesc(d.rec, k, d.start * scale, d.frames * scale, d.prefix * scale, d.pad * scale, d.last)
    return out


def _chunk_cut(src: torch.Tensor, desc, rows: torch.Tensor, stream) -> None:
    """src (B, stride[, c]) -> rows (N, row_frames[, c]) on the device (l3ac_chunk_cut)."""
    c = src.shape[2] if src.dim() == 3 else 1
    _capi.check(_capi.load_library().l3ac_chunk_cut(src.data_ptr(), src.shape[0], src.stride(0) // c if src.shape[0] > 1 else src.shape[1],
                                                     c, desc, len(desc), rows.data_ptr(), rows.shape[0], rows.stride(0) // c, stream))


def _chunk_merge(rows: torch.Tensor, desc, dst: torch.Tensor, stream) -> None:
    """rows (N, row_frames[, c]) -> dst (B, out_frames[, c]), prefixes dropped, zeros after each recording (l3ac_chunk_merge)."""
    c = dst.shape[2] if dst.dim() == 3 else 1
    _capi.check(_capi.load_library().l3ac_chunk_merge(rows.data_ptr(), rows.shape[0], rows.stride(0) // c, c, desc, len(desc), dst.data_ptr(),
                                                       dst.shape[0], dst.shape[1], dst.shape[1], stream))
