"""What every call of the Python layer shares: argument checks, the ``validate=`` bracket, and the encode / decode of a block of rows.

``encode_audio`` / ``decode_audio``, the long calls and the stream sessions differ only in how rows get in and out of these (the chunk
movers of chunking.py, the state movers of streaming.py); errors are raised before any device work, in the order of the checks here.
"""
from __future__ import annotations

import ctypes
from contextlib import contextmanager

import torch

from . import _capi


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def int_list(values, count: int, lo: int, hi: int, what: str, of: str) -> list:
    """``values`` as ``count`` Python ints in lo..hi; raises ValueError otherwise.  Accepts a sequence, a NumPy array or a tensor (a CUDA
    tensor is copied to the host).  ``what`` names the argument and ``of`` what it has one entry for ("a batch of 3", "3 streams")."""
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().reshape(-1).tolist()
    try:
        seq = list(values)
        vals = [int(v) for v in seq]
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a sequence of {count} ints") from None
    if any(float(v) != int(v) for v in seq):
        raise ValueError(f"{what} must be integers")
    if len(vals) != count:
        raise ValueError(f"{what}: {len(vals)} entries for {of}")
    bad = [v for v in vals if not lo <= v <= hi]
    if bad:
        raise ValueError(f"{what}: {bad[0]} outside [{lo}, {hi}]")
    return vals


def end_flags(end, count: int) -> list:
    """``end=`` of a session's push as ``count`` bools: a bool (absent: False) for every stream, or one per stream."""
    if end is None or isinstance(end, bool):
        return [bool(end)] * count
    if isinstance(end, torch.Tensor):
        end = end.detach().cpu().reshape(-1).tolist()
    vals = [bool(v) for v in end]
    if len(vals) != count:
        raise ValueError(f"end: {len(vals)} entries for {count} streams")
    return vals


def window_args(mc, sample_rate: int, process_window, prefix_tokens, chunks_per_call, geometry):
    """The window arguments of the long calls and the codec's sessions -> (chunk_len in samples, prefix_tokens, chunks_per_call).
    ``prefix_tokens`` defaults to the attention window, ``chunks_per_call`` to 512 s of rows, and is capped at the 65,535 rows of one call.
    ``geometry(hop, process_window, prefix_tokens) -> (chunk_len, prefix_len)`` is the caller's own check of the window against the
    look-back (chunking.plan offline; a session takes any look-back): its errors come before ``chunks_per_call``'s."""
    prefix_tokens = mc.en_coder_window_size if prefix_tokens is None else prefix_tokens
    chunk_len, prefix_len = geometry(mc.hop_length, process_window, prefix_tokens)
    if chunks_per_call is None:
        chunks_per_call = max(1, (512 * sample_rate) // (chunk_len + prefix_len))
    if int(chunks_per_call) < 1:
        raise ValueError(f"chunks_per_call must be at least 1, got {chunks_per_call}")
    return chunk_len, int(prefix_tokens), min(int(chunks_per_call), 65535)


def check_codec_input(network, ctx, t: torch.Tensor, what: str, owner: str = ""):
    """What a codec call checks first, in this order: eval mode, the network on a GPU — on ``ctx`` still, when the caller is the session
    ``owner`` whose state belongs to that context (None: whichever context the network has) —, ``t`` on its device.  Returns the context."""
    if network.training:
        raise RuntimeError("call codec.network.eval() first: the training-mode quantiser injects noise "
                           "(reference vq/fsq.py:31,40-43), which this inference path does not implement")
    if ctx is None:
        ctx = network.context()
    elif network._ctx is not ctx or ctx.handle is None:
        raise RuntimeError(f"{owner}: the network was moved to another device or reloaded after this session was created; its "
                           "state belongs to the context it was created on: create a new session")
    if not t.is_cuda or t.device != network.device:
        raise RuntimeError(f"{what} is on {t.device} but the network is on {network.device}")
    return ctx


def refuse_grn_exact(network, what: str, instead: str) -> None:
    """Calls that batch chunks as ragged rows refuse the validation mode, whose normaliser would see the rows' padding."""
    if network.grn_exact:
        raise _capi.L3acError(f"{what}: this network evaluates the GRN normaliser per clip (grn_exact = True); ragged calls "
                              f"would include their padding: use {instead} per recording")


# ---- tensors ---------------------------------------------------------------------------------------------------------------------------
def row_stride(x: torch.Tensor) -> int:
    """Elements between the rows of a 2-D ``x`` as the library takes them: one row, or rows of nothing, have no stride of their own."""
    return x.stride(0) if x.shape[0] > 1 and x.shape[1] else max(x.shape[1], 1)


def contiguous_rows(x: torch.Tensor) -> torch.Tensor:
    """``x`` with unit stride along its last dimension (rows may stay strided); an empty tensor is left alone."""
    return x.contiguous() if x.stride(-1) != 1 and x.numel() else x


def zero_after(x: torch.Tensor, ends) -> torch.Tensor:
    """(B, T) with row i zero from ends[i] on: each clip of a ragged batch masked to its own end (sample_rate= with lengths=)."""
    keep = torch.arange(x.shape[1], device=x.device)[None, :] < torch.tensor(ends, device=x.device)[:, None]
    return torch.where(keep, x, 0.0)


# ---- validate= -------------------------------------------------------------------------------------------------------------------------
def _coop_check_before(ctx, what: str):
    """validate=True, before the call: an EARLIER call's expired polls that nobody has been told about must not disappear into this
    call's baseline (they would: l3ac_coop_timeout_count acknowledges what it reports).  Synchronises."""
    earlier = ctx.coop_timeout_pending()
    if earlier:
        ctx.coop_timeout_count()  # delivered by the exception below: fall back, re-zero the arrival counters
        raise _capi.L3acError(
            f"{what}(validate=True): an EARLIER call on this context lost {earlier} arrival poll(s) of the cooperative transformer "
            "kernel to its time limit; that call's outputs are invalid (every call since the last validated one is suspect). "
            "Nothing was run. The context now runs the one-workgroup form (same bits): repeat those calls")


def _raise_on_coop_timeout(ctx, what: str):
    lost = ctx.coop_timeout_pending()  # (synchronises)
    if lost:
        ctx.coop_timeout_count()  # delivered here: the context falls back to the one-workgroup form, counters re-zeroed
        raise _capi.L3acError(
            f"{what}: the cooperative transformer kernel lost {lost} arrival poll(s) to its time limit (its six workgroups per "
            "clip were not co-resident: another process or a CU mask on the device?); this call's outputs are invalid. The "
            "context now runs the one-workgroup form (same bits): repeat the call")


@contextmanager
def validated(ctx, what: str, validate: bool, bad_indices=None):
    """``validate=`` of the call ``what``, around its launches.  Set: synchronise before (raising, with nothing run, on an earlier call's
    lost cooperative launch) and after (raising on one of this call's); a caller that decodes indices passes ``bad_indices``, its message
    for a count of out-of-range indices, and the rise of the context's cumulative counter (read, never reset) over the body raises
    ValueError last.  An exception from the body skips the after-checks.  Not set: nothing, and nothing touches the device."""
    if not validate:
        yield
        return
    before = ctx.bad_index_count() if bad_indices else 0
    _coop_check_before(ctx, what)
    yield
    _raise_on_coop_timeout(ctx, what)
    if bad_indices:
        bad = ctx.bad_index_count() - before
        if bad:
            raise ValueError(bad_indices(bad))


# ---- rows through the codec ----------------------------------------------------------------------------------------------------------------
def encode_rows(ctx, rows: torch.Tensor, n: int, t: int, stride: int, lens, stream):
    """``n`` rows of ``t`` samples, ``stride`` floats apart, through the encode path -> fresh (q (n, T_tok, C), indices int32 (n, T_tok),
    level_indices (n, T_tok, D)), T_tok = ceil(t / hop).  ``lens`` None: the plain call; else the ragged call, row i ``lens[i]`` long."""
    mc, dev = ctx.mc, rows.device
    n_tok = -(-t // mc.hop_length)
    q = torch.empty((n, n_tok, mc.feature_dim), dtype=torch.float32, device=dev)
    idx = torch.empty((n, n_tok), dtype=torch.int32, device=dev)
    li = torch.empty((n, n_tok, len(mc.levels)), dtype=torch.float32, device=dev)
    if lens is None:
        _capi.check(ctx.lib.l3ac_encode(ctx.handle, rows.data_ptr(), n, t, stride, q.data_ptr(), idx.data_ptr(), li.data_ptr(), stream))
    else:
        _capi.check(ctx.lib.l3ac_encode_ragged(ctx.handle, rows.data_ptr(), n, t, stride, (ctypes.c_int32 * n)(*lens), q.data_ptr(),
                                               idx.data_ptr(), li.data_ptr(), stream))
    return q, idx, li


def decode_rows(ctx, rows: torch.Tensor, is_feature: bool, n: int, n_tok: int, lens, stream) -> torch.Tensor:
    """``n`` contiguous rows of ``n_tok`` tokens — features when ``is_feature``, else int32 indices — through the decode path -> a fresh
    wave (n, n_tok * hop).  ``lens`` None: the plain call; else the ragged call, row i ``lens[i]`` tokens long."""
    f_ptr, i_ptr = (rows.data_ptr(), None) if is_feature else (None, rows.data_ptr())
    wave = torch.empty((n, n_tok * ctx.mc.hop_length), dtype=torch.float32, device=rows.device)
    if lens is None:
        _capi.check(ctx.lib.l3ac_decode(ctx.handle, f_ptr, i_ptr, n, n_tok, wave.data_ptr(), stream))
    else:
        _capi.check(ctx.lib.l3ac_decode_ragged(ctx.handle, f_ptr, i_ptr, n, n_tok, (ctypes.c_int32 * n)(*lens), wave.data_ptr(), stream))
    return wave
