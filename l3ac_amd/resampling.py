"""Sample-rate conversion on the GPU: ``resample`` (scipy.signal.resample_poly's defaults as one HIP kernel, csrc/kernels/resample.hip),
``resample_length`` and the per-device cache of the library's polyphase filter banks, which ``StreamResampler`` (streaming.py) shares."""
from __future__ import annotations

from typing import Optional

import torch

from . import _capi
from ._rows import contiguous_rows, row_stride


def resample_length(orig_sr: int, target_sr: int, n_in: int) -> int:
    """Samples out of ``resample`` for ``n_in`` samples in: ceil(n_in * up / down).  Raises ValueError for rates the library does
    not support (non-positive, or a reduced max(up, down) above 1024)."""
    n = _capi.load_library().l3ac_resample_length(int(orig_sr), int(target_sr), int(n_in))
    if n < 0:
        raise ValueError(_capi.load_library().l3ac_last_error().decode())
    return int(n)


_banks = {}  # (device, orig_sr, target_sr) -> device copy of the library's polyphase filter bank


def _resample_bank(device: torch.device, orig_sr: int, target_sr: int) -> Optional[torch.Tensor]:
    key = (device, orig_sr, target_sr)
    if key in _banks:
        return _banks[key]
    lib = _capi.load_library()
    n = lib.l3ac_resample_bank(orig_sr, target_sr, None, 0)
    if n < 0:
        raise ValueError(lib.l3ac_last_error().decode())
    if n > 0 and torch.cuda.is_current_stream_capturing():
        # uploading the bank would be a host -> device copy inside the graph; the eager warm-up call before capture fills the cache
        raise RuntimeError(f"resample {orig_sr} -> {target_sr}: this rate pair's filter bank is not on {device} yet; run the call "
                           "once outside stream capture (the warm-up call before graph capture) to upload it")
    bank = None
    if n > 0:
        host = torch.empty(n, dtype=torch.float32)
        lib.l3ac_resample_bank(orig_sr, target_sr, host.data_ptr(), n)
        bank = host.to(device)
    _banks[key] = bank
    return bank


@torch.no_grad()
def resample(audio: torch.Tensor, orig_sr: int, target_sr: int) -> torch.Tensor:
    """(B, T) fp32 CUDA audio at ``orig_sr`` -> (B, resample_length(orig_sr, target_sr, T)) at ``target_sr``, on the GPU.
    ``scipy.signal.resample_poly(audio, up, down, axis=-1)`` with its defaults (Kaiser-windowed sinc, beta 5, zero padding at
    both ends; up / down = target_sr / orig_sr reduced), in fp32: each output is one fmaf chain in a fixed tap order, so a clip's
    bits do not depend on the batch it is in.  Equal rates return a copy.  No CPU path: CPU tensors raise.  Each rate pair's
    filter bank is uploaded once per device and cached; under stream capture a pair that has not run on the device yet raises."""
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if not isinstance(audio, torch.Tensor) or not audio.is_cuda:
        raise RuntimeError("resample needs a CUDA tensor: l3ac_amd has no CPU path")
    if audio.dim() != 2:
        raise ValueError(f"audio must be (batch, samples), got {tuple(audio.shape)}")
    b, t = audio.shape
    if b == 0 or t == 0:
        raise ValueError("empty audio")
    n_out = resample_length(orig_sr, target_sr, t)  # validates the rates before any device work
    x = contiguous_rows(audio.to(torch.float32))
    dev = x.device
    bank = _resample_bank(dev, orig_sr, target_sr)
    y = torch.empty((b, n_out), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.load_library().l3ac_resample(
            x.data_ptr(), b, t, row_stride(x), orig_sr, target_sr, None if bank is None else bank.data_ptr(),
            y.data_ptr(), n_out, torch.cuda.current_stream(dev).cuda_stream))
    return y
