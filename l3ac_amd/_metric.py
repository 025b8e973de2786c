"""What the metric modules share (metrics, loudness, pitch, align, mcd, lpc, sdr, bands): the library's host values and
tables, the checks of ``(batch, samples)`` audio and of ``lengths=``, the per-device cache of uploaded tables, the scratch allocation and
the result columns.  Each module's parameters and the order of its checks are its own."""
from __future__ import annotations

import ctypes

import torch

from . import _capi
from ._rows import contiguous_rows, int_list

# bytes a call allocates above the minimum scratch: spectra of more frames per product (the results do not depend on it)
EXTRA_SCRATCH = 64 << 20


def lib_value(fn: str, *args) -> int:
    """The library's ``fn(*args)``: a size, a count or a status, never negative.  A negative one raises ValueError with its message."""
    lib = _capi.load_library()
    n = getattr(lib, fn)(*args)
    if n < 0:
        raise ValueError(lib.l3ac_last_error().decode())
    return int(n)


def host_table(fn: str, dtype: torch.dtype, *args) -> torch.Tensor:
    """A host table of the library, flat, on the CPU: ``fn(*args, None, 0)`` is its length, ``fn(*args, buffer, length)`` fills it."""
    n = lib_value(fn, *args, None, 0)
    host = torch.empty(n, dtype=dtype)
    lib_value(fn, *args, host.data_ptr(), n)
    return host


# (device, "basis", n_fft) / (device, "mel", sample_rate, n_fft, n_mels) / (device, "stoi_basis") / (device, "dct", n_mels, n_coeffs) /
# (device, "lpc_window", frame) / (device, "bands_twiddles", n_fft) / (device, "band_weights", sample_rate, n_fft, centres, widths) /
# (device, "sii_importance", importances...) -> device copy of the table; every metric module's tables live here
tables = {}


def table(device: torch.device, key: tuple, make) -> torch.Tensor:
    key = (device,) + key
    if key not in tables:
        if torch.cuda.is_current_stream_capturing():
            # uploading the table would be a host -> device copy inside the graph; the eager warm-up call before capture fills the cache
            raise RuntimeError(f"metrics: the table {key[1:]} is not on {device} yet; run the call once outside stream capture (the "
                               "warm-up call before graph capture) to upload it")
        tables[key] = make().to(device)
    return tables[key]


def check_mel_params(sample_rate: int, n_fft: int, hop: int, n_mels: int) -> None:
    """The supported parameters of the mel front end (``log_mel``, ``mfcc``), checked by the library before any device work: ValueError
    with its message."""
    lib_value("l3ac_mel_weights", sample_rate, n_fft, n_mels, None, 0)
    lib_value("l3ac_mel_scratch_bytes", 1, 1, n_fft, hop, n_mels)


def shape(x, what: str, empty_ok: bool = False):
    """``(batch, samples)`` of a tensor, checked before its device is (ValueError); None for what is not a tensor."""
    if not isinstance(x, torch.Tensor):
        return None
    if x.dim() != 2:
        raise ValueError(f"{what} must be (batch, samples), got {tuple(x.shape)}")
    if not empty_ok and (x.shape[0] == 0 or x.shape[1] == 0):
        raise ValueError("empty audio")
    return tuple(x.shape)


def audio(x, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{what} needs a CUDA tensor: l3ac_amd has no CPU path")
    shape(x, what)
    return contiguous_rows(x.to(torch.float32))


def pair(reference, estimate, what: str):
    r, e = audio(reference, what), audio(estimate, what)
    if r.shape != e.shape:
        raise ValueError(f"{what}: reference {tuple(r.shape)} and estimate {tuple(e.shape)} differ in shape")
    if r.device != e.device:
        raise RuntimeError(f"{what}: reference is on {r.device} but estimate is on {e.device}")
    return r, e


def lengths(lengths, b: int, t: int):
    """``lengths=`` -> (Python ints or None, the ctypes array the library takes or None)."""
    if lengths is None:
        return None, None
    lens = int_list(lengths, b, 1, t, "lengths", f"a batch of {b}")  # (ragged_lengths of the package: the same check)
    return lens, (ctypes.c_int32 * b)(*lens)


def scratch(dev, need: int, extra_scratch=0, rows: int = 0, row_floats: int = 0) -> torch.Tensor:
    """``need`` bytes on ``dev`` plus ``extra_scratch``.  ``None`` is the default of the entries that walk their spectra in groups of
    frame rows: never more than ``rows`` rows of ``row_floats`` fp32 of both signals, at most 64 MiB; nothing for the others."""
    if extra_scratch is None:
        extra = min(EXTRA_SCRATCH, 2 * rows * row_floats * 4)
    else:
        extra = max(0, int(extra_scratch))
    return torch.empty(int(need) + extra, dtype=torch.uint8, device=dev)  # (the caching allocator hands out 512-byte aligned blocks)


def mel_scratch(dev, need: int, b: int, t: int, n_fft: int, hop: int, extra_scratch) -> torch.Tensor:
    """``scratch`` of the entries built on the STFT product (``stft``, ``log_mel``, ``mel_distance``, ``mfcc``): the default extra room
    holds the spectra of every frame row."""
    return scratch(dev, need, extra_scratch, b * (t // hop + n_fft // hop + 2), n_fft + 4)


def columns(values: torch.Tensor, names) -> dict:
    """``{name: values[..., i]}``, each contiguous."""
    return {name: values[..., i].contiguous() for i, name in enumerate(names)}


def stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream
