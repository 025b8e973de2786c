"""Quality metrics on the GPU (csrc/kernels/metrics.hip): ``stft``, ``log_mel``, ``mel_distance`` and
``signal_metrics``, and the per-device cache of the library's two fp32 tables (the window-folded DFT basis and the mel weights); and
speech intelligibility (csrc/kernels/stoi.hip, section 3.13): ``stoi`` and its host accessors."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _capi
from ._rows import contiguous_rows, int_list, row_stride, zero_after
from .resampling import resample, resample_length

DEFAULT_SCALES = ((256, 64, 20), (512, 128, 40), (1024, 256, 80), (2048, 512, 80))  # (n_fft, hop, n_mels) at 16 kHz

# bytes a call allocates above the minimum scratch: spectra of more frames per product (the results do not depend on it)
_EXTRA_SCRATCH = 64 << 20


def stft_frames(samples: int, hop: int) -> int:
    """Frames of a clip of ``samples`` samples: 1 + samples // hop.  Raises ValueError for samples < 1 or hop < 1."""
    n = _capi.load_library().l3ac_stft_frames(int(samples), int(hop))
    if n < 0:
        raise ValueError(_capi.load_library().l3ac_last_error().decode())
    return int(n)


def stft_basis(n_fft: int) -> torch.Tensor:
    """The library's window-folded DFT basis (n_fft + 2, n_fft) fp32 on the CPU: row 2k = w cos, row 2k + 1 = -w sin."""
    lib = _capi.load_library()
    n = lib.l3ac_stft_basis(int(n_fft), None, 0)
    if n < 0:
        raise ValueError(lib.l3ac_last_error().decode())
    host = torch.empty(n, dtype=torch.float32)
    lib.l3ac_stft_basis(int(n_fft), host.data_ptr(), n)
    return host.view(int(n_fft) + 2, int(n_fft))


def mel_weights(sample_rate: int, n_fft: int, n_mels: int) -> torch.Tensor:
    """The library's mel weights (n_mels, n_fft // 2 + 1) fp32 on the CPU: HTK scale, triangles, no normalisation."""
    lib = _capi.load_library()
    n = lib.l3ac_mel_weights(int(sample_rate), int(n_fft), int(n_mels), None, 0)
    if n < 0:
        raise ValueError(lib.l3ac_last_error().decode())
    host = torch.empty(n, dtype=torch.float32)
    lib.l3ac_mel_weights(int(sample_rate), int(n_fft), int(n_mels), host.data_ptr(), n)
    return host.view(int(n_mels), int(n_fft) // 2 + 1)


# (device, "basis", n_fft) / (device, "mel", sample_rate, n_fft, n_mels) / (device, "dct", n_mels, n_coeffs: mcd.py) /
# (device, "lpc_window", frame: lpc.py) -> device copy of the table
_tables = {}


def _table(device: torch.device, key: tuple, make) -> torch.Tensor:
    key = (device,) + key
    if key not in _tables:
        if torch.cuda.is_current_stream_capturing():
            # uploading the table would be a host -> device copy inside the graph; the eager warm-up call before capture fills the cache
            raise RuntimeError(f"metrics: the table {key[1:]} is not on {device} yet; run the call once outside stream capture (the "
                               "warm-up call before graph capture) to upload it")
        _tables[key] = make().to(device)
    return _tables[key]


def _check_params(sample_rate: int, n_fft: int, hop: int, n_mels: int) -> None:
    """The supported parameters, checked by the library before any device work: ValueError with its message."""
    lib = _capi.load_library()
    if lib.l3ac_mel_weights(sample_rate, n_fft, n_mels, None, 0) < 0 or lib.l3ac_mel_scratch_bytes(1, 1, n_fft, hop, n_mels) < 0:
        raise ValueError(lib.l3ac_last_error().decode())


def _audio(x, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{what} needs a CUDA tensor: l3ac_amd has no CPU path")
    if x.dim() != 2:
        raise ValueError(f"{what} must be (batch, samples), got {tuple(x.shape)}")
    if x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("empty audio")
    return contiguous_rows(x.to(torch.float32))


def _lengths(lengths, b: int, t: int):
    """``lengths=`` -> (Python ints or None, the ctypes array the library takes or None)."""
    if lengths is None:
        return None, None
    lens = int_list(lengths, b, 1, t, "lengths", f"a batch of {b}")  # (ragged_lengths of the package: the same check)
    return lens, (ctypes.c_int32 * b)(*lens)


def _extra_bytes(b: int, t: int, n_fft: int, hop: int, extra_scratch) -> int:
    """Bytes a call allocates above the minimum scratch."""
    if extra_scratch is None:  # the default, never more than the spectra of every frame row of both signals
        return min(_EXTRA_SCRATCH, 2 * b * (t // hop + n_fft // hop + 2) * (n_fft + 4) * 4)
    return max(0, int(extra_scratch))


def _scratch(dev, b: int, t: int, n_fft: int, hop: int, n_mels: int, extra_scratch) -> torch.Tensor:
    need = _capi.load_library().l3ac_mel_scratch_bytes(b, t, n_fft, hop, n_mels)
    if need < 0:
        raise ValueError(_capi.load_library().l3ac_last_error().decode())
    extra = _extra_bytes(b, t, n_fft, hop, extra_scratch)
    return torch.empty(int(need) + extra, dtype=torch.uint8, device=dev)  # (the caching allocator hands out 512-byte aligned blocks)


def _hop(n_fft: int, hop) -> int:
    return int(n_fft) // 4 if hop is None else int(hop)


@torch.no_grad()
def stft(audio: torch.Tensor, n_fft: int, hop: Optional[int] = None, lengths=None, extra_scratch=None) -> torch.Tensor:
    """(B, T) fp32 CUDA audio -> complex64 (B, 1 + T // hop, n_fft // 2 + 1): ``torch.stft(audio, n_fft, hop, n_fft,
    hann_window(n_fft), center=True, pad_mode="constant", onesided=True)`` transposed to frame-major, computed as one exact-fp32 matrix
    product per group of frames.  ``hop`` defaults to ``n_fft // 4``.  ``lengths``: B ints in 1..T; clip i has ``1 + lengths[i] // hop``
    frames, samples at or after its length are ignored and the frames after its own are zero.  A clip's bits do not depend on the batch
    it is in.  ``extra_scratch``: bytes to allocate above the minimum scratch (default 64 MiB, 0: the minimum; the result does not depend on it).
    No CPU path: CPU tensors raise.  Under stream capture a table that is not on the device yet raises (run one eager call first)."""
    n_fft, hop = int(n_fft), _hop(n_fft, hop)
    _check_params(1, n_fft, hop, 1)
    x = _audio(audio, "stft")
    b, t = x.shape
    lens, c_lens = _lengths(lengths, b, t)
    dev = x.device
    basis = _table(dev, ("basis", n_fft), lambda: stft_basis(n_fft))
    spec = torch.empty((b, stft_frames(t, hop), n_fft // 2 + 1, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        scratch = _scratch(dev, b, t, n_fft, hop, 1, extra_scratch)
        _capi.check(_capi.load_library().l3ac_stft(x.data_ptr(), b, t, row_stride(x), c_lens, n_fft, hop, basis.data_ptr(), spec.data_ptr(),
                                                   scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return torch.view_as_complex(spec)


@torch.no_grad()
def log_mel(audio: torch.Tensor, sample_rate: int = 16000, n_fft: int = 1024, hop: Optional[int] = None, n_mels: int = 80, lengths=None,
            extra_scratch=None):
    """(B, T) fp32 CUDA audio -> (B, 1 + T // hop, n_mels) fp32: log10(max(mel power, 1e-10)) of ``stft``'s frames, HTK mel scale without
    normalisation, triangular filters.  With ``lengths`` returns ``(log_mel, frames)``: the frame counts ``1 + lengths[i] // hop``
    (int32, on the CPU); the rows after a clip's own frames are zero.  Other arguments as ``stft``."""
    sample_rate, n_fft, hop, n_mels = int(sample_rate), int(n_fft), _hop(n_fft, hop), int(n_mels)
    _check_params(sample_rate, n_fft, hop, n_mels)
    x = _audio(audio, "log_mel")
    b, t = x.shape
    lens, c_lens = _lengths(lengths, b, t)
    dev = x.device
    basis = _table(dev, ("basis", n_fft), lambda: stft_basis(n_fft))
    weights = _table(dev, ("mel", sample_rate, n_fft, n_mels), lambda: mel_weights(sample_rate, n_fft, n_mels))
    out = torch.empty((b, stft_frames(t, hop), n_mels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        scratch = _scratch(dev, b, t, n_fft, hop, n_mels, extra_scratch)
        _capi.check(_capi.load_library().l3ac_log_mel(x.data_ptr(), b, t, row_stride(x), c_lens, n_fft, hop, basis.data_ptr(),
                                                      weights.data_ptr(), n_mels, out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                      torch.cuda.current_stream(dev).cuda_stream))
    if lens is None:
        return out
    return out, torch.tensor([1 + n // hop for n in lens], dtype=torch.int32)


def _pair(reference, estimate, what: str):
    r, e = _audio(reference, what), _audio(estimate, what)
    if r.shape != e.shape:
        raise ValueError(f"{what}: reference {tuple(r.shape)} and estimate {tuple(e.shape)} differ in shape")
    if r.device != e.device:
        raise RuntimeError(f"{what}: reference is on {r.device} but estimate is on {e.device}")
    return r, e


def _scales(scales) -> tuple:
    try:
        scales = DEFAULT_SCALES if scales is None else tuple(scales)
        scales = tuple((int(f), int(h), int(m)) for f, h, m in scales)
    except (TypeError, ValueError):
        raise ValueError("scales must be a sequence of (n_fft, hop, n_mels)") from None
    if not scales:
        raise ValueError("scales must name at least one (n_fft, hop, n_mels)")
    return scales


@torch.no_grad()
def mel_distance(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, scales=None, lengths=None, extra_scratch=None) -> dict:
    """Multi-scale log-mel distance of (B, T) fp32 CUDA pairs -> ``{"mel_distance": (B,) fp64 CUDA, "per_scale": (B, n_scales) fp64}``.
    At one scale ``(n_fft, hop, n_mels)`` the distance is the mean of ``|log_mel(reference) - log_mel(estimate)|`` over the clip's own
    cells, taken in fp64 from ``log_mel``'s fp32 cells and summed in a fixed order; ``"mel_distance"`` is ``per_scale.mean(dim=1)``.
    ``scales`` defaults to ``DEFAULT_SCALES`` (made for 16 kHz).  ``lengths``: the pairs' common lengths, as in ``stft``."""
    sample_rate, scales = int(sample_rate), _scales(scales)
    for n_fft, hop, n_mels in scales:
        _check_params(sample_rate, n_fft, hop, n_mels)
    r, e = _pair(reference, estimate, "mel_distance")
    b, t = r.shape
    lens, c_lens = _lengths(lengths, b, t)
    dev = r.device
    lib = _capi.load_library()
    rows = torch.empty((len(scales), b), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for i, (n_fft, hop, n_mels) in enumerate(scales):
            basis = _table(dev, ("basis", n_fft), lambda: stft_basis(n_fft))
            weights = _table(dev, ("mel", sample_rate, n_fft, n_mels), lambda: mel_weights(sample_rate, n_fft, n_mels))
            scratch = _scratch(dev, b, t, n_fft, hop, n_mels, extra_scratch)
            _capi.check(lib.l3ac_mel_distance(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, n_fft, hop, n_mels,
                                              basis.data_ptr(), weights.data_ptr(), rows[i].data_ptr(), scratch.data_ptr(), scratch.numel(), stream))
    per_scale = rows.t().contiguous()
    return {"mel_distance": per_scale.mean(dim=1), "per_scale": per_scale}


@torch.no_grad()
def signal_metrics(reference: torch.Tensor, estimate: torch.Tensor, lengths=None) -> dict:
    """Time-domain metrics of (B, T) fp32 CUDA pairs, each clip over its own samples, in fp64 -> ``{"mse", "snr_db", "si_sdr_db"}``,
    each (B,) fp64 CUDA.  ``si_sdr_db`` is the zero-mean scale-invariant SDR of Le Roux et al.; the residual energies are summed
    directly in a second pass, so 80 dB pairs keep their digits.  A zero denominator gives +inf, 0 / 0 gives nan."""
    r, e = _pair(reference, estimate, "signal_metrics")
    b, t = r.shape
    lens, c_lens = _lengths(lengths, b, t)
    dev = r.device
    out = torch.empty((b, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        scratch = torch.empty(4 * b, dtype=torch.uint8, device=dev)
        _capi.check(_capi.load_library().l3ac_signal_metrics(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens,
                                                             out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                             torch.cuda.current_stream(dev).cuda_stream))
    return {"mse": out[:, 0].contiguous(), "snr_db": out[:, 1].contiguous(), "si_sdr_db": out[:, 2].contiguous()}


# ---- speech intelligibility (csrc/kernels/stoi.hip) -----------------------------------------------------------
STOI_RATE = 10000  # the rate STOI and ESTOI are defined at


def stoi_frames(samples: int) -> int:
    """Analysis frames of a clip of ``samples`` samples at 10 kHz: 0 up to 256 samples, else ceil((samples - 256) / 128); ``stoi``
    then has one spectral frame fewer than the frames it keeps.  Raises ValueError for samples < 1."""
    n = _capi.load_library().l3ac_stoi_frames(int(samples))
    if n < 0:
        raise ValueError(_capi.load_library().l3ac_last_error().decode())
    return int(n)


def stoi_basis() -> torch.Tensor:
    """The library's window-folded STOI basis (514, 256) fp32 on the CPU: row 2k = w cos, row 2k + 1 = -w sin of bin k of a 512-point
    DFT, w = hanning(258)[1:-1]; row 0 is the window."""
    lib = _capi.load_library()
    n = lib.l3ac_stoi_basis(None, 0)
    host = torch.empty(n, dtype=torch.float32)
    lib.l3ac_stoi_basis(host.data_ptr(), n)
    return host.view(514, 256)


def stoi_bands() -> list:
    """The 15 third-octave bands as runs of bins ``[(lo, hi), ...]`` (hi exclusive) of the 512-point DFT at 10 kHz."""
    runs = (ctypes.c_int32 * 30)()
    _capi.check(_capi.load_library().l3ac_stoi_bands(runs))
    return [(int(runs[2 * i]), int(runs[2 * i + 1])) for i in range(15)]


@torch.no_grad()
def stoi(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, lengths=None, return_bands: bool = False,
         extra_scratch=None) -> dict:
    """STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of (B, T) fp32 CUDA pairs -> ``{"stoi": (B,) fp64 CUDA, "estoi": (B,) fp64
    CUDA, "frames": (B,) int32 CUDA}``, with the published implementations' constants (10 kHz, frames of 256 at hop 128, 15
    third-octave bands from 150 Hz, segments of 30 frames, -15 dB clipping, 40 dB range).  ``frames`` is the number of spectral
    frames left after the reference's silent frames are removed; below 30 there is no segment and both values are exactly 1e-5, the
    published convention.  When ``sample_rate`` is not 10000 both signals go through this library's ``resample`` first (each clip as
    it would be alone), not through the Matlab-style resampler of ``pystoi``: for such inputs the values differ from that package's
    in the later digits.  ``lengths``: the pairs' common lengths at ``sample_rate``, as in ``stft``.  ``return_bands`` adds
    ``"bands_reference"`` and ``"bands_estimate"``, (B, stoi_frames(T at 10 kHz) - 1, 15) fp32, zero after a clip's own frames.
    A clip's bits do not depend on the batch it is in; ``extra_scratch`` as in ``stft``.  No CPU path: CPU tensors raise."""
    sample_rate = int(sample_rate)
    if sample_rate != STOI_RATE:
        resample_length(sample_rate, STOI_RATE, 1)  # unsupported rates raise before any device work
    r, e = _pair(reference, estimate, "stoi")
    b, t = r.shape
    lens, c_lens = _lengths(lengths, b, t)
    if sample_rate != STOI_RATE:
        given = [t] * b if lens is None else lens
        r = resample(zero_after(r, given), sample_rate, STOI_RATE)
        e = resample(zero_after(e, given), sample_rate, STOI_RATE)
        t = r.shape[1]
        lens, c_lens = _lengths([resample_length(sample_rate, STOI_RATE, n) for n in given], b, t)
    dev = r.device
    lib = _capi.load_library()
    basis = _table(dev, ("stoi_basis",), stoi_basis)
    need = lib.l3ac_stoi_scratch_bytes(b, t)
    if need < 0:
        raise ValueError(lib.l3ac_last_error().decode())
    t_max = max(stoi_frames(t) - 1, 0)
    if extra_scratch is None:  # the default, never more than the spectra of every frame row of both signals
        extra = min(_EXTRA_SCRATCH, 2 * b * (t_max + 3) * 516 * 4)
    else:
        extra = max(0, int(extra_scratch))
    out = torch.empty((b, 2), dtype=torch.float64, device=dev)
    frames = torch.empty(b, dtype=torch.int32, device=dev)
    bands = torch.empty((2, b, t_max, 15), dtype=torch.float32, device=dev) if return_bands else None
    with torch.cuda.device(dev):
        scratch = torch.empty(int(need) + extra, dtype=torch.uint8, device=dev)
        _capi.check(lib.l3ac_stoi(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, basis.data_ptr(), out.data_ptr(),
                                  frames.data_ptr(), None if bands is None or not t_max else bands.data_ptr(), scratch.data_ptr(),
                                  scratch.numel(), torch.cuda.current_stream(dev).cuda_stream))
    result = {"stoi": out[:, 0].contiguous(), "estoi": out[:, 1].contiguous(), "frames": frames}
    if return_bands:
        result["bands_reference"], result["bands_estimate"] = bands[0], bands[1]
    return result
