"""Quality metrics on the GPU (csrc/kernels/metrics.hip): ``stft``, ``log_mel``, ``mel_distance`` and
``signal_metrics``, and the library's two fp32 tables (the window-folded DFT basis and the mel weights; ``_metric.py`` caches the device copies); and
speech intelligibility (csrc/kernels/stoi.hip, section 3.13): ``stoi`` and its host accessors."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _capi, _metric
from ._metric import check_mel_params as _check_params, tables as _tables  # noqa: F401 (the package and the tests use these names)
from ._rows import row_stride, zero_after
from .resampling import resample, resample_length

DEFAULT_SCALES = ((256, 64, 20), (512, 128, 40), (1024, 256, 80), (2048, 512, 80))  # (n_fft, hop, n_mels) at 16 kHz


def stft_frames(samples: int, hop: int) -> int:
    """Frames of a clip of ``samples`` samples: 1 + samples // hop.  Raises ValueError for samples < 1 or hop < 1."""
    return _metric.lib_value("l3ac_stft_frames", int(samples), int(hop))


def stft_basis(n_fft: int) -> torch.Tensor:
    """The library's window-folded DFT basis (n_fft + 2, n_fft) fp32 on the CPU: row 2k = w cos, row 2k + 1 = -w sin."""
    return _metric.host_table("l3ac_stft_basis", torch.float32, int(n_fft)).view(int(n_fft) + 2, int(n_fft))


def mel_weights(sample_rate: int, n_fft: int, n_mels: int) -> torch.Tensor:
    """The library's mel weights (n_mels, n_fft // 2 + 1) fp32 on the CPU: HTK scale, triangles, no normalisation."""
    return _metric.host_table("l3ac_mel_weights", torch.float32, int(sample_rate), int(n_fft), int(n_mels)).view(int(n_mels), int(n_fft) // 2 + 1)


def _scratch(dev, b: int, t: int, n_fft: int, hop: int, n_mels: int, extra_scratch) -> torch.Tensor:
    need = _metric.lib_value("l3ac_mel_scratch_bytes", b, t, n_fft, hop, n_mels)
    return _metric.mel_scratch(dev, need, b, t, n_fft, hop, extra_scratch)


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
    x = _metric.audio(audio, "stft")
    b, t = x.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = x.device
    basis = _metric.table(dev, ("basis", n_fft), lambda: stft_basis(n_fft))
    spec = torch.empty((b, stft_frames(t, hop), n_fft // 2 + 1, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        scratch = _scratch(dev, b, t, n_fft, hop, 1, extra_scratch)
        _capi.check(_capi.load_library().l3ac_stft(x.data_ptr(), b, t, row_stride(x), c_lens, n_fft, hop, basis.data_ptr(), spec.data_ptr(),
                                                   scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return torch.view_as_complex(spec)


@torch.no_grad()
def log_mel(audio: torch.Tensor, sample_rate: int = 16000, n_fft: int = 1024, hop: Optional[int] = None, n_mels: int = 80, lengths=None,
            extra_scratch=None):
    """(B, T) fp32 CUDA audio -> (B, 1 + T // hop, n_mels) fp32: log10(max(mel power, 1e-10)) of ``stft``'s frames, HTK mel scale without
    normalisation, triangular filters.  With ``lengths`` returns ``(log_mel, frames)``: the frame counts ``1 + lengths[i] // hop``
    (int32, on the CPU); the rows after a clip's own frames are zero.  Other arguments as ``stft``."""
    sample_rate, n_fft, hop, n_mels = int(sample_rate), int(n_fft), _hop(n_fft, hop), int(n_mels)
    _check_params(sample_rate, n_fft, hop, n_mels)
    x = _metric.audio(audio, "log_mel")
    b, t = x.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = x.device
    basis = _metric.table(dev, ("basis", n_fft), lambda: stft_basis(n_fft))
    weights = _metric.table(dev, ("mel", sample_rate, n_fft, n_mels), lambda: mel_weights(sample_rate, n_fft, n_mels))
    out = torch.empty((b, stft_frames(t, hop), n_mels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        scratch = _scratch(dev, b, t, n_fft, hop, n_mels, extra_scratch)
        _capi.check(_capi.load_library().l3ac_log_mel(x.data_ptr(), b, t, row_stride(x), c_lens, n_fft, hop, basis.data_ptr(),
                                                      weights.data_ptr(), n_mels, out.data_ptr(), scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    if lens is None:
        return out
    return out, torch.tensor([1 + n // hop for n in lens], dtype=torch.int32)


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
    r, e = _metric.pair(reference, estimate, "mel_distance")
    b, t = r.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = r.device
    lib = _capi.load_library()
    rows = torch.empty((len(scales), b), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = _metric.stream(dev)
        for i, (n_fft, hop, n_mels) in enumerate(scales):
            basis = _metric.table(dev, ("basis", n_fft), lambda: stft_basis(n_fft))
            weights = _metric.table(dev, ("mel", sample_rate, n_fft, n_mels), lambda: mel_weights(sample_rate, n_fft, n_mels))
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
    r, e = _metric.pair(reference, estimate, "signal_metrics")
    b, t = r.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = r.device
    out = torch.empty((b, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, 4 * b)
        _capi.check(_capi.load_library().l3ac_signal_metrics(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens,
                                                             out.data_ptr(), scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return _metric.columns(out, ("mse", "snr_db", "si_sdr_db"))


# ---- speech intelligibility (csrc/kernels/stoi.hip) -----------------------------------------------------------
STOI_RATE = 10000  # the rate STOI and ESTOI are defined at


def stoi_frames(samples: int) -> int:
    """Analysis frames of a clip of ``samples`` samples at 10 kHz: 0 up to 256 samples, else ceil((samples - 256) / 128); ``stoi``
    then has one spectral frame fewer than the frames it keeps.  Raises ValueError for samples < 1."""
    return _metric.lib_value("l3ac_stoi_frames", int(samples))


def stoi_basis() -> torch.Tensor:
    """The library's window-folded STOI basis (514, 256) fp32 on the CPU: row 2k = w cos, row 2k + 1 = -w sin of bin k of a 512-point
    DFT, w = hanning(258)[1:-1]; row 0 is the window."""
    return _metric.host_table("l3ac_stoi_basis", torch.float32).view(514, 256)


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
    r, e = _metric.pair(reference, estimate, "stoi")
    b, t = r.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    if sample_rate != STOI_RATE:
        given = [t] * b if lens is None else lens
        r = resample(zero_after(r, given), sample_rate, STOI_RATE)
        e = resample(zero_after(e, given), sample_rate, STOI_RATE)
        t = r.shape[1]
        lens, c_lens = _metric.lengths([resample_length(sample_rate, STOI_RATE, n) for n in given], b, t)
    dev = r.device
    lib = _capi.load_library()
    basis = _metric.table(dev, ("stoi_basis",), stoi_basis)
    need = _metric.lib_value("l3ac_stoi_scratch_bytes", b, t)
    t_max = max(stoi_frames(t) - 1, 0)
    out = torch.empty((b, 2), dtype=torch.float64, device=dev)
    frames = torch.empty(b, dtype=torch.int32, device=dev)
    bands = torch.empty((2, b, t_max, 15), dtype=torch.float32, device=dev) if return_bands else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch, b * (t_max + 3), 516)  # (the default: every frame row of both signals)
        _capi.check(lib.l3ac_stoi(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, basis.data_ptr(), out.data_ptr(),
                                  frames.data_ptr(), None if bands is None or not t_max else bands.data_ptr(), scratch.data_ptr(),
                                  scratch.numel(), _metric.stream(dev)))
    result = dict(_metric.columns(out, ("stoi", "estoi")), frames=frames)
    if return_bands:
        result["bands_reference"], result["bands_estimate"] = bands[0], bands[1]
    return result
