"""Critical-band measures on the GPU (csrc/kernels/bands.hip): the fp64 spectrum of the un-centred, windowed frames
of ``lpc`` (``frame_spectrum``), the energies of band filters on it (``band_energies``) and the three measures of speech-codec evaluation
built on them — frequency-weighted segmental SNR, weighted spectral slope distance, log-spectral distance (``band_metrics``) — with the
host accessors of the band table and the filter weights."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _capi, _metric
from ._rows import row_stride
from .lpc import WINDOWS, _window, lpc_defaults, lpc_frames

MAX_FRAMES = 16384  # the most frames a pair of ``band_metrics`` may have


def critical_bands() -> tuple:
    """The default band table ``(centre_hz, bandwidth_hz)``, (25,) fp64 each on the CPU: the 25 critical bands of the published measures,
    50 Hz to 3597.63 Hz.  The table stops below 4 kHz whatever the sample rate: a caller who wants the bands of 4-8 kHz weighted passes a
    table of their own as ``bands=``."""
    table = _metric.host_table("l3ac_bands_critical", torch.float64)
    return table[:25].clone(), table[25:].clone()


def _band_table(bands) -> tuple:
    """``bands=`` -> (centres, widths) as tuples of Python floats; ValueError for what is not two equally long sequences of numbers."""
    if bands is None:
        bands = critical_bands()
    try:
        centre, width = bands
        centre = tuple(float(v) for v in (centre.tolist() if isinstance(centre, torch.Tensor) else centre))
        width = tuple(float(v) for v in (width.tolist() if isinstance(width, torch.Tensor) else width))
    except (TypeError, ValueError):
        raise ValueError("bands must be a pair (centre_hz, bandwidth_hz) of equally long sequences of numbers") from None
    if len(centre) != len(width):
        raise ValueError(f"bands: {len(centre)} centres but {len(width)} bandwidths")
    return centre, width


def _weights_host(rate: int, n_fft: int, centre: tuple, width: tuple) -> torch.Tensor:
    nb = len(centre)
    c, w = (ctypes.c_double * nb)(*centre), (ctypes.c_double * nb)(*width)
    return _metric.host_table("l3ac_band_weights", torch.float64, rate, n_fft, nb, c, w).reshape(nb, n_fft // 2)


def band_weights(sample_rate: int = 16000, n_fft: int = 1024, bands=None) -> torch.Tensor:
    """The band filters (bands, n_fft / 2) fp64 on the CPU.  With ``h = n_fft / 2``, ``f0 = centre / (fs / 2) h`` and ``bw = bandwidth /
    (fs / 2) h``: ``W[i][k] = exp(-11 ((k - floor(f0)) / bw)^2 + ln(min_j bandwidth_j) - ln(bandwidth_i))``, 0 where that is at or below
    ``exp(-30 / (2 * 2.303))``; designed in long double and rounded once.  ``bands``: ``(centre_hz, bandwidth_hz)``, 2 to 64 bands;
    default ``critical_bands()``.  Raises ValueError for a centre at or above ``fs / 2``, a bandwidth that is not positive, or a band
    without a non-zero weight."""
    centre, width = _band_table(bands)
    return _weights_host(_int(sample_rate, "sample_rate"), _int(n_fft, "n_fft"), centre, width)


def _int(v, name: str) -> int:
    try:
        return int(v)
    except (TypeError, ValueError):
        raise ValueError(f"bands: {name} must be an integer") from None


def _check_params(sample_rate, frame=None, hop=None, n_fft=None, window="hann", bands=False) -> tuple:
    """The supported parameters, checked by the library before any device work: ValueError with its message.  Returns the resolved
    ``(sample_rate, frame, hop, n_fft)`` and, where ``bands`` is not False, the band table ``(centres, widths)``."""
    _, d_frame, _ = lpc_defaults(sample_rate)
    rate = int(sample_rate)
    frame = d_frame if frame is None else _int(frame, "frame")
    hop = frame // 4 if hop is None else _int(hop, "hop")
    if n_fft is None:
        n_fft = _metric.lib_value("l3ac_bands_default_fft", frame)
    n_fft = _int(n_fft, "n_fft")
    _metric.lib_value("l3ac_frame_spectrum_scratch_bytes", 1, 1, frame, hop, n_fft)
    if window not in WINDOWS:
        raise ValueError(f"bands: window {window!r} is not one of {WINDOWS}")
    if bands is False:
        return rate, frame, hop, n_fft
    centre, width = _band_table(bands)
    _metric.lib_value("l3ac_band_weights", rate, n_fft, len(centre), (ctypes.c_double * len(centre))(*centre),
                      (ctypes.c_double * len(width))(*width), None, 0)
    return rate, frame, hop, n_fft, (centre, width)


def _twiddles(dev, n_fft: int) -> torch.Tensor:
    return _metric.table(dev, ("bands_twiddles", n_fft), lambda: _metric.host_table("l3ac_bands_twiddles", torch.float64, n_fft))


def _weights(dev, rate: int, n_fft: int, table: tuple) -> torch.Tensor:
    return _metric.table(dev, ("band_weights", rate, n_fft) + table, lambda: _weights_host(rate, n_fft, *table))


def _lengths(lengths, shape):
    return (None, None) if shape is None else _metric.lengths(lengths, *shape)


@torch.no_grad()
def frame_spectrum(audio: torch.Tensor, sample_rate: int = 16000, frame: Optional[int] = None, hop: Optional[int] = None,
                   n_fft: Optional[int] = None, window: str = "hann", lengths=None, detail: bool = False, extra_scratch=None) -> dict:
    """The short-time spectrum of (B, T) fp32 CUDA mono clips on ``lpc``'s frames -> ``{"spectrum": (B, F, n_fft / 2) complex128, "frames":
    (B,) int32}`` on the device, ``F = lpc_frames(T, frame, hop)``.  Frame t reads samples ``[t hop, t hop + frame)`` of its clip and
    nothing else (no padding, no centring); the samples times the fp32 window (``"hann"``: ``lpc_window``; ``"rect"``: ones) are exact in
    fp64 and are transformed by a complex radix-2 decimation-in-time FFT of ``n_fft`` points in fp64 on the library's twiddle table
    (section 3.22 states the network: every bin is one fixed expression tree).  Bins ``0 .. n_fft / 2 - 1`` are kept; the Nyquist bin is
    dropped.  ``frame`` in 2..2048; ``n_fft`` a power of two in 16..4096, at least ``frame`` (default: the smallest power of two >= 2
    frame); ``hop >= 1``; the defaults of ``frame`` and ``hop`` are ``lpc_defaults(sample_rate)``'s.  ``detail=True`` adds ``"power"``
    (``re re + im im``), ``"magnitude"`` (its correctly rounded square root), both (B, F, n_fft / 2) fp64, and ``"magnitude_sum"`` (B, F):
    the sum of the magnitudes in the order ``band_metrics`` normalises with.  ``lengths``: B ints in 1..T; samples at or after a clip's
    length are ignored, whatever they hold, and the rows at and after a clip's own frames hold NaN.  A clip's bits do not depend on the
    batch it is in; ``extra_scratch``: bytes to allocate above the minimum scratch (the result does not depend on it).  Capturable after
    one eager call (the window and the twiddles).  No CPU path: CPU tensors raise."""
    rate, n, hop, n_fft = _check_params(sample_rate, frame, hop, n_fft, window)
    lens, c_lens = _lengths(lengths, _metric.shape(audio, "frame_spectrum"))
    x = _metric.audio(audio, "frame_spectrum")
    b, t = x.shape
    dev = x.device
    h = n_fft // 2
    need = _metric.lib_value("l3ac_frame_spectrum_scratch_bytes", b, t, n, hop, n_fft)
    f_max = lpc_frames(t, n, hop)
    win, tw = _window(dev, window, n), _twiddles(dev, n_fft)
    spec = torch.empty((b, f_max, h, 2), dtype=torch.float64, device=dev)
    power = torch.empty((b, f_max, h), dtype=torch.float64, device=dev) if detail else None
    mag = torch.empty((b, f_max, h), dtype=torch.float64, device=dev) if detail else None
    total = torch.empty((b, f_max), dtype=torch.float64, device=dev) if detail else None
    frames = torch.empty(b, dtype=torch.int32, device=dev)
    ptr = lambda v: v.data_ptr() if v is not None and f_max else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_frame_spectrum(x.data_ptr(), row_stride(x), b, t, c_lens, n, hop, n_fft,
                                                             None if win is None else win.data_ptr(), tw.data_ptr(), ptr(spec), ptr(power), ptr(mag),
                                                             ptr(total), frames.data_ptr(), scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    res = {"spectrum": torch.view_as_complex(spec), "frames": frames}
    if detail:
        res.update(power=power, magnitude=mag, magnitude_sum=total)
    return res


@torch.no_grad()
def band_energies(audio: torch.Tensor, sample_rate: int = 16000, frame: Optional[int] = None, hop: Optional[int] = None,
                  n_fft: Optional[int] = None, window: str = "hann", lengths=None, bands=None, extra_scratch=None) -> dict:
    """The band filters on ``frame_spectrum``'s frames -> ``{"power", "magnitude": (B, F, bands) fp64, "frames": (B,) int32}`` on the
    device: per frame and band the sum of ``band_weights(sample_rate, n_fft, bands)[i][k]`` times the bin's power, and times its
    magnitude, over the band's run of non-zero weights in increasing k.  ``power`` is what the weighted spectral slope measure floors at
    1e-10 and takes to dB; ``magnitude`` is the frequency-weighted SNR's band sum without its normalisation.  Other parameters, the bit
    guarantee and stream capture as ``frame_spectrum`` (one more table: the weights)."""
    rate, n, hop, n_fft, table = _check_params(sample_rate, frame, hop, n_fft, window, bands)
    lens, c_lens = _lengths(lengths, _metric.shape(audio, "band_energies"))
    x = _metric.audio(audio, "band_energies")
    b, t = x.shape
    dev = x.device
    nb = len(table[0])
    need = _metric.lib_value("l3ac_frame_spectrum_scratch_bytes", b, t, n, hop, n_fft)
    f_max = lpc_frames(t, n, hop)
    win, tw, wt = _window(dev, window, n), _twiddles(dev, n_fft), _weights(dev, rate, n_fft, table)
    power = torch.empty((b, f_max, nb), dtype=torch.float64, device=dev)
    mag = torch.empty((b, f_max, nb), dtype=torch.float64, device=dev)
    frames = torch.empty(b, dtype=torch.int32, device=dev)
    ptr = lambda v: v.data_ptr() if f_max else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_band_energies(x.data_ptr(), row_stride(x), b, t, c_lens, n, hop, n_fft,
                                                            None if win is None else win.data_ptr(), tw.data_ptr(), wt.data_ptr(), nb, ptr(power),
                                                            ptr(mag), frames.data_ptr(), scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return {"power": power, "magnitude": mag, "frames": frames}


def _check_metric_params(gamma, normalize, trim) -> tuple:
    try:
        gamma, trim = float(gamma), float(trim)
    except (TypeError, ValueError):
        raise ValueError("band_metrics: gamma and trim must be numbers") from None
    if not math.isfinite(gamma):
        raise ValueError(f"band_metrics: gamma {gamma} must be finite")
    if not 0.0 < trim <= 1.0:
        raise ValueError(f"band_metrics: trim {trim} outside (0, 1]")
    return gamma, int(bool(normalize)), trim


@torch.no_grad()
def band_metrics(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, frame: Optional[int] = None,
                 hop: Optional[int] = None, n_fft: Optional[int] = None, window: str = "hann", lengths=None, bands=None, gamma: float = 0.2,
                 normalize: bool = True, trim: float = 0.95, return_frames: bool = False, extra_scratch=None) -> dict:
    """The critical-band measures of (B, T) fp32 CUDA pairs -> ``{"fw_seg_snr_db", "wss", "lsd_db"}`` (B,) fp64 and ``{"frames",
    "snr_frames"}`` (B,) int32, all on the device.  Per frame, on ``frame_spectrum`` of each side (power ``P``, magnitude ``A``) and the
    filters ``band_weights(sample_rate, n_fft, bands)``:

    the frequency-weighted segmental SNR: ``M[i]`` the band sum of ``A / sum A`` (``normalize``) or of ``A``; ``snr_i = 10 log10(Mr_i^2 /
    max((Mr_i - Me_i)^2, 2^-52))`` weighted by ``Mr_i^gamma``, clamped to [-10, 35]; a frame counts iff ``sum A > 0`` on both sides
    (``"snr_frames"``), and the pair's value is the mean over its counted frames, NaN for none;

    the weighted spectral slope distance (Klatt): with ``e[i] = 10 log10 max(E[i], 1e-10)`` of the band sums of ``P`` and the slopes
    ``s[i] = e[i+1] - e[i]``: ``sum W (s_r - s_e)^2 / sum W``, ``W`` the mean of the two sides' ``20 / (20 + emax - e[i]) * 1 / (1 +
    peak_i - e[i])`` with ``peak_i`` the nearest spectral peak in the direction of the slope; which band is a peak or the maximum is
    decided on ``E``, never on its logarithm.  The pair's value is the mean of the lowest ``floor(trim V + 0.5)`` of its ``V`` frame
    values (``trim = 0.95``), as ``lpc_metrics`` trims;

    the log-spectral distance: ``sqrt(mean_k (10 log10 max(Pr[k], 1e-10) - 10 log10 max(Pe[k], 1e-10))^2)`` in dB; the pair's value is
    the mean over all its frames.

    Section 3.22 states every order of summation.  The numbers are this library's definition: no equality with any published code's
    numbers is claimed.  The default band table stops below 4 kHz (``critical_bands``).  A pair may have at most 16384 frames; there is
    no time alignment of the pair (``align`` makes one first).  ``return_frames`` adds ``"fw_seg_snr_frames"`` (NaN where not counted),
    ``"wss_frames"``, ``"lsd_frames"``: (B, F) fp64; ``"magnitude_sum"``: (B, F, 2) fp64 (reference, estimate); ``"band_power"``,
    ``"band_magnitude"``: (B, F, 2, bands) fp64, the band sums of ``P`` before the floor and of the possibly normalised ``A``;
    ``"peaks"``: (B, F, 2, bands - 1) int32, the band of ``peak_i``; ``"argmax"``: (B, F, 2) int32, the first band of the largest ``E``.
    ``lengths``: the pairs' common lengths.  Other parameters, the bit guarantee and stream capture as ``band_energies``."""
    rate, n, hop, n_fft, table = _check_params(sample_rate, frame, hop, n_fft, window, bands)
    gamma, normalize, trim = _check_metric_params(gamma, normalize, trim)
    shape_r, shape_e = _metric.shape(reference, "band_metrics"), _metric.shape(estimate, "band_metrics")
    if shape_r is not None and shape_e is not None and shape_r != shape_e:
        raise ValueError(f"band_metrics: reference {shape_r} and estimate {shape_e} differ in shape")
    lens, c_lens = _lengths(lengths, shape_r)
    if shape_r is not None and lpc_frames(shape_r[1], n, hop) > MAX_FRAMES:
        raise ValueError(f"band_metrics: {lpc_frames(shape_r[1], n, hop)} frames are more than the {MAX_FRAMES} of a pair")
    r, e = _metric.audio(reference, "band_metrics"), _metric.audio(estimate, "band_metrics")
    if r.device != e.device:
        raise RuntimeError(f"band_metrics: reference is on {r.device} but estimate is on {e.device}")
    b, t = r.shape
    dev = r.device
    nb = len(table[0])
    need = _metric.lib_value("l3ac_band_metrics_scratch_bytes", b, t, n, hop, n_fft, nb)
    f_max = lpc_frames(t, n, hop)
    win, tw, wt = _window(dev, window, n), _twiddles(dev, n_fft), _weights(dev, rate, n_fft, table)
    out = torch.empty((b, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 2), dtype=torch.int32, device=dev)
    vals = total = band_p = band_m = peaks = None
    if return_frames:
        vals = torch.empty((b, f_max, 3), dtype=torch.float64, device=dev)
        total = torch.empty((b, f_max, 2), dtype=torch.float64, device=dev)
        band_p = torch.empty((b, f_max, 2, nb), dtype=torch.float64, device=dev)
        band_m = torch.empty((b, f_max, 2, nb), dtype=torch.float64, device=dev)
        peaks = torch.empty((b, f_max, 2, nb), dtype=torch.int32, device=dev)
    ptr = lambda v: v.data_ptr() if v is not None and f_max else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_band_metrics(
            r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, n, hop, n_fft, None if win is None else win.data_ptr(),
            tw.data_ptr(), wt.data_ptr(), nb, gamma, normalize, trim, out.data_ptr(), counts.data_ptr(), ptr(vals), ptr(total), ptr(band_p),
            ptr(band_m), ptr(peaks), scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    res = dict(_metric.columns(out, ("fw_seg_snr_db", "wss", "lsd_db")), **_metric.columns(counts, ("frames", "snr_frames")))
    if return_frames:
        res.update(_metric.columns(vals, ("fw_seg_snr_frames", "wss_frames", "lsd_frames")), magnitude_sum=total, band_power=band_p,
                   band_magnitude=band_m, peaks=peaks[..., :nb - 1].contiguous(), argmax=peaks[..., nb - 1].contiguous())
    return res
