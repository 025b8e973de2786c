"""Coherence measures on the GPU (csrc/kernels/coherence.hip): the magnitude-squared coherence of a pair of clips on
``frame_spectrum``'s frames, over all frames and per level class of the reference's frames (``coherence``), and the coherence speech
intelligibility index of Kates & Arehart with its three-level form I3 (``csii``), with the host accessor of the critical-band table of ANSI
S3.5-1997 (``sii_bands``)."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _capi, _metric
from ._rows import row_stride
from .bands import _check_params, _lengths, _twiddles, _weights
from .lpc import _window, lpc_frames

MAX_FRAMES = 16384  # the most frames a pair may have
VALUE_KEYS = ("csii", "csii_high", "csii_mid", "csii_low", "i3", "intelligibility")


def sii_bands(sample_rate: Optional[int] = None) -> tuple:
    """The critical-band table of ANSI S3.5-1997 (SII) ``(centre_hz, bandwidth_hz, importance)``, fp64 on the CPU: all 21 bands (150 Hz to
    8500 Hz; a bandwidth is the band's upper edge minus its lower edge; the importances sum to 1), or with ``sample_rate`` the bands
    ``csii`` keeps by default at that rate: those whose upper edge is at or below ``sample_rate / 2`` (20 at 16 kHz, 16 at 8 kHz)."""
    table = _metric.host_table("l3ac_sii_bands", torch.float64).reshape(3, 21)
    keep = 21
    if sample_rate is not None:
        lower = [100.0]
        for w in table[1].tolist():
            lower.append(lower[-1] + w)
        keep = sum(1 for upper in lower[1:] if upper <= int(sample_rate) / 2.0)
    return table[0, :keep].clone(), table[1, :keep].clone(), table[2, :keep].clone()


def _sii_table(bands, rate: int) -> tuple:
    """``bands=`` -> (centres, widths, importances) as tuples of Python floats; ValueError for what is not three equally long sequences of
    numbers with finite positive importances."""
    if bands is None:
        bands = sii_bands(rate)
    try:
        centre, width, imp = bands
        centre, width, imp = (tuple(float(v) for v in (x.tolist() if isinstance(x, torch.Tensor) else x)) for x in (centre, width, imp))
    except (TypeError, ValueError):
        raise ValueError("csii: bands must be a triple (centre_hz, bandwidth_hz, importance) of equally long sequences of numbers") from None
    if not len(centre) == len(width) == len(imp):
        raise ValueError(f"csii: {len(centre)} centres, {len(width)} bandwidths and {len(imp)} importances")
    if not 2 <= len(centre) <= 64:
        raise ValueError(f"csii: {len(centre)} bands outside 2..64")
    if not all(math.isfinite(v) and v > 0.0 for v in imp):
        raise ValueError("csii: every importance must be finite and positive")
    return centre, width, imp


def _importance(dev, imp: tuple) -> torch.Tensor:
    return _metric.table(dev, ("sii_importance",) + imp, lambda: torch.tensor(imp, dtype=torch.float64))


def _pair(reference, estimate, what: str, n: int, hop: int, lengths):
    """The checks of a pair that need no device, then the pair on its device and the lengths."""
    shape_r, shape_e = _metric.shape(reference, what), _metric.shape(estimate, what)
    if shape_r is not None and shape_e is not None and shape_r != shape_e:
        raise ValueError(f"{what}: reference {shape_r} and estimate {shape_e} differ in shape")
    _, c_lens = _lengths(lengths, shape_r)
    if shape_r is not None and lpc_frames(shape_r[1], n, hop) > MAX_FRAMES:
        raise ValueError(f"{what}: {lpc_frames(shape_r[1], n, hop)} frames are more than the {MAX_FRAMES} of a pair")
    r, e = _metric.audio(reference, what), _metric.audio(estimate, what)
    if r.device != e.device:
        raise RuntimeError(f"{what}: reference is on {r.device} but estimate is on {e.device}")
    return r, e, c_lens


def _sums(res: dict, sums: torch.Tensor) -> None:
    res.update(sxx=sums[:, :, 0].contiguous(), syy=sums[:, :, 1].contiguous(),
               sxy=torch.view_as_complex(torch.stack([sums[:, :, 2], sums[:, :, 3]], dim=-1).contiguous()))


@torch.no_grad()
def coherence(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, frame: Optional[int] = None, hop: Optional[int] = None,
              n_fft: Optional[int] = None, window: str = "hann", lengths=None, return_sums: bool = False, extra_scratch=None) -> dict:
    """The magnitude-squared coherence of (B, T) fp32 CUDA pairs on ``frame_spectrum``'s frames -> ``{"msc": (B, n_fft / 2) fp64, "frames":
    (B,) int32, "level_frames": (B, 4) int32}`` on the device.  With ``X``, ``Y`` the spectra of the reference's and the estimate's frame
    and the sums over a set of frames ``Sxx = sum |X|^2``, ``Syy = sum |Y|^2``, ``Sxy = sum X conj(Y)``: ``msc = min(|Sxy|^2 / (Sxx Syy),
    1)``, 0 where ``Sxx Syy == 0``: the part of the estimate's spectrum that is linearly related to the reference.  ``"msc"`` is over all
    frames; NaN for a pair with fewer than 2 frames (one frame is coherent with anything).

    Every frame of the reference has a level class, decided on its energy ``E_t = sum_j (x_j w_j)^2`` against the clip's mean ``M``: 0
    (high) ``E_t >= M``, 1 (mid) ``E_t >= 0.1 M``, 2 (low) ``E_t >= 0.001 M``, 3 (below) otherwise: Kates & Arehart's segments at or above
    the overall RMS level, 0-10 dB below it and 10-30 dB below it.  ``"level_frames"`` counts them; a silent reference has all its frames
    in class 3.  The sums are kept per class; "all frames" is ``((c0 + c1) + (c2 + c3))`` of the class sums.  ``return_sums=True`` adds
    ``"msc_levels"`` (B, 4, n_fft / 2) (NaN for a class with fewer than 2 frames), ``"sxx"``, ``"syy"`` (B, 4, n_fft / 2) fp64 and
    ``"sxy"`` (B, 4, n_fft / 2) complex128 per class, ``"frame_class"`` (B, F) int32 (-1 after a clip's frames) and ``"frame_energy"``
    (B, F) fp64 (NaN there).

    Section 3.23 states every order of summation; an estimate that is the reference, or a power-of-two multiple of it of either sign, has
    ``msc == 1`` exactly wherever ``Sxx > 0``.  Frames, ``n_fft``, ``window``, ``lengths``, ``extra_scratch``, the bit guarantee and stream
    capture as ``band_metrics`` (a pair may have at most 16384 frames; there is no time alignment of the pair: ``align`` makes one first).
    No CPU path: CPU tensors raise."""
    rate, n, hop, n_fft = _check_params(sample_rate, frame, hop, n_fft, window)
    r, e, c_lens = _pair(reference, estimate, "coherence", n, hop, lengths)
    b, t = r.shape
    dev = r.device
    h = n_fft // 2
    need = _metric.lib_value("l3ac_coherence_scratch_bytes", b, t, n, hop, n_fft)
    f_max = lpc_frames(t, n, hop)
    win, tw = _window(dev, window, n), _twiddles(dev, n_fft)
    msc = torch.empty((b, h), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 5), dtype=torch.int32, device=dev)
    levels = sums = cls = energy = None
    if return_sums:
        levels = torch.empty((b, 4, h), dtype=torch.float64, device=dev)
        sums = torch.empty((b, 4, 4, h), dtype=torch.float64, device=dev)
        cls = torch.empty((b, f_max), dtype=torch.int32, device=dev)
        energy = torch.empty((b, f_max), dtype=torch.float64, device=dev)
    ptr = lambda v: v.data_ptr() if v is not None and v.numel() else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_coherence(
            r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, n, hop, n_fft, None if win is None else win.data_ptr(),
            tw.data_ptr(), msc.data_ptr(), ptr(levels), ptr(sums), counts.data_ptr(), ptr(cls), ptr(energy), scratch.data_ptr(), scratch.numel(),
            _metric.stream(dev)))
    res = {"msc": msc, "frames": counts[:, 0].contiguous(), "level_frames": counts[:, 1:].contiguous()}
    if return_sums:
        res.update(msc_levels=levels, frame_class=cls, frame_energy=energy)
        _sums(res, sums)
    return res


@torch.no_grad()
def csii(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, frame: Optional[int] = None, hop: Optional[int] = None,
         n_fft: Optional[int] = None, window: str = "hann", lengths=None, bands=None, return_bands: bool = False, return_sums: bool = False,
         extra_scratch=None) -> dict:
    """The coherence speech intelligibility index (CSII, Kates & Arehart 2005) of (B, T) fp32 CUDA pairs -> ``{"csii", "csii_high",
    "csii_mid", "csii_low", "i3", "intelligibility"}`` (B,) fp64 and ``{"frames": (B,), "level_frames": (B, 4)}`` int32, all on the device.
    On ``coherence``'s sums of a set of frames and the filters ``W = band_weights(sample_rate, n_fft, bands)``: the band's signal ``N_i =
    sum_k W[i][k] msc_k Syy_k`` and distortion ``D_i = sum_k W[i][k] (1 - msc_k) Syy_k``; ``T_i = (clamp(10 log10(N_i / D_i), -15, 15) +
    15) / 30``, 0 where ``N_i == 0`` and 1 where ``D_i == 0 < N_i``; the value is the importance-weighted mean ``sum_i I_i T_i / sum_i
    I_i``.  ``"csii"`` is over all frames, ``"csii_high"``, ``"csii_mid"`` and ``"csii_low"`` over the frames of level classes 0, 1 and 2
    (``coherence``); a set with fewer than 2 frames gives NaN.  ``i3 = -3.47 + 1.84 csii_low + 9.99 csii_mid`` (``csii_high`` has weight 0)
    and ``intelligibility = 1 / (1 + exp(-i3))``, NaN if either term is.  An estimate that is the reference gives exactly 1, a zero
    estimate exactly 0.

    ``bands``: ``(centre_hz, bandwidth_hz, importance)``, 2 to 64 bands with finite positive importances; default ``sii_bands(sample_rate)``,
    the critical bands of ANSI S3.5-1997 that fit below ``sample_rate / 2``.  ``return_bands=True`` adds ``"band_signal"``,
    ``"band_distortion"`` and ``"band_value"`` (``N``, ``D``, ``T``): (B, 4, bands) fp64; rows 0..2 are the level classes high, mid, low and
    row 3 is the "all frames" mapping, each computed whatever its frame count.  ``return_sums=True`` adds ``coherence``'s ``"sxx"``,
    ``"syy"`` and ``"sxy"``.

    The numbers are this library's definition: the band filters are the library's Gaussian filters, not ro-ex filters, and the masking and
    hearing-threshold terms of the full SII are left out; no equality with any published code's numbers is claimed.  Section 3.23 states
    every order of summation.  Other parameters, the bit guarantee and stream capture as ``coherence`` (two more tables: the weights and
    the importances)."""
    rate, n, hop, n_fft = _check_params(sample_rate, frame, hop, n_fft, window)
    centre, width, imp = _sii_table(bands, rate)
    _metric.lib_value("l3ac_band_weights", rate, n_fft, len(centre), (ctypes.c_double * len(centre))(*centre),
                      (ctypes.c_double * len(width))(*width), None, 0)
    r, e, c_lens = _pair(reference, estimate, "csii", n, hop, lengths)
    b, t = r.shape
    dev = r.device
    h, nb = n_fft // 2, len(centre)
    need = _metric.lib_value("l3ac_coherence_scratch_bytes", b, t, n, hop, n_fft)
    win, tw = _window(dev, window, n), _twiddles(dev, n_fft)
    wt, it = _weights(dev, rate, n_fft, (centre, width)), _importance(dev, imp)
    out = torch.empty((b, 6), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 5), dtype=torch.int32, device=dev)
    band = torch.empty((3, b, 4, nb), dtype=torch.float64, device=dev) if return_bands else None
    sums = torch.empty((b, 4, 4, h), dtype=torch.float64, device=dev) if return_sums else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_csii(
            r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, n, hop, n_fft, None if win is None else win.data_ptr(),
            tw.data_ptr(), wt.data_ptr(), it.data_ptr(), nb, out.data_ptr(), counts.data_ptr(), None if band is None else band[0].data_ptr(),
            None if band is None else band[1].data_ptr(), None if band is None else band[2].data_ptr(), None if sums is None else sums.data_ptr(),
            scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    res = dict(_metric.columns(out, VALUE_KEYS), frames=counts[:, 0].contiguous(), level_frames=counts[:, 1:].contiguous())
    if return_bands:
        res.update(band_signal=band[0], band_distortion=band[1], band_value=band[2])
    if return_sums:
        _sums(res, sums)
    return res
