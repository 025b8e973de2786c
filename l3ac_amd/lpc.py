"""Linear prediction on the GPU (csrc/kernels/lpc.hip): batched short-time LPC analysis of mono clips (``lpc``),
the spectral-envelope measures of speech-codec evaluation on top of it — log-likelihood ratio, Itakura-Saito distance, LPC cepstral
distance — with the segmental SNR of the same frames (``lpc_metrics``), and the host accessors of the frame geometry and the window."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _capi, _metric
from ._rows import row_stride

MAX_FRAMES = 16384  # the most frames a pair of ``lpc_metrics`` may have
WINDOWS = ("hann", "rect")


def lpc_window(frame: int) -> torch.Tensor:
    """The library's analysis window (frame,) fp32 on the CPU: ``w[i] = 0.5 (1 - cos(2 pi (i + 1) / (frame + 1)))``, the asymmetric Hann
    form of the published measures, designed in fp64 and rounded once.  Raises ValueError for ``frame`` outside 2..8192."""
    return _metric.host_table("l3ac_lpc_window", torch.float32, int(frame))


def lpc_defaults(sample_rate: int) -> tuple:
    """``(order, frame, hop)`` at ``sample_rate``: order 10 below 10 kHz, else 16; a 30 ms frame, ``(30 fs + 500) // 1000`` samples; a hop
    of ``frame // 4``.  Raises ValueError for a rate outside 8000..192000."""
    out = (ctypes.c_int32 * 3)()
    try:
        rate = int(sample_rate)
    except (TypeError, ValueError):
        raise ValueError("lpc: sample_rate must be an integer") from None
    _metric.lib_value("l3ac_lpc_defaults", rate, out)
    return int(out[0]), int(out[1]), int(out[2])


def lpc_frames(samples: int, frame: int, hop: int) -> int:
    """Frames of a clip of ``samples`` samples: 0 below ``frame``, else ``1 + (samples - frame) // hop``.  Frame t reads samples
    ``[t hop, t hop + frame)``.  Raises ValueError for samples < 0, ``frame`` outside 2..8192 or hop < 1."""
    return _metric.lib_value("l3ac_lpc_frames", int(samples), int(frame), int(hop))


def _check_params(sample_rate, order=None, frame=None, hop=None, window="hann") -> tuple:
    """The supported parameters, checked by the library before any device work: ValueError with its message.  Returns the resolved
    ``(sample_rate, order, frame, hop)``."""
    d_order, d_frame, _ = lpc_defaults(sample_rate)
    try:
        order = d_order if order is None else int(order)
        frame = d_frame if frame is None else int(frame)
        hop = frame // 4 if hop is None else int(hop)
    except (TypeError, ValueError):
        raise ValueError("lpc: order, frame and hop must be integers") from None
    _metric.lib_value("l3ac_lpc_scratch_bytes", 1, 1, int(sample_rate), order, frame, hop)
    if window not in WINDOWS:
        raise ValueError(f"lpc: window {window!r} is not one of {WINDOWS}")
    return int(sample_rate), order, frame, hop


def _clip_lengths(lengths, shape):
    """``lengths=`` checked against a shape that is known (``_metric.shape``: before the device is) -> as ``_metric.lengths``."""
    return (None, None) if shape is None else _metric.lengths(lengths, *shape)


def _window(dev, window: str, frame: int):
    """The device copy of the window, uploaded by the first eager call; None for the rectangular window."""
    return None if window == "rect" else _metric.table(dev, ("lpc_window", frame), lambda: lpc_window(frame))


@torch.no_grad()
def lpc(audio: torch.Tensor, sample_rate: int = 16000, order: Optional[int] = None, frame: Optional[int] = None, hop: Optional[int] = None,
        window: str = "hann", lengths=None, extra_scratch=None) -> dict:
    """Short-time linear prediction of (B, T) fp32 CUDA mono clips by the autocorrelation method -> ``{"a": (B, F, p + 1), "reflection":
    (B, F, p), "error": (B, F) (the final prediction error E_p), "autocorr": (B, F, p + 1)}`` fp64 and ``{"valid": (B, F), "frames":
    (B,)}`` int32, all on the device, ``F = lpc_frames(T, frame, hop)``.  Frame t reads samples ``[t hop, t hop + frame)`` of its clip
    and nothing else (no padding, no centring).  The samples times the fp32 window (``"hann"``: ``lpc_window``; ``"rect"``: ones) are
    exact in fp64; the autocorrelation ``r[0..p]`` is summed in fp64 in a fixed order and the Levinson-Durbin recursion runs in fp64
    (section 3.18 states both).  ``A(z) = sum_i a[i] z^-i`` with ``a[0] = 1``: the prediction is ``-sum_{i>=1} a[i] x[n - i]``.  A frame
    is valid iff ``r[0] > 0`` and every intermediate error is positive; an invalid frame has ``a``, ``reflection`` and ``error`` NaN and
    keeps its ``autocorr``.  ``order`` in 1..32, ``order < frame <= 8192``, ``hop >= 1``; the defaults are ``lpc_defaults(sample_rate)``.
    ``lengths``: B ints in 1..T; samples at or after a clip's length are ignored, whatever they hold, and the rows at and after a clip's
    own frames hold NaN / 0.  A clip's bits do not depend on the batch it is in; ``extra_scratch``: bytes to allocate above the minimum
    scratch (the result does not depend on it).  Capturable after one eager call (the window).  No CPU path: CPU tensors raise."""
    rate, p, n, hop = _check_params(sample_rate, order, frame, hop, window)
    lens, c_lens = _clip_lengths(lengths, _metric.shape(audio, "lpc"))
    x = _metric.audio(audio, "lpc")
    b, t = x.shape
    dev = x.device
    need = _metric.lib_value("l3ac_lpc_scratch_bytes", b, t, rate, p, n, hop)
    f_max = lpc_frames(t, n, hop)
    win = _window(dev, window, n)
    a = torch.empty((b, f_max, p + 1), dtype=torch.float64, device=dev)
    refl = torch.empty((b, f_max, p), dtype=torch.float64, device=dev)
    err = torch.empty((b, f_max), dtype=torch.float64, device=dev)
    r = torch.empty((b, f_max, p + 1), dtype=torch.float64, device=dev)
    valid = torch.empty((b, f_max), dtype=torch.int32, device=dev)
    frames = torch.empty(b, dtype=torch.int32, device=dev)
    ptr = (lambda v: v.data_ptr()) if f_max else (lambda v: None)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_lpc(x.data_ptr(), row_stride(x), b, t, c_lens, rate, p, n, hop, None if win is None else win.data_ptr(),
                                                  ptr(a), ptr(refl), ptr(err), ptr(r), ptr(valid), frames.data_ptr(), scratch.data_ptr(),
                                                  scratch.numel(), _metric.stream(dev)))
    return {"a": a, "reflection": refl, "error": err, "autocorr": r, "valid": valid, "frames": frames}


def _check_metric_params(trim, llr_max, is_max, cd_max) -> tuple:
    try:
        trim, llr_max, is_max, cd_max = float(trim), float(llr_max), float(is_max), float(cd_max)
    except (TypeError, ValueError):
        raise ValueError("lpc_metrics: trim, llr_max, is_max and cd_max must be numbers") from None
    if not 0.0 < trim <= 1.0:
        raise ValueError(f"lpc_metrics: trim {trim} outside (0, 1]")
    for v, name in ((llr_max, "llr_max"), (is_max, "is_max"), (cd_max, "cd_max")):
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f"lpc_metrics: {name} {v} must be finite and not negative")
    return trim, llr_max, is_max, cd_max


@torch.no_grad()
def lpc_metrics(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, order: Optional[int] = None,
                frame: Optional[int] = None, hop: Optional[int] = None, window: str = "hann", lengths=None, trim: float = 0.95,
                llr_max: float = 2.0, is_max: float = 100.0, cd_max: float = 10.0, return_frames: bool = False, extra_scratch=None) -> dict:
    """The spectral-envelope measures of (B, T) fp32 CUDA pairs -> ``{"llr", "is_distance", "cepstral_distance_db", "seg_snr_db"}`` (B,)
    fp64 and ``{"frames", "lpc_frames", "snr_frames"}`` (B,) int32, all on the device.  Per frame, with ``lpc`` of each side (``r``, ``a``)
    and ``q(a, r) = a' R a`` on the Toeplitz matrix of ``r``: ``num = q(a_e, r_r)``, ``g_r = q(a_r, r_r)``, ``g_e = q(a_e, r_e)``; the
    log-likelihood ratio ``ln(num / g_r)`` clamped to ``[0, llr_max]``; the Itakura-Saito distance ``(g_r / g_e)(num / g_r) + ln(g_e /
    g_r) - 1`` clamped to ``[0, is_max]``; the distance of the LPC cepstra ``(10 / ln 10) sqrt(2 sum_m (c_r[m] - c_e[m])^2)`` in dB
    clamped to ``[0, cd_max]``; and ``10 log10(sig / noise)`` of the windowed frames clamped to ``[-10, 35]`` (35 for no noise at all).
    A frame enters the first three iff it is valid on both sides (``"lpc_frames"`` counts them) and the SNR iff its reference energy is
    positive (``"snr_frames"``).  Per pair ``seg_snr_db`` is the mean over its counted frames; each of the other three is the mean of
    the lowest ``k = floor(trim V + 0.5)`` of its ``V`` values (``trim = 0.95``: the published "lowest 95 %"), NaN for ``V = 0`` or ``k =
    0``.  There is no time alignment of the pair (``align`` makes one first).  A pair may have at most 16384 frames.
    ``return_frames`` adds ``"llr_frames"``, ``"is_frames"``, ``"cd_frames"``, ``"seg_snr_frames"``: (B, F) fp64, the clamped values,
    NaN where not counted, and ``"forms"``: (B, F, 5) fp64 = ``num, g_r, g_e, sig, noise``.  ``lengths``: the pairs' common lengths.
    Other parameters, the bit guarantee and stream capture as ``lpc``."""
    rate, p, n, hop = _check_params(sample_rate, order, frame, hop, window)
    trim, llr_max, is_max, cd_max = _check_metric_params(trim, llr_max, is_max, cd_max)
    shape_r, shape_e = _metric.shape(reference, "lpc_metrics"), _metric.shape(estimate, "lpc_metrics")
    if shape_r is not None and shape_e is not None and shape_r != shape_e:
        raise ValueError(f"lpc_metrics: reference {shape_r} and estimate {shape_e} differ in shape")
    lens, c_lens = _clip_lengths(lengths, shape_r)
    if shape_r is not None and lpc_frames(shape_r[1], n, hop) > MAX_FRAMES:
        raise ValueError(f"lpc_metrics: {lpc_frames(shape_r[1], n, hop)} frames are more than the {MAX_FRAMES} of a pair")
    r, e = _metric.audio(reference, "lpc_metrics"), _metric.audio(estimate, "lpc_metrics")
    if r.device != e.device:
        raise RuntimeError(f"lpc_metrics: reference is on {r.device} but estimate is on {e.device}")
    b, t = r.shape
    dev = r.device
    need = _metric.lib_value("l3ac_lpc_metrics_scratch_bytes", b, t, rate, p, n, hop)
    f_max = lpc_frames(t, n, hop)
    win = _window(dev, window, n)
    out = torch.empty((b, 4), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 3), dtype=torch.int32, device=dev)
    vals = torch.empty((b, f_max, 4), dtype=torch.float64, device=dev) if return_frames else None
    forms = torch.empty((b, f_max, 5), dtype=torch.float64, device=dev) if return_frames else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_lpc_metrics(
            r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, rate, p, n, hop, None if win is None else win.data_ptr(), trim,
            llr_max, is_max, cd_max, out.data_ptr(), counts.data_ptr(), vals.data_ptr() if return_frames and f_max else None,
            forms.data_ptr() if return_frames and f_max else None, scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    res = dict(_metric.columns(out, ("llr", "is_distance", "cepstral_distance_db", "seg_snr_db")),
               **_metric.columns(counts, ("frames", "lpc_frames", "snr_frames")))
    if return_frames:
        res.update(_metric.columns(vals, ("llr_frames", "is_frames", "cd_frames", "seg_snr_frames")), forms=forms)
    return res
