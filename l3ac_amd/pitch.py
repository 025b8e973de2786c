"""Pitch on the GPU (csrc/kernels/pitch.hip): a deterministic YIN tracker of mono clips (``pitch``), the pairwise
F0 metrics of low-bitrate codec and vocoder evaluation on top of it (``pitch_metrics``), and the host accessors of the frame geometry."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _capi, _metric
from ._rows import row_stride


def _args(sample_rate, fmin, fmax, window, hop) -> tuple:
    """The geometry parameters as the library takes them (-1: the default of ``window`` / ``hop``)."""
    try:
        return int(sample_rate), float(fmin), float(fmax), -1 if window is None else int(window), -1 if hop is None else int(hop)
    except (TypeError, ValueError):
        raise ValueError("pitch: sample_rate, window and hop must be integers, fmin and fmax numbers") from None


def _check_params(sample_rate, fmin=60.0, fmax=500.0, threshold=0.1, hop=None, window=None) -> tuple:
    """The supported parameters, checked by the library before any device work: ValueError with its message.  Returns what the
    library's calls take and the resolved ``(tau_min, tau_max, window, hop, span)``."""
    args = _args(sample_rate, fmin, fmax, window, hop)
    for given, name in ((window, "window"), (hop, "hop")):
        if given is not None and int(given) < 1:  # (-1 is the library's own spelling of the default, not the caller's)
            raise ValueError(f"pitch: {name} {given} must be at least 1")
    lags = (ctypes.c_int32 * 5)()
    _metric.lib_value("l3ac_pitch_lags", *args, lags)
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("pitch: threshold must be a number") from None
    if not 0.0 < threshold < 1.0:
        raise ValueError(f"pitch: threshold {threshold} outside (0, 1)")
    return args, threshold, tuple(int(v) for v in lags)


def pitch_lags(sample_rate: int = 16000, fmin: float = 60.0, fmax: float = 500.0, hop: Optional[int] = None, window: Optional[int] = None) -> dict:
    """The tracker's geometry -> ``{"tau_min", "tau_max", "window", "hop", "span"}`` (Python ints): ``tau_min = floor(fs / fmax)``,
    ``tau_max = ceil(fs / fmin)``, ``window`` defaults to ``tau_max`` and ``hop`` to ``fs // 100``, ``span = window + tau_max + 1``.
    Raises ValueError for unsupported parameters (8000 <= fs <= 192000, 0 < fmin < fmax <= fs / 4, tau_max > tau_min, hop and window at
    least 1, span at most 4000)."""
    _, _, lags = _check_params(sample_rate, fmin, fmax, 0.5, hop, window)
    return dict(zip(("tau_min", "tau_max", "window", "hop", "span"), lags))


def pitch_frames(samples: int, sample_rate: int = 16000, fmin: float = 60.0, fmax: float = 500.0, hop: Optional[int] = None,
                 window: Optional[int] = None) -> int:
    """Frames of a clip of ``samples`` samples: 0 below ``span``, else ``1 + (samples - span) // hop``.  Frame t reads samples
    ``[t hop, t hop + span)``; its nominal time is ``(t hop + span / 2) / fs``.  Raises ValueError for samples < 0 or unsupported
    parameters."""
    args, _, _ = _check_params(sample_rate, fmin, fmax, 0.5, hop, window)
    return _metric.lib_value("l3ac_pitch_frames", int(samples), *args)


def _track(x: torch.Tensor, c_lens, args: tuple, threshold: float, lags: tuple, return_cmnd: bool, extra_scratch) -> dict:
    """One l3ac_pitch call on checked arguments."""
    b, t = x.shape
    dev = x.device
    need = _metric.lib_value("l3ac_pitch_scratch_bytes", b, t, *args)
    f_max = _metric.lib_value("l3ac_pitch_frames", t, *args)
    f0 =torch.empty((b, f_max), dtype=torch.float64, device=dev)
    voiced = torch.empty((b, f_max), dtype=torch.int32, device=dev)
    aper = torch.empty((b, f_max), dtype=torch.float64, device=dev)
    frames = torch.empty(b, dtype=torch.int32, device=dev)
    cmnd = torch.empty((b, f_max, lags[1] + 2), dtype=torch.float64, device=dev) if return_cmnd else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_pitch(x.data_ptr(), row_stride(x), b, t, c_lens, *args, threshold, f0.data_ptr(), voiced.data_ptr(),
                                                    aper.data_ptr(), cmnd.data_ptr() if return_cmnd and f_max else None, frames.data_ptr(),
                                                    scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    out = {"f0": f0, "voiced": voiced, "aperiodicity": aper, "frames": frames}
    if return_cmnd:
        out["cmnd"] = cmnd
    return out


@torch.no_grad()
def pitch(audio: torch.Tensor, sample_rate: int = 16000, fmin: float = 60.0, fmax: float = 500.0, threshold: float = 0.1,
          hop: Optional[int] = None, window: Optional[int] = None, lengths=None, return_cmnd: bool = False, extra_scratch=None) -> dict:
    """YIN (de Cheveigne & Kawahara 2002, steps 1-5) of (B, T) fp32 CUDA mono clips -> ``{"f0": (B, F) fp64 in Hz, "voiced": (B, F)
    int32, "aperiodicity": (B, F) fp64, "frames": (B,) int32}``, all on the device, ``F = pitch_frames(T, ...)``.  Frame t reads samples
    ``[t hop, t hop + span)`` of its clip and nothing else (no padding, no centring; ``pitch_lags`` gives the geometry).  The
    difference function is summed in fp32 in the direct form, everything after it is fp64.  ``voiced`` is 1 where a lag in
    ``[tau_min, tau_max]`` has its cumulative-mean-normalised difference below ``threshold`` (the first such lag, followed down to its
    local minimum, is the period); otherwise the period is the first global minimum.  ``f0 = sample_rate / (period + shift)`` with the
    parabolic ``shift``; ``aperiodicity`` is the normalised difference at the period.  There is no smoothing and no octave correction.
    ``lengths``: B ints in 1..T; samples at or after a clip's length are ignored, whatever they hold, and the rows at and after a
    clip's own frames hold NaN / 0 / NaN.  ``return_cmnd`` adds ``"cmnd"``: (B, F, tau_max + 2) fp64, the normalised difference of lags
    0 .. tau_max + 1.  A clip's bits do not depend on the batch it is in; ``extra_scratch``: bytes to allocate above the minimum scratch
    (the result does not depend on it).  No table is uploaded: the call can be captured without a warm-up.  No CPU path: CPU tensors raise."""
    args, threshold, lags = _check_params(sample_rate, fmin, fmax, threshold, hop, window)
    x = _metric.audio(audio, "pitch")
    _, c_lens = _metric.lengths(lengths, *x.shape)
    return _track(x, c_lens, args, threshold, lags, return_cmnd, extra_scratch)


@torch.no_grad()
def pitch_metrics(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, fmin: float = 60.0, fmax: float = 500.0,
                  threshold: float = 0.1, hop: Optional[int] = None, window: Optional[int] = None, lengths=None) -> dict:
    """F0 metrics of (B, T) fp32 CUDA pairs -> ``{"f0_rmse_cents", "gpe", "vde", "ffe"}`` (B,) fp64 and ``{"frames", "voiced_reference",
    "voiced_estimate", "voiced_both"}`` (B,) int32, all on the device: ``pitch`` of each side, then per clip over its own frames the
    voicing decision error ``vde`` (frames voiced on one side only / frames), the gross pitch error ``gpe`` (frames voiced on both
    sides whose f0 differ by more than 20 % / frames voiced on both), the F0 frame error ``ffe`` (either / frames) and the RMS of
    ``1200 log2(f_estimate / f_reference)`` over the frames voiced on both sides, in fp64 in a fixed order.  A ratio whose denominator
    is zero is NaN.  There is no time alignment of the pair (``align`` makes one first).  ``lengths``: the pairs' common lengths.  Parameters as ``pitch``."""
    args, threshold, lags = _check_params(sample_rate, fmin, fmax, threshold, hop, window)
    r, e = _metric.pair(reference, estimate, "pitch_metrics")
    b, t = r.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    lib = _capi.load_library()
    c_frames = None if lens is None else (ctypes.c_int32 * b)(*(lib.l3ac_pitch_frames(n, *args) for n in lens))
    ref = _track(r, c_lens, args, threshold, lags, False, None)
    est = _track(e, c_lens, args, threshold, lags, False, None)
    dev = r.device
    out = torch.empty((b, 4), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 4), dtype=torch.int32, device=dev)
    f_max = ref["f0"].shape[1]
    with torch.cuda.device(dev):
        _capi.check(lib.l3ac_pitch_metrics(ref["f0"].data_ptr() if f_max else None, ref["voiced"].data_ptr() if f_max else None,
                                           est["f0"].data_ptr() if f_max else None, est["voiced"].data_ptr() if f_max else None, b, f_max, c_frames,
                                           out.data_ptr(), counts.data_ptr(), _metric.stream(dev)))
    return dict(_metric.columns(out, ("f0_rmse_cents", "gpe", "vde", "ffe")),
                **_metric.columns(counts, ("frames", "voiced_reference", "voiced_estimate", "voiced_both")))
