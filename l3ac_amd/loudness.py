"""Loudness on the GPU (csrc/kernels/loudness.hip): ITU-R BS.1770-4 integrated loudness of mono clips
(``loudness``), the gain to a target (``loudness_gain``), its application (``apply_gain``) and the three composed
(``normalize_loudness``); the host accessors of the K-weighting design; and the EBU R128 measures of section 3.25 on the same base: the true
peak (``true_peak``, csrc/kernels/true_peak.hip), the block loudness series (``short_term_loudness``) and the loudness range
(``loudness_range``)."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _capi, _metric
from ._rows import row_stride


def loudness_coeffs(sample_rate: int):
    """The library's K-weighting at ``sample_rate`` -> ``(sos (2, 6), M (4, 4))`` fp64 on the CPU: the two biquads as rows
    ``b0 b1 b2 a0 a1 a2`` (``scipy.signal.sosfilt``'s layout), and the matrix that advances the cascade's state over one 100 ms step of
    zero input.  Raises ValueError for an unsupported rate (a multiple of 10 in 8000..192000 is supported)."""
    host = _metric.host_table("l3ac_loudness_coeffs", torch.float64, int(sample_rate))
    return host[:12].view(2, 6).clone(), host[12:].view(4, 4).clone()


def loudness_blocks(samples: int, sample_rate: int) -> int:
    """Gating blocks (400 ms, every 100 ms) of a clip of ``samples`` samples: ``max(samples // (sample_rate // 10) - 3, 0)``.  Raises
    ValueError for samples < 1 or an unsupported rate."""
    return _metric.lib_value("l3ac_loudness_blocks", int(samples), int(sample_rate))


def _check_rate(sample_rate: int) -> None:
    _metric.lib_value("l3ac_loudness_blocks", 1, sample_rate)


def _finite(value, what: str) -> float:
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number") from None
    if not math.isfinite(value):
        raise ValueError(f"{what} must be finite, got {value}")
    return value


def _limit(peak_limit_db) -> float:
    """``peak_limit_db=`` as the library takes it: NaN for none."""
    if peak_limit_db is None:
        return math.nan
    value = float(peak_limit_db)
    if math.isnan(value):
        raise ValueError("peak_limit_db must be a number of dB or None")
    return value


@torch.no_grad()
def loudness(audio: torch.Tensor, sample_rate: int = 16000, lengths=None, return_momentary: bool = False) -> dict:
    """ITU-R BS.1770-4 integrated loudness of (B, T) fp32 CUDA mono clips, in fp64 -> ``{"lufs": (B,) fp64, "peak": (B,) fp64,
    "blocks": (B,) int32, "gated": (B,) int32}``, all on the device.  K-weighting by De Man's closed forms evaluated at ``sample_rate``
    (the standard's table at 48 kHz; the choice ``pyloudnorm`` makes elsewhere), blocks of 400 ms every 100 ms, the absolute gate at
    -70 LKFS and the relative gate 10 LU below.  ``sample_rate``: a multiple of 10 in 8000..192000.  ``blocks`` is the clip's number of
    blocks, ``gated`` how many pass both gates; ``lufs`` is -inf exactly when none does (clips below 400 ms and digital silence
    included).  ``peak`` is the sample peak ``max |x|`` over the clip's own samples (not the true peak).  ``lengths``: B ints in 1..T;
    samples at or after a clip's length are ignored, whatever they hold.  ``return_momentary`` adds ``"momentary"``: (B,
    loudness_blocks(T)) fp64, the blocks' own loudness, -inf at and after a clip's own blocks.  A clip's bits do not depend on the batch
    it is in.  No table is uploaded: the call can be captured without a warm-up.  No CPU path: CPU tensors raise."""
    sample_rate = int(sample_rate)
    _check_rate(sample_rate)
    x = _metric.audio(audio, "loudness")
    b, t = x.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = x.device
    need = _metric.lib_value("l3ac_loudness_scratch_bytes", b, t, sample_rate)
    stats = torch.empty((b, 2), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 2), dtype=torch.int32, device=dev)
    momentary = torch.empty((b, loudness_blocks(t, sample_rate)), dtype=torch.float64, device=dev) if return_momentary else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need)
        _capi.check(_capi.load_library().l3ac_loudness(x.data_ptr(), row_stride(x), b, t, c_lens, sample_rate, stats.data_ptr(), counts.data_ptr(),
                                                       momentary.data_ptr() if return_momentary and momentary.numel() else None,
                                                       scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    out = dict(_metric.columns(stats, ("lufs", "peak")), **_metric.columns(counts, ("blocks", "gated")))
    if return_momentary:
        out["momentary"] = momentary
    return out


def _stat(stats: dict, key: str) -> torch.Tensor:
    v = stats.get(key) if isinstance(stats, dict) else None
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise RuntimeError(f"loudness_gain needs a CUDA tensor stats[{key!r}] (what loudness returns): l3ac_amd has no CPU path")
    if v.dim() != 1 or v.shape[0] == 0:
        raise ValueError(f"stats[{key!r}] must be (batch,), got {tuple(v.shape)}")
    return v.to(torch.float64)


@torch.no_grad()
def loudness_gain(stats: dict, target_lufs: float = -23.0, peak_limit_db: Optional[float] = None) -> dict:
    """What ``loudness`` returned -> ``{"gain_db": (B,) fp64, "gain": (B,) fp64}`` on the device, without a host synchronisation:
    ``gain_db = target_lufs - lufs``; with ``peak_limit_db`` and a non-zero peak at most ``peak_limit_db - 20 log10(peak)``, so that the
    scaled clip's sample peak stays at or below the limit; exactly 0 dB for a clip whose loudness is -inf.  ``gain = 10^(gain_db / 20)``."""
    target = _finite(target_lufs, "target_lufs")
    limit = _limit(peak_limit_db)
    lufs, peak = _stat(stats, "lufs"), _stat(stats, "peak")
    if lufs.shape != peak.shape or lufs.device != peak.device:
        raise ValueError("stats['lufs'] and stats['peak'] differ in shape or device")
    b = lufs.shape[0]
    dev = lufs.device
    packed = torch.stack((lufs, peak), dim=1).contiguous()
    gain = torch.empty((b, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.load_library().l3ac_loudness_gain(packed.data_ptr(), b, target, limit, gain.data_ptr(), _metric.stream(dev)))
    return _metric.columns(gain, ("gain_db", "gain"))


@torch.no_grad()
def apply_gain(audio: torch.Tensor, gain: torch.Tensor, lengths=None) -> torch.Tensor:
    """(B, T) fp32 CUDA audio times a per-clip linear ``gain`` (B,) fp64 CUDA (``loudness_gain(...)["gain"]``, or its reciprocal to
    undo it after decoding) -> a new (B, T) fp32: ``float(double(x) * gain)``, one rounding.  ``lengths``: samples at or after a clip's
    length come out as zero."""
    x = _metric.audio(audio, "apply_gain")
    b, t = x.shape
    if not isinstance(gain, torch.Tensor) or not gain.is_cuda:
        raise RuntimeError("apply_gain needs a CUDA tensor gain: l3ac_amd has no CPU path")
    if gain.shape != (b,):
        raise ValueError(f"gain must be ({b},), got {tuple(gain.shape)}")
    if gain.device != x.device:
        raise RuntimeError(f"apply_gain: audio is on {x.device} but gain is on {gain.device}")
    lens, c_lens = _metric.lengths(lengths, b, t)
    g = gain.to(torch.float64)
    out = torch.empty((b, t), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _capi.check(_capi.load_library().l3ac_apply_gain(x.data_ptr(), row_stride(x), out.data_ptr(), row_stride(out), b, t, c_lens, g.data_ptr(),
                                                         g.stride(0) if b > 1 else 1, _metric.stream(x.device)))
    return out


def true_peak_factor(sample_rate: int) -> int:
    """The oversampling factor of ``true_peak``: 4 for 8000 <= sample_rate < 96000, 2 up to 192000.  Raises ValueError outside that range."""
    return _metric.lib_value("l3ac_true_peak_factor", int(sample_rate))


@torch.no_grad()
def true_peak(audio: torch.Tensor, sample_rate: int = 16000, lengths=None) -> dict:
    """The true peak of (B, T) fp32 CUDA mono clips after BS.1770-4 annex 2 -> ``{"true_peak": (B,) fp64, "true_peak_db": (B,) fp64,
    "peak": (B,) fp64}`` on the device: ``true_peak = max(peak, max |resample(clip alone, sample_rate, L * sample_rate)|)`` bit for bit,
    ``L = true_peak_factor(sample_rate)``, with zeros at and after the clip's length; ``peak`` is the sample peak ``max |x|``;
    ``true_peak_db = 20 log10(true_peak)`` in dBTP, -inf for a silent clip.  The oversampled signal is never written.  ``lengths``: B ints
    in 1..T; samples at or after a clip's length are ignored, whatever they hold.  A clip's bits do not depend on the batch it is in.  No
    table is uploaded: the call can be captured as the first of a process.  No CPU path: CPU tensors raise."""
    sample_rate = int(sample_rate)
    true_peak_factor(sample_rate)
    x = _metric.audio(audio, "true_peak")
    b, t = x.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = x.device
    need = _metric.lib_value("l3ac_true_peak_scratch_bytes", b, t, sample_rate)
    stats = torch.empty((b, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need)
        _capi.check(_capi.load_library().l3ac_true_peak(x.data_ptr(), row_stride(x), b, t, c_lens, sample_rate, stats.data_ptr(), scratch.data_ptr(),
                                                        scratch.numel(), _metric.stream(dev)))
    out = _metric.columns(stats, ("true_peak", "peak"))
    return {"true_peak": out["true_peak"], "true_peak_db": 20.0 * torch.log10(out["true_peak"]), "peak": out["peak"]}


def _window_steps(window) -> int:
    """``window=`` in seconds -> whole steps of 100 ms, 1..600."""
    try:
        steps = round(float(window) * 10.0)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("window must be a number of seconds") from None
    if not 1 <= steps <= 600 or abs(float(window) * 10.0 - steps) > 1e-9:
        raise ValueError(f"window must be a multiple of 0.1 s in 0.1..60, got {window}")
    return steps


@torch.no_grad()
def short_term_loudness(audio: torch.Tensor, sample_rate: int = 16000, lengths=None, window: float = 3.0, return_parts: bool = False) -> dict:
    """The loudness of the blocks of ``window`` seconds, one every 100 ms, of (B, T) fp32 CUDA mono clips (EBU Tech 3341: 3 s is the
    short-term loudness, 0.4 the momentary one, which is ``loudness(return_momentary=True)["momentary"]`` bit for bit) -> ``{"lufs": (B,
    K(T)) fp64, "blocks": (B,) int32}`` on the device; a clip of n samples has ``K(n) = max(n // (sample_rate // 10) - W + 1, 0)`` blocks,
    ``W = 10 window``, and ``lufs`` is -inf at and after them.  ``window``: a multiple of 0.1 s in 0.1..60.  ``return_parts`` adds
    ``"mean_square"`` (B, K(T)), the blocks' K-weighted mean squares summed left to right over the steps (0 after a clip's blocks), and
    ``"energies"`` (B, T // (sample_rate // 10)), the 100 ms step energies (0 after a clip's steps).  ``sample_rate``, ``lengths``, the bit
    guarantee and capture: as ``loudness``."""
    sample_rate = int(sample_rate)
    _check_rate(sample_rate)
    steps = _window_steps(window)
    x = _metric.audio(audio, "short_term_loudness")
    b, t = x.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = x.device
    step = sample_rate // 10
    s_max = t // step
    k_max = max(s_max - steps + 1, 0)
    need = _metric.lib_value("l3ac_r128_scratch_bytes", b, t, sample_rate)
    lufs = torch.empty((b, k_max), dtype=torch.float64, device=dev)
    blocks = torch.empty((b,), dtype=torch.int32, device=dev)
    mean_square = torch.empty((b, k_max), dtype=torch.float64, device=dev) if return_parts else None
    energies = torch.empty((b, s_max), dtype=torch.float64, device=dev) if return_parts else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need)
        _capi.check(_capi.load_library().l3ac_r128_series(x.data_ptr(), row_stride(x), b, t, c_lens, sample_rate, steps, lufs.data_ptr() if k_max else None,
                                                          mean_square.data_ptr() if return_parts and k_max else None,
                                                          energies.data_ptr() if return_parts and s_max else None, blocks.data_ptr(),
                                                          scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    out = {"lufs": lufs, "blocks": blocks}
    if return_parts:
        out["mean_square"], out["energies"] = mean_square, energies
    return out


@torch.no_grad()
def loudness_range(audio: torch.Tensor, sample_rate: int = 16000, lengths=None) -> dict:
    """EBU Tech 3342 loudness range of (B, T) fp32 CUDA mono clips, in fp64 -> ``{"lra", "low_lufs", "high_lufs", "short_term_max",
    "momentary_max": (B,) fp64, "blocks", "above_absolute", "gated": (B,) int32}`` on the device.  Short-term blocks of 3 s every 100 ms
    (``short_term_loudness``); those above -70 LUFS set the relative gate 20 LU below their mean level; of the ``gated`` blocks above both,
    sorted by level, ``low_lufs`` is the 10th and ``high_lufs`` the 95th percentile (the blocks at ``((gated - 1) * 10 + 50) // 100`` and
    ``((gated - 1) * 95 + 50) // 100``) and ``lra = high_lufs - low_lufs`` in LU; no gated block: ``lra`` is exactly 0 and both bounds
    -inf.  ``short_term_max`` and ``momentary_max`` are the largest 3 s and 400 ms block loudness (EBU Tech 3341), -inf for a clip
    without such a block.  A clip may have at most 16384 blocks (27 min).  ``sample_rate``, ``lengths``, the bit guarantee and capture:
    as ``loudness``."""
    sample_rate = int(sample_rate)
    _check_rate(sample_rate)
    x = _metric.audio(audio, "loudness_range")
    b, t = x.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = x.device
    need = _metric.lib_value("l3ac_r128_scratch_bytes", b, t, sample_rate)
    stats = torch.empty((b, 5), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 3), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need)
        _capi.check(_capi.load_library().l3ac_r128_range(x.data_ptr(), row_stride(x), b, t, c_lens, sample_rate, stats.data_ptr(), counts.data_ptr(),
                                                         scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return dict(_metric.columns(stats, ("lra", "low_lufs", "high_lufs", "short_term_max", "momentary_max")),
                **_metric.columns(counts, ("blocks", "above_absolute", "gated")))


def _peak_mode(peak) -> bool:
    if peak not in ("sample", "true"):
        raise ValueError(f"peak must be 'sample' or 'true', got {peak!r}")
    return peak == "true"


@torch.no_grad()
def normalize_loudness(audio: torch.Tensor, target_lufs: float = -23.0, sample_rate: int = 16000, lengths=None,
                       peak_limit_db: Optional[float] = -1.0, peak: str = "sample"):
    """(B, T) fp32 CUDA audio brought to ``target_lufs`` -> ``(audio_out, {"lufs", "peak", "gain_db", "gain"})``: ``loudness``,
    ``loudness_gain`` and ``apply_gain`` composed, bit for bit.  ``lufs`` and ``peak`` are the INPUT's.  The gain never reaches the host;
    hand ``1 / info["gain"]`` to ``apply_gain`` after decoding to restore the level.  ``peak_limit_db=None``: no peak limit.
    ``peak="true"``: the limit is in dBTP; it applies to ``true_peak(audio)["true_peak"]``, which takes the place of the sample peak in
    ``loudness_gain``'s input, and ``info`` gains ``"true_peak"`` (``"peak"`` stays the sample peak)."""
    sample_rate = int(sample_rate)
    _check_rate(sample_rate)
    _finite(target_lufs, "target_lufs")
    _limit(peak_limit_db)
    if _peak_mode(peak):
        true_peak_factor(sample_rate)
    stats = loudness(audio, sample_rate=sample_rate, lengths=lengths)
    info = {"lufs": stats["lufs"], "peak": stats["peak"]}
    limited = stats["peak"]
    if peak == "true":
        limited = info["true_peak"] = true_peak(audio, sample_rate=sample_rate, lengths=lengths)["true_peak"]
    gain = loudness_gain({"lufs": stats["lufs"], "peak": limited}, target_lufs=target_lufs, peak_limit_db=peak_limit_db)
    out = apply_gain(audio, gain["gain"], lengths=lengths)
    info.update({"gain_db": gain["gain_db"], "gain": gain["gain"]})
    return out, info
