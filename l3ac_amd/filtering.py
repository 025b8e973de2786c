"""IIR filtering on the GPU (csrc/kernels/iir.hip): ``scipy.signal.sosfilt`` for batches of clips, parallel over
time (``sosfilt``), the Butterworth designs (``butter_sos``), the loudness meter's K-weighting as a cascade (``k_weighting_sos``), the
two composed (``highpass``), and the streaming session (``StreamFilter``, ``l3ac_amd.stream_filter``)."""
from __future__ import annotations

import ctypes
import math
import operator

import torch

from . import _capi, _metric
from ._rows import row_stride
from .loudness import loudness_coeffs
from .streaming import FILTER_SEGMENT, FilterState, _CarrySession, filter_advance

MAX_SECTIONS = 8


def sosfilt_segment() -> int:
    """The segment of the parallel recursion in samples (``l3ac_sosfilt_segment``): part of the definition of ``sosfilt``'s bits."""
    return int(_capi.load_library().l3ac_sosfilt_segment())


def _sections(sos):
    """``sos`` (N, 6) in scipy's layout, checked -> (N, the (N, 5) rows b0 b1 b2 a1 a2 divided by a0 as the library takes them).  Every
    error is a ValueError, before any device work."""
    try:
        rows = torch.as_tensor(sos).detach().to("cpu", torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("sos must be an (N, 6) array of numbers") from None
    if rows.dim() != 2 or rows.shape[1] != 6:
        raise ValueError(f"sos must be (N, 6) rows b0 b1 b2 a0 a1 a2, got {tuple(rows.shape)}")
    n = rows.shape[0]
    if not 1 <= n <= MAX_SECTIONS:
        raise ValueError(f"sos: {n} sections outside 1..{MAX_SECTIONS}")
    if not bool(torch.isfinite(rows).all()):
        raise ValueError("sos has a non-finite coefficient")
    if bool((rows[:, 3] == 0).any()):
        raise ValueError("sos: a0 = 0")
    rows = rows / rows[:, 3:4]
    for i, (a1, a2) in enumerate(zip(rows[:, 4].tolist(), rows[:, 5].tolist())):
        if not (math.isfinite(a1) and math.isfinite(a2) and abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
            raise ValueError(f"sos: section {i} (a1 = {a1!r}, a2 = {a2!r}) is not stable: it needs |a2| < 1 and |a1| < 1 + a2")
    flat = rows[:, [0, 1, 2, 4, 5]].reshape(-1).tolist()
    if not all(math.isfinite(v) for v in flat):
        raise ValueError("sos has a non-finite coefficient after the division by a0")
    return n, (ctypes.c_double * (5 * n))(*flat)


def _out_dtype(dtype) -> torch.dtype:
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype!r}")
    return dtype


@torch.no_grad()
def sosfilt(audio: torch.Tensor, sos, lengths=None, dtype: torch.dtype = torch.float32, extra_scratch: int = 0) -> torch.Tensor:
    """``scipy.signal.sosfilt(sos, audio)`` of (B, T) fp32 CUDA mono clips, in fp64 -> a new (B, T) ``dtype`` tensor (fp32: the fp64
    result rounded once).  ``sos``: (N, 6) rows ``b0 b1 b2 a0 a1 a2``, 1 <= N <= 8, finite, a0 != 0, every section inside the
    stability triangle (``|a2| < 1`` and ``|a1| < 1 + a2`` after the division by a0); anything else is a ValueError before any device
    work, on CPU tensors as well.  Every clip starts from rest at its sample 0.  ``lengths``: B ints in 1..T; samples at or after a
    clip's length are ignored, whatever they hold, and come out as zero.

    The recursion runs in parallel over time in segments of ``sosfilt_segment()`` = 256 samples (zero-state pass, a scan of the
    2N-value state in double-double arithmetic, output pass): the result is the sequential filter's to within its own rounding error,
    not bit for bit scipy's, and it is defined by DESIGN.md section 3.24 to the bit.  A clip's bits do not depend on the batch it is in
    or on ``extra_scratch``.  Nothing is uploaded: the call can be captured without a warm-up.  No CPU path: CPU tensors raise."""
    dtype = _out_dtype(dtype)
    n_sec, c_sos = _sections(sos)
    shape = _metric.shape(audio, "sosfilt")
    if shape is not None:
        _metric.lengths(lengths, *shape)
    x = _metric.audio(audio, "sosfilt")
    b, t = x.shape
    lens, c_lens = _metric.lengths(lengths, b, t)
    dev = x.device
    need = _metric.lib_value("l3ac_sosfilt_scratch_bytes", b, t, n_sec)
    out = torch.empty((b, t), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_sosfilt(x.data_ptr(), row_stride(x), b, t, c_lens, c_sos, n_sec, out.data_ptr(), row_stride(out),
                                                      int(dtype == torch.float64), scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return out


@torch.no_grad()
def sosfilt_matrix(sos, device) -> tuple:
    """The library's M for ``sos`` -> ``(hi, lo)``, two (2N, 2N) fp64 tensors on ``device``: the matrix that advances the cascade's state
    over one segment of zero input, as the unevaluated sum hi + lo (``l3ac_sosfilt_matrix``)."""
    n_sec, c_sos = _sections(sos)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("sosfilt_matrix needs a CUDA device: l3ac_amd has no CPU path")
    hi = torch.empty((2 * n_sec, 2 * n_sec), dtype=torch.float64, device=dev)
    lo = torch.empty_like(hi)
    with torch.cuda.device(dev):
        _capi.check(_capi.load_library().l3ac_sosfilt_matrix(c_sos, n_sec, hi.data_ptr(), lo.data_ptr(), _metric.stream(hi.device)))
    return hi, lo


def butter_sos(order: int, cutoff_hz: float, sample_rate: float, kind: str = "highpass") -> torch.Tensor:
    """The bilinear Butterworth ``kind`` = "highpass" | "lowpass" of ``order`` 1..16 at ``cutoff_hz`` (0 < cutoff < sample_rate / 2), with
    pre-warping, in closed form -> (ceil(order / 2), 6) fp64 on the CPU, rows ``b0 b1 b2 1 a1 a2``.  With ``K = tan(pi fc / fs)``, pair
    k = 0 .. order // 2 - 1 has ``q = 2 sin(pi (2 k + 1) / (2 order))``, ``a0 = 1 + q K + K^2``, ``a = [1, 2 (K^2 - 1) / a0,
    (1 - q K + K^2) / a0]`` and ``b = [K^2, 2 K^2, K^2] / a0`` (low-pass) or ``[1, -2, 1] / a0`` (high-pass); an odd order puts the
    first-order section first, ``b = [K, K, 0] / (1 + K)`` or ``[1, -1, 0] / (1 + K)``, ``a = [1, (K - 1) / (K + 1), 0]``.  That is the
    definition; its response agrees with ``scipy.signal.butter(order, fc, kind, fs=fs, output="sos")`` to 1e-10 for cutoffs from
    fs / 100 up (the pairing and order of the sections differ).  ValueError for anything else."""
    if kind not in ("highpass", "lowpass"):
        raise ValueError(f"kind must be 'highpass' or 'lowpass', got {kind!r}")
    try:
        if isinstance(order, bool):
            raise TypeError
        order = operator.index(order)
    except TypeError:
        raise ValueError(f"order must be an integer, got {order!r}") from None
    try:
        cutoff_hz, sample_rate = float(cutoff_hz), float(sample_rate)
    except (TypeError, ValueError):
        raise ValueError("cutoff_hz and sample_rate must be numbers") from None
    if not -2 ** 31 <= int(order) < 2 ** 31:
        raise ValueError(f"order {order} outside 1..16")
    host = _metric.host_table("l3ac_butter_sos", torch.float64, int(order), cutoff_hz, sample_rate, int(kind == "highpass"))
    return host.view(-1, 6).clone()


def k_weighting_sos(sample_rate: int) -> torch.Tensor:
    """``loudness``' K-weighting at ``sample_rate`` as a (2, 6) fp64 cascade on the CPU (``loudness_coeffs(sample_rate)[0]``):
    ``sosfilt(x, k_weighting_sos(fs))`` is K-weighted audio.  ValueError for a rate the meter does not support."""
    return loudness_coeffs(sample_rate)[0]


def highpass(audio: torch.Tensor, cutoff_hz: float = 50.0, sample_rate: int = 16000, order: int = 4, lengths=None) -> torch.Tensor:
    """``sosfilt(audio, butter_sos(order, cutoff_hz, sample_rate, "highpass"), lengths=lengths)``, bit for bit: the high-pass against DC
    and rumble that speech codecs put in front of everything else."""
    return sosfilt(audio, butter_sos(order, cutoff_hz, sample_rate, "highpass"), lengths=lengths)


class StreamFilter(_CarrySession):
    """``l3ac_amd.stream_filter(streams, sos)``: S concurrent live streams through the cascade ``sos`` packet by packet, with ``sosfilt``'s
    bits; see ``push``.  Needs no codec and no context.  It drops into the chain of the other sessions::

        y, n = rs.push(packet_48k, lengths=new_samples, end=finished)
        y, n = flt.push(y, lengths=n, end=finished)
        q_feature, indices = enc.push(y, lengths=n, end=finished)
    """

    _what = "stream_filter"
    _fresh = FilterState()
    _elements = "samples"
    _phase = "the position of every stream in its segment"

    def __init__(self, streams: int, sos, dtype: torch.dtype = torch.float32):
        self.dtype = _out_dtype(dtype)
        self.sections, self._sos = _sections(sos)
        super().__init__(streams)
        if self.streams > 65535:
            raise ValueError(f"streams {self.streams} outside 1..65535")
        self.state_doubles = _metric.lib_value("l3ac_sosfilt_stream_state", self.sections)
        if sosfilt_segment() != FILTER_SEGMENT:
            raise _capi.L3acError(f"l3ac_sosfilt_segment() = {sosfilt_segment()} but streaming.FILTER_SEGMENT = {FILTER_SEGMENT}")

    @torch.no_grad()
    def push(self, audio, lengths=None, end=None):
        """New samples of every stream -> ``(y, lengths_out)``: the same samples, filtered.

        ``audio`` (S, n) fp32 CUDA, n >= 0: row i holds stream i's new samples, ``lengths[i]`` in 0..n of them (absent: n; samples at or
        after ``lengths[i]`` are ignored, whatever they hold).  ``y`` is (S, n) in the session's dtype, zero at and after each stream's
        own count; ``lengths_out`` (int32, CPU) echoes the counts: as many outputs as inputs, no latency, nothing to flush.  ``end``: a
        bool or S bools; a stream that ends leaves its slot at rest for the next stream, and that is all it does.  ``reset`` hands a
        slot to a new stream at any time: a stream's first push starts from rest whatever the slot held.

        However a stream's samples are split over pushes and whatever the other streams do, the concatenation of what stream i emits
        is ``sosfilt(x_i[None, :], sos)[0]`` bit for bit.  No host synchronisation; every count is a host integer.  Errors are raised
        before any device work and leave the session unchanged.  A push under stream capture raises RuntimeError: the position in the
        segment advances with every push, so a captured push would replay one position for ever."""
        if not isinstance(audio, torch.Tensor) or audio.dim() != 2 or audio.shape[0] != self.streams:
            raise ValueError(f"audio must be a ({self.streams}, samples) tensor, got {tuple(getattr(audio, 'shape', ()))}")
        new, plan, total, _ = self._take(audio, "audio", torch.float32, lengths, "lengths", end, filter_advance)
        dev, n = new.device, new.shape[1]
        need = _metric.lib_value("l3ac_sosfilt_scratch_bytes", self.streams, max(n, 1), self.sections)
        with torch.cuda.device(dev):
            src, dst = self._buffers(dev, (self.streams, self.state_doubles), torch.float64)
            y = torch.empty((self.streams, n), dtype=self.dtype, device=dev)
            scratch = _metric.scratch(dev, need)
            desc = (_capi.SosStreamDesc * self.streams)(*[_capi.SosStreamDesc(i, p.k, p.take, p.end * _capi.SosStreamDesc.END | p.fresh * _capi.SosStreamDesc.FRESH) for i, (p, _) in enumerate(plan)])
            _capi.check(self._lib.l3ac_sosfilt_stream(
                src, dst, self.streams, self.state_doubles, new.data_ptr() if n else None, n, row_stride(new), self._sos, self.sections, desc,
                self.streams, y.data_ptr() if n else None, row_stride(y), int(self.dtype == torch.float64), scratch.data_ptr(), scratch.numel(),
                _metric.stream(dev)))
            self._commit(plan)
        return y, torch.tensor(total, dtype=torch.int32)
