"""Time alignment on the GPU (csrc/kernels/align.hip): the delay and the polarity of an estimate against its
reference by cross-correlation (``delay``), the shift that puts the pair on common samples (``apply_delay``), and the two composed for
the metric functions, which compare sample j with sample j (``align``)."""
from __future__ import annotations

import operator

import torch

from . import _capi, _metric
from ._rows import row_stride

MAX_LAG = 16384  # the largest supported ``max_lag``


def _max_lag(max_lag) -> int:
    """``max_lag`` as the library takes it, checked before any device work: ValueError."""
    try:
        max_lag = operator.index(max_lag)
    except TypeError:
        raise ValueError(f"delay: max_lag {max_lag!r} must be an integer") from None
    if not 0 <= max_lag <= MAX_LAG:
        raise ValueError(f"delay: max_lag {max_lag} outside 0..{MAX_LAG}")
    return max_lag


@torch.no_grad()
def delay(reference: torch.Tensor, estimate: torch.Tensor, max_lag: int, lengths=None, return_xcorr: bool = False, extra_scratch=None) -> dict:
    """Delay of (B, T) fp32 CUDA pairs -> ``{"lag": (B,) int32, "polarity": (B,) int32, "delay": (B,) fp64, "correlation": (B,) fp64}``,
    all on the device.  ``r(d) = sum_j reference[j] estimate[j + d]`` over the clip's own samples for ``d = -max_lag .. max_lag``
    (``0 <= max_lag <= 16384``), per segment of 4096 samples as an fp32 matrix product, from there in fp64 in a fixed order.  ``lag``
    maximises ``|r|`` (ties: the smaller ``|d|``, then the smaller ``d``): a positive lag means the estimate is late,
    ``estimate[j + lag] ~ reference[j]``.  ``polarity`` is -1 where ``r(lag) < 0`` (an inverted estimate), else +1; ``correlation =
    r(lag) / sqrt(E_reference E_estimate)`` lies in [-1, 1] and is the confidence of the pick; ``delay = lag +`` the vertex of the
    parabola through ``r`` at ``lag - 1, lag, lag + 1`` (no refinement at ``+-max_lag``).  A pair with a silent side gives lag 0,
    polarity 0, delay 0 and correlation NaN.  ``lengths``: the pairs' common lengths, B ints in 1..T; samples at or after a clip's
    length are ignored, whatever they hold.  ``return_xcorr`` adds ``"xcorr"``: (B, 2 max_lag + 1) fp64, ``r(-max_lag) .. r(max_lag)``.
    A clip's bits do not depend on the batch it is in; ``extra_scratch``: bytes to allocate above the minimum scratch (the result does
    not depend on it).  No table is uploaded: the call can be captured without a warm-up.  No CPU path: CPU tensors raise."""
    max_lag = _max_lag(max_lag)
    r, e = _metric.pair(reference, estimate, "delay")
    b, t = r.shape
    _, c_lens = _metric.lengths(lengths, b, t)
    dev = r.device
    need = _metric.lib_value("l3ac_xcorr_scratch_bytes", b, t, max_lag)
    lag =torch.empty(b, dtype=torch.int32, device=dev)
    polarity = torch.empty(b, dtype=torch.int32, device=dev)
    dly = torch.empty(b, dtype=torch.float64, device=dev)
    corr = torch.empty(b, dtype=torch.float64, device=dev)
    xcorr = torch.empty((b, 2 * max_lag + 1), dtype=torch.float64, device=dev) if return_xcorr else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_xcorr(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, max_lag, lag.data_ptr(),
                                                    polarity.data_ptr(), dly.data_ptr(), corr.data_ptr(), xcorr.data_ptr() if return_xcorr else None,
                                                    scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    out = {"lag": lag, "polarity": polarity, "delay": dly, "correlation": corr}
    if return_xcorr:
        out["xcorr"] = xcorr
    return out


@torch.no_grad()
def apply_delay(reference: torch.Tensor, estimate: torch.Tensor, lag: torch.Tensor, lengths=None) -> tuple:
    """Shifts (B, T) fp32 CUDA pairs by per-clip lags -> ``(reference_aligned, estimate_aligned, lengths_aligned)``: two new (B, T) fp32
    tensors and (B,) int32, all on the device.  ``lag``: (B,) int32 on the pair's device (``delay(...)["lag"]``); it is read on the
    device, so the call can be captured together with ``delay``.  With ``m = max(0, n - |lag|)``, ``reference_aligned[j] = reference[j +
    max(0, -lag)]`` and ``estimate_aligned[j] = estimate[j + max(0, lag)]`` for ``j < m`` — the samples both sides have — and exact
    zeros from ``m`` on; ``lengths_aligned = m``.  The polarity is not applied: negate the estimate where ``polarity`` is -1 before a
    metric that sees the sign, such as ``signal_metrics``' ``mse`` and ``snr_db`` (its ``si_sdr_db`` fits a signed scale and does
    not; nor do ``mel_distance``, ``stoi`` and ``pitch_metrics``)."""
    if not isinstance(lag, torch.Tensor) or lag.dtype != torch.int32 or lag.dim() != 1:
        raise ValueError("apply_delay: lag must be a one-dimensional int32 tensor, one lag per clip")
    r, e = _metric.pair(reference, estimate, "apply_delay")
    b, t = r.shape
    _, c_lens = _metric.lengths(lengths, b, t)
    dev = r.device
    if lag.shape[0] != b:
        raise ValueError(f"apply_delay: {lag.shape[0]} lags for a batch of {b}")
    if lag.device != dev:
        raise RuntimeError(f"apply_delay: lag is on {lag.device} but the audio is on {dev}")
    lag = lag.contiguous()
    need = _metric.lib_value("l3ac_xcorr_scratch_bytes", b, t, 0)  # (covers the lengths' upload, all this entry needs)
    out_r = torch.empty((b, t), dtype=torch.float32, device=dev)
    out_e = torch.empty((b, t), dtype=torch.float32, device=dev)
    m = torch.empty(b, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need)
        _capi.check(_capi.load_library().l3ac_align_apply(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, lag.data_ptr(),
                                                          out_r.data_ptr(), t, out_e.data_ptr(), t, m.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                          _metric.stream(dev)))
    return out_r, out_e, m


@torch.no_grad()
def align(reference: torch.Tensor, estimate: torch.Tensor, max_lag: int, lengths=None) -> tuple:
    """``delay`` then ``apply_delay``, bit for bit -> ``(reference_aligned, estimate_aligned, lengths, info)``, ready for the metric
    functions: ``signal_metrics(reference_aligned, estimate_aligned, lengths=lengths)``.  ``lengths`` is a list of Python ints, which
    is what those functions take: this call makes ONE device-to-host read, of the B aligned lengths (it synchronises the stream and
    cannot be captured; ``delay`` and ``apply_delay`` can).  ``info`` is ``delay``'s dict plus ``"lengths"``, the aligned lengths on
    the device as ``apply_delay`` wrote them, and ``"empty"``, the list of the clips whose aligned length is 0 (``|lag|`` reaches the
    clip's length): the metric functions require lengths of at least 1, so such a clip has length 1 in ``lengths`` — one sample, an exact
    zero on both sides — and its metrics mean nothing."""
    info = delay(reference, estimate, max_lag, lengths=lengths)
    ref_aligned, est_aligned, m = apply_delay(reference, estimate, info["lag"], lengths=lengths)
    counts = [int(v) for v in m.tolist()]  # the one device-to-host read
    info = dict(info, lengths=m, empty=[i for i, v in enumerate(counts) if v == 0])
    return ref_aligned, est_aligned, [max(v, 1) for v in counts], info
