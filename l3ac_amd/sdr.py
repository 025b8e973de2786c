"""The SDR of BSS Eval on the GPU (csrc/kernels/sdr.hip): the signal-to-distortion ratio of an estimate after any
linear time-invariant distortion of up to ``filter_length`` taps of the reference has been allowed (``sdr``), and its two primitives on
their own: the lag correlation of whole clips (``correlate``) and the batched Toeplitz solve (``toeplitz_solve``)."""
from __future__ import annotations

import math

import torch

from . import _capi, _metric
from ._rows import row_stride

MAX_TAPS = 1024  # the longest filter, the most lags, the largest Toeplitz system


def _taps(value, name: str, what: str) -> int:
    try:
        taps = int(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be an integer") from None
    if not 1 <= taps <= MAX_TAPS:
        raise ValueError(f"{what}: {name} {taps} outside 1..{MAX_TAPS}")
    return taps


def _pair_shape(a, b, what: str, names: tuple):
    """The common ``(batch, samples)`` of two tensors, checked before their devices are; None where one is not a tensor (``_metric.audio``
    refuses it afterwards)."""
    shape_a, shape_b = _metric.shape(a, what), _metric.shape(b, what)
    if shape_a is None or shape_b is None:
        return None
    if shape_a != shape_b:
        raise ValueError(f"{what}: {names[0]} {shape_a} and {names[1]} {shape_b} differ in shape")
    if a.device != b.device:
        raise RuntimeError(f"{what}: {names[0]} is on {a.device} but {names[1]} is on {b.device}")
    return shape_a


def _clips(a, b, taps: int, lengths, what: str, names: tuple):
    """Two batches of clips and their lengths, everything checked before any device work -> (a, b, the ctypes lengths or None)."""
    shape = _pair_shape(a, b, what, names)
    c_lens = None
    if shape is not None:
        _, c_lens = _metric.lengths(lengths, *shape)
        _metric.lib_value("l3ac_correlate_scratch_bytes" if what == "correlate" else "l3ac_sdr_scratch_bytes", shape[0], shape[1], taps)
    return _metric.audio(a, what), _metric.audio(b, what), c_lens


@torch.no_grad()
def correlate(u: torch.Tensor, v: torch.Tensor, lags: int, lengths=None, extra_scratch=None) -> torch.Tensor:
    """The lag correlation of (B, T) fp32 CUDA clips -> (B, lags) fp64 on the device: ``out[k] = sum_{t=0}^{n-1-k} u[t] v[t+k]`` for
    ``k = 0..lags-1`` over each clip's own ``n`` samples, +0 for ``k >= n``.  The samples are converted to fp64 first, so every product
    is exact; the sum is 64 interleaved partial sums (partial ``l`` takes ``t = l mod 64`` in increasing ``t``) and a fixed fold
    (section 3.21): the bits depend on ``n`` and ``k`` alone.  ``lags`` in 1..1024, ``T + lags - 1 < 2^31``.  ``lengths``: B ints in 1..T;
    samples at or after a clip's length are never read.  ``extra_scratch``: bytes to allocate above the minimum scratch (the result does
    not depend on it).  Capturable as the first call.  No CPU path: CPU tensors raise."""
    lags = _taps(lags, "lags", "correlate")
    x, y, c_lens = _clips(u, v, lags, lengths, "correlate", ("u", "v"))
    b, t = x.shape
    dev = x.device
    need = _metric.lib_value("l3ac_correlate_scratch_bytes", b, t, lags)
    out = torch.empty((b, lags), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_correlate(x.data_ptr(), row_stride(x), y.data_ptr(), row_stride(y), b, t, c_lens, lags, out.data_ptr(),
                                                        scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return out


@torch.no_grad()
def toeplitz_solve(r: torch.Tensor, b: torch.Tensor) -> dict:
    """``G x = b`` with ``G[i][j] = r[|i - j|]`` for (B, L) CUDA tensors (taken as fp64), one system a row, by the Levinson recursion in
    fp64 in the order section 3.21 states -> ``{"x": (B, L), "error": (B,)}`` fp64 (``error`` is the final prediction error ``E_{L-1}``
    of ``r``) and ``{"valid": (B,)}`` int32 on the device.  A system is valid iff ``r[0] > 0`` and every intermediate error is positive
    (``G`` positive definite as far as the recursion can tell); an invalid one has ``x`` and ``error`` NaN and disturbs no other row.
    ``L`` in 1..1024.  Capturable as the first call.  No CPU path: CPU tensors raise."""
    for value, name in ((r, "r"), (b, "b")):
        if isinstance(value, torch.Tensor) and value.dim() != 2:
            raise ValueError(f"toeplitz_solve: {name} must be (batch, length), got {tuple(value.shape)}")
    if isinstance(r, torch.Tensor) and isinstance(b, torch.Tensor):
        if r.shape != b.shape:
            raise ValueError(f"toeplitz_solve: r {tuple(r.shape)} and b {tuple(b.shape)} differ in shape")
        if r.shape[0] == 0:
            raise ValueError("toeplitz_solve: empty batch")
        _taps(r.shape[1], "length", "toeplitz_solve")
        if r.device != b.device:
            raise RuntimeError(f"toeplitz_solve: r is on {r.device} but b is on {b.device}")
        _metric.lib_value("l3ac_toeplitz_solve_scratch_bytes", r.shape[0], r.shape[1])
    for value in (r, b):
        if not isinstance(value, torch.Tensor) or not value.is_cuda:
            raise RuntimeError("toeplitz_solve needs CUDA tensors: l3ac_amd has no CPU path")
    r64, b64 = r.to(torch.float64).contiguous(), b.to(torch.float64).contiguous()
    n, length = r64.shape
    dev = r64.device
    need = _metric.lib_value("l3ac_toeplitz_solve_scratch_bytes", n, length)
    x = torch.empty((n, length), dtype=torch.float64, device=dev)
    error = torch.empty(n, dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need)
        _capi.check(_capi.load_library().l3ac_toeplitz_solve(r64.data_ptr(), b64.data_ptr(), n, length, x.data_ptr(), error.data_ptr(), valid.data_ptr(),
                                                             scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return {"x": x, "error": error, "valid": valid}


def _check_load(load) -> float:
    try:
        load = float(load)
    except (TypeError, ValueError):
        raise ValueError("sdr: load must be a number") from None
    if not (load >= 0.0 and math.isfinite(load)):
        raise ValueError(f"sdr: load {load} must be finite and not negative")
    return load


@torch.no_grad()
def sdr(reference: torch.Tensor, estimate: torch.Tensor, filter_length: int = 512, load: float = 0.0, lengths=None, return_filter: bool = False,
        extra_scratch=None) -> dict:
    """The SDR of BSS Eval (Vincent, Gribonval, Fevotte 2006; one source) of (B, T) fp32 CUDA pairs -> ``{"sdr_db", "target_energy",
    "error_energy", "prediction_error"}`` (B,) fp64 and ``{"valid"}`` (B,) int32, all on the device.  The estimate is projected on the
    ``filter_length`` delayed copies of the reference: ``r = correlate(s, s)``, ``b = correlate(s, est)``, ``r[0] *= 1 + load`` (the
    diagonal loading; skipped for 0), the filter ``c = toeplitz_solve(r, b)``, the target ``y[t] = sum_k c[k] s[t-k]`` over ``t = 0..n+L-2``,
    the error ``e = est - y`` (the estimate zero past ``n``), ``target_energy = sum y^2``, ``error_energy = sum e^2`` in a fixed order and
    ``sdr_db = 10 log10(target_energy / error_energy)`` as IEEE has it: +inf for an estimate that IS a filtered reference, -inf for no
    target at all, NaN for 0 / 0.  ``prediction_error`` is ``E_{L-1}`` of the reference.  A pair is valid iff ``r[0] > 0`` and every
    intermediate error of the recursion is positive; an invalid pair (a silent reference) has NaN everywhere.  With one source BSS
    Eval's SIR is +inf and its SAR equals the SDR.  ``filter_length`` in 1..1024 (1: the plain projection ``<s, est> / <s, s>``; more
    taps than samples are supported), ``T + filter_length - 1 < 2^31``.  There is no time alignment beyond the filter's own taps
    (``align`` removes a longer delay first).  ``return_filter`` adds ``"filter"`` (B, L) fp64, the fitted linear response, and
    ``"autocorr"`` / ``"crosscorr"`` (B, L) fp64 (``r`` after the loading, ``b``).  ``lengths``: the pairs' common lengths, B ints in
    1..T.  A pair's bits do not depend on the batch it is in; ``extra_scratch`` as ``correlate``.  Capturable as the first call.  No CPU
    path: CPU tensors raise."""
    taps = _taps(filter_length, "filter_length", "sdr")
    load = _check_load(load)
    r, e, c_lens = _clips(reference, estimate, taps, lengths, "sdr", ("reference", "estimate"))
    b, t = r.shape
    dev = r.device
    need = _metric.lib_value("l3ac_sdr_scratch_bytes", b, t, taps)
    out = torch.empty((b, 4), dtype=torch.float64, device=dev)
    valid = torch.empty(b, dtype=torch.int32, device=dev)
    filt = torch.empty((b, taps), dtype=torch.float64, device=dev) if return_filter else None
    corr = torch.empty((b, 2, taps), dtype=torch.float64, device=dev) if return_filter else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_sdr(r.data_ptr(), row_stride(r), e.data_ptr(), row_stride(e), b, t, c_lens, taps, load, out.data_ptr(),
                                                  valid.data_ptr(), filt.data_ptr() if return_filter else None,
                                                  corr.data_ptr() if return_filter else None, scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    res = dict(_metric.columns(out, ("sdr_db", "target_energy", "error_energy", "prediction_error")), valid=valid)
    if return_filter:
        res.update(filter=filt, autocorr=corr[:, 0].contiguous(), crosscorr=corr[:, 1].contiguous())
    return res
