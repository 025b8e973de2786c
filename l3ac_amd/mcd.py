"""Mel-cepstral distortion along a dynamic-time-warping path on the GPU (csrc/kernels/mcd.hip): the cepstra of
``log_mel``'s cells (``mfcc``), a batched DTW over rows of fp32 features (``dtw``), and the two composed into the number that
low-bitrate codec and vocoder evaluation reports for outputs that drift against, or differ in length from, their reference (``mcd``)."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _capi, _metric
from ._rows import int_list, row_stride
from .metrics import mel_weights, stft_basis, stft_frames

MAX_FRAMES = 4096  # the most frames a side of a DTW pair may have
MAX_DIM = 64       # the widest feature row of ``dtw``; also the most cepstral coefficients (``n_coeffs``)
MCD_SCALE = 5.0 * math.sqrt(2.0)  # 10 sqrt(2) / ln 10 on cepstra of the natural-log mel amplitude = 5 sqrt(2) on log10 mel power cells


def dct_table(n_mels: int, n_coeffs: int) -> torch.Tensor:
    """The library's orthonormal DCT-II table (n_coeffs + 1, n_mels) fp32 on the CPU: row 0 = sqrt(1 / M), row q = sqrt(2 / M) cos(pi q
    (m + 1/2) / M), designed in fp64 and rounded once.  Raises ValueError for ``n_coeffs`` outside 1..min(n_mels - 1, 64)."""
    return _metric.host_table("l3ac_dct_table", torch.float32, int(n_mels), int(n_coeffs)).view(int(n_coeffs) + 1, int(n_mels))


def _mfcc_hop(n_fft: int, hop) -> int:
    """``hop=None``: 160 (10 ms at 16 kHz) beside the default ``n_fft`` of 512, else ``n_fft // 4`` as in ``log_mel``."""
    if hop is not None:
        return int(hop)
    return 160 if int(n_fft) == 512 else int(n_fft) // 4


def _check_mfcc_params(sample_rate: int, n_fft: int, hop: int, n_mels: int, n_coeffs: int) -> None:
    """The supported parameters, checked by the library before any device work: ValueError with its message."""
    _metric.check_mel_params(sample_rate, n_fft, hop, n_mels)
    _metric.lib_value("l3ac_dct_table", n_mels, n_coeffs, None, 0)


def _mfcc(x: torch.Tensor, sample_rate: int, n_fft: int, hop: int, n_mels: int, n_coeffs: int, c_lens, extra_scratch) -> torch.Tensor:
    b, t = x.shape
    dev = x.device
    basis = _metric.table(dev, ("basis", n_fft), lambda: stft_basis(n_fft))
    weights = _metric.table(dev, ("mel", sample_rate, n_fft, n_mels), lambda: mel_weights(sample_rate, n_fft, n_mels))
    dct = _metric.table(dev, ("dct", n_mels, n_coeffs), lambda: dct_table(n_mels, n_coeffs))
    out = torch.empty((b, stft_frames(t, hop), n_coeffs + 1), dtype=torch.float32, device=dev)
    need = _metric.lib_value("l3ac_mfcc_scratch_bytes", b, t, n_fft, hop, n_mels, n_coeffs)
    with torch.cuda.device(dev):
        # the minimum — the lengths, the cells, log_mel's own scratch — and log_mel's extra room for larger products
        scratch = _metric.mel_scratch(dev, need, b, t, n_fft, hop, extra_scratch)
        _capi.check(_capi.load_library().l3ac_mfcc(x.data_ptr(), b, t, row_stride(x), c_lens, n_fft, hop, basis.data_ptr(), weights.data_ptr(), n_mels,
                                                   dct.data_ptr(), n_coeffs, out.data_ptr(), scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    return out


@torch.no_grad()
def mfcc(audio: torch.Tensor, sample_rate: int = 16000, n_fft: int = 512, hop: Optional[int] = None, n_mels: int = 40, n_coeffs: int = 13,
         lengths=None, extra_scratch=None):
    """(B, T) fp32 CUDA audio -> (B, 1 + T // hop, n_coeffs + 1) fp32 mel cepstra: the orthonormal DCT-II (``dct_table``) of ``log_mel``'s
    cells — log10 of the mel POWER, clamped at 1e-10 — for the same ``sample_rate, n_fft, hop, n_mels``, each coefficient one fp32 fmaf
    chain over the filters in increasing order.  Column 0 is the level ``c0``.  ``n_coeffs`` in 1..min(n_mels - 1, 64).  ``hop`` defaults
    to 160 beside ``n_fft = 512`` (10 ms at 16 kHz), else to ``n_fft // 4``.  With ``lengths`` returns ``(mfcc, frames)`` as ``log_mel``
    does; the rows after a clip's own frames are zero.  Other arguments, the bit guarantee and stream capture as ``log_mel`` (the three
    tables are uploaded by the first eager call)."""
    sample_rate, n_fft, hop, n_mels, n_coeffs = int(sample_rate), int(n_fft), _mfcc_hop(n_fft, hop), int(n_mels), int(n_coeffs)
    _check_mfcc_params(sample_rate, n_fft, hop, n_mels, n_coeffs)
    x = _metric.audio(audio, "mfcc")
    lens, c_lens = _metric.lengths(lengths, x.shape[0], x.shape[1])
    out = _mfcc(x, sample_rate, n_fft, hop, n_mels, n_coeffs, c_lens, extra_scratch)
    if lens is None:
        return out
    return out, torch.tensor([1 + n // hop for n in lens], dtype=torch.int32)


def _features(x, name: str):
    """The shape of one side of ``dtw``, checked before any device work -> (batch, frames, dim)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"dtw: {name} must be a (batch, frames, dim) tensor")
    b, f, dim = x.shape
    if b < 1:
        raise ValueError(f"dtw: {name} has no pairs")
    if not 1 <= f <= MAX_FRAMES:
        raise ValueError(f"dtw: {name} has {f} frames, outside 1..{MAX_FRAMES}")
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"dtw: {name} has dim {dim}, outside 1..{MAX_DIM}")
    return b, f, dim


def _rows_view(x: torch.Tensor) -> torch.Tensor:
    """fp32 with unit stride inside a frame and strides the library can walk (a frame stride of at least dim, rows that do not overlap);
    a view such as ``c[..., 1:]`` stays a view."""
    x = x.to(torch.float32)
    b, f, dim = x.shape
    ok = x.stride(2) == 1 and (f == 1 or x.stride(1) >= dim) and (b == 1 or x.stride(0) >= (f - 1) * (x.stride(1) if f > 1 else 0) + dim)
    return x if ok else x.contiguous()


def _frame_counts(lengths, b: int, frames: int, what: str):
    if lengths is None:
        return [frames] * b, None
    lens = int_list(lengths, b, 1, frames, what, f"a batch of {b}")
    return lens, (ctypes.c_int32 * b)(*lens)


@torch.no_grad()
def dtw(a: torch.Tensor, b: torch.Tensor, lengths_a=None, lengths_b=None, return_path: bool = False, return_cost_matrix: bool = False,
        diagonal_only: bool = False, extra_scratch=None) -> dict:
    """Dynamic time warping of B pairs of feature sequences, ``a`` (B, Fa, dim) against ``b`` (B, Fb, dim), fp32 CUDA with any frame or
    row stride (``Fa, Fb`` in 1..4096, ``dim`` in 1..64) -> ``{"cost": (B,) fp64, "path_length": (B,) int32}``, on the device.  The frame
    distance is the Euclidean ``delta(i, j) = sqrt(sum_q (a[i][q] - b[j][q])^2)`` in fp64; ``Dacc[i][j] = delta(i, j) + min(Dacc[i-1][j-1],
    Dacc[i-1][j], Dacc[i][j-1])`` with ties to the diagonal, then to ``(i-1, j)``, then to ``(i, j-1)``; ``cost = Dacc[Fa-1][Fb-1]``,
    the sequential sum of ``delta`` along the path, whose ``path_length`` lies in ``max(Fa, Fb) .. Fa + Fb - 1``.  ``lengths_a``,
    ``lengths_b``: the pairs' own frame counts, B ints in 1..Fa / 1..Fb; frames at or after a count are never read.
    ``return_path`` adds ``"path"``: (B, Fa + Fb - 1, 2) int32, the ``(i, j)`` of the path from ``(0, 0)`` forward, -1 after its length.
    ``return_cost_matrix`` adds ``"cost_matrix"``: (B, Fa, Fb) fp64, ``delta`` on the cells the call evaluated and 0 elsewhere (a test
    hook: 8 Fa Fb bytes per pair).  ``diagonal_only``: no warping — every pair needs equal counts (ValueError) — ``cost = sum_f delta(f,
    f)`` in the order of ``f``, ``path_length = F``.  A pair's bits do not depend on the batch it is in, on the strides or on
    ``extra_scratch`` (bytes to allocate above the minimum scratch).  No table is uploaded: the call can be captured without a warm-up.
    No CPU path: CPU tensors raise."""
    n, fa, dim = _features(a, "a")
    n_b, fb, dim_b = _features(b, "b")
    if n != n_b or dim != dim_b:
        raise ValueError(f"dtw: a {tuple(a.shape)} and b {tuple(b.shape)} differ in batch or dim")
    lens_a, c_a = _frame_counts(lengths_a, n, fa, "lengths_a")
    lens_b, c_b = _frame_counts(lengths_b, n, fb, "lengths_b")
    if diagonal_only and lens_a != lens_b:
        raise ValueError(f"dtw: diagonal_only needs equal frame counts in every pair, got {lens_a} and {lens_b}")
    if not a.is_cuda or not b.is_cuda:
        raise RuntimeError("dtw needs CUDA tensors: l3ac_amd has no CPU path")
    if a.device != b.device:
        raise RuntimeError(f"dtw: a is on {a.device} but b is on {b.device}")
    a, b = _rows_view(a), _rows_view(b)
    dev = a.device
    need = _metric.lib_value("l3ac_dtw_scratch_bytes", n, fa, fb)
    cost =torch.empty(n, dtype=torch.float64, device=dev)
    steps = torch.empty(n, dtype=torch.int32, device=dev)
    path = torch.empty((n, fa + fb - 1, 2), dtype=torch.int32, device=dev) if return_path else None
    delta = torch.zeros((n, fa, fb), dtype=torch.float64, device=dev) if return_cost_matrix else None
    with torch.cuda.device(dev):
        scratch = _metric.scratch(dev, need, extra_scratch)
        _capi.check(_capi.load_library().l3ac_dtw(a.data_ptr(), a.stride(1), a.stride(0), b.data_ptr(), b.stride(1), b.stride(0), n, dim, fa, fb, c_a,
                                                  c_b, 1 if diagonal_only else 0, cost.data_ptr(), steps.data_ptr(),
                                                  path.data_ptr() if return_path else None, delta.data_ptr() if return_cost_matrix else None,
                                                  scratch.data_ptr(), scratch.numel(), _metric.stream(dev)))
    out = {"cost": cost, "path_length": steps}
    if return_path:
        out["path"] = path
    if return_cost_matrix:
        out["cost_matrix"] = delta
    return out


_dtw = dtw  # (``mcd`` has a parameter of that name)


def _sides(reference, estimate):
    """(batch, Tr, Te) of two tensors, checked before their devices are; None when a side is not a tensor."""
    shape_r, shape_e = _metric.shape(reference, "mcd: reference", empty_ok=True), _metric.shape(estimate, "mcd: estimate", empty_ok=True)
    if shape_r is None or shape_e is None:
        return None
    if shape_r[0] != shape_e[0]:
        raise ValueError(f"mcd: reference {shape_r} and estimate {shape_e} differ in batch")
    return shape_r[0], shape_r[1], shape_e[1]


@torch.no_grad()
def mcd(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, n_fft: int = 512, hop: Optional[int] = None, n_mels: int = 40,
        n_coeffs: int = 13, lengths=None, estimate_lengths=None, dtw: bool = True, return_path: bool = False, extra_scratch=None) -> dict:
    """Mel-cepstral distortion of B pairs, ``reference`` (B, Tr) against ``estimate`` (B, Te) fp32 CUDA (``Tr != Te`` is allowed), along
    the DTW path of their cepstra -> ``{"mcd_db": (B,) fp64, "cost": (B,) fp64, "path_length": (B,) int32}`` on the device and
    ``"frames_ref"``, ``"frames_est"`` (int32, on the CPU).  It is ``mfcc`` of each side, ``dtw`` of the ``[..., 1:]`` views (``c0``, the
    level, is dropped), and ``mcd_db = 5 sqrt(2) cost / path_length`` in fp64 on the device, bit for bit.
    The convention, for comparing with other tools: orthonormal DCT-II, cells that are log10 of the mel POWER (5 sqrt(2) is Kubichek's
    10 sqrt(2) / ln 10 on cepstra of the natural-log mel amplitude, (ln 10 / 2) times these cells), HTK mel triangles without
    normalisation, no silence trimming, the DTW's own frame distance as the distortion of a step, the mean over the path's steps.
    ``lengths``: the references' sample counts, B ints in 1..Tr; ``estimate_lengths``: the estimates', 1..Te (absent: ``lengths`` when
    ``Te == Tr``, else Te).  Each side may have at most 4096 frames (``1 + samples // hop``).  ``dtw=False``: frame f against frame f,
    ``cost = sum_f delta(f, f)`` and ``path_length = F``; every pair must then have equal frame counts (ValueError).  ``return_path`` adds
    ``"path"`` as in ``dtw``.  Capturable after one eager call (the tables).  No CPU path: CPU tensors raise."""
    sample_rate, n_fft, hop, n_mels, n_coeffs = int(sample_rate), int(n_fft), _mfcc_hop(n_fft, hop), int(n_mels), int(n_coeffs)
    _check_mfcc_params(sample_rate, n_fft, hop, n_mels, n_coeffs)
    shape = _sides(reference, estimate)
    if shape is not None:
        n, t_r, t_e = shape
        if n == 0 or t_r == 0 or t_e == 0:
            raise ValueError("empty audio")
        if estimate_lengths is None and t_e == t_r:
            estimate_lengths = lengths
        lens_r = [t_r] * n if lengths is None else int_list(lengths, n, 1, t_r, "lengths", f"a batch of {n}")
        lens_e = [t_e] * n if estimate_lengths is None else int_list(estimate_lengths, n, 1, t_e, "estimate_lengths", f"a batch of {n}")
        for t, name in ((t_r, "reference"), (t_e, "estimate")):
            if 1 + t // hop > MAX_FRAMES:
                raise ValueError(f"mcd: {name} has {1 + t // hop} frames of hop {hop}, above the {MAX_FRAMES} of a DTW pair")
        frames_r, frames_e = [1 + v // hop for v in lens_r], [1 + v // hop for v in lens_e]
        if not dtw and frames_r != frames_e:
            raise ValueError(f"mcd: dtw=False needs equal frame counts in every pair, got {frames_r} and {frames_e}")
    r, e = _metric.audio(reference, "mcd"), _metric.audio(estimate, "mcd")
    if r.device != e.device:
        raise RuntimeError(f"mcd: reference is on {r.device} but estimate is on {e.device}")
    c_r = _mfcc(r, sample_rate, n_fft, hop, n_mels, n_coeffs, None if lengths is None else (ctypes.c_int32 * n)(*lens_r), extra_scratch)
    c_e = _mfcc(e, sample_rate, n_fft, hop, n_mels, n_coeffs, None if estimate_lengths is None else (ctypes.c_int32 * n)(*lens_e), extra_scratch)
    res = _dtw(c_r[..., 1:], c_e[..., 1:], lengths_a=frames_r, lengths_b=frames_e, return_path=return_path, diagonal_only=not dtw)
    out = {"mcd_db": (res["cost"] * MCD_SCALE) / res["path_length"].to(torch.float64), "cost": res["cost"], "path_length": res["path_length"],
           "frames_ref": torch.tensor(frames_r, dtype=torch.int32), "frames_est": torch.tensor(frames_e, dtype=torch.int32)}
    if return_path:
        out["path"] = res["path"]
    return out
