"""fp64 numpy restatement of the library's sample-rate conversion (include/l3ac_hip.h, 'sample-rate conversion'):
scipy.signal.resample_poly with its default window, written out from its definition so that the GPU tests need no scipy.

For in_rate a, out_rate b: g = gcd(a, b), up = b / g, down = a / g, M = max(up, down), half_len = 10 M,
h = firwin(2 half_len + 1, 1 / M, window=('kaiser', 5.0)) * up, n_out = ceil(n_in up / down) and
    y[m] = sum_j h[j] xu[m down + half_len - j],   xu[n] = x[n / up] if up | n and 0 <= n / up < n_in, else 0.
"""
from __future__ import annotations

import math

import numpy as np

MAX_FACTOR = 1024


def factors(in_rate: int, out_rate: int):
    """(up, down) reduced; ValueError for rates the library does not support."""
    if in_rate <= 0 or out_rate <= 0:
        raise ValueError(f"rates must be positive: {in_rate} -> {out_rate}")
    g = math.gcd(in_rate, out_rate)
    up, down = out_rate // g, in_rate // g
    if max(up, down) > MAX_FACTOR:
        raise ValueError(f"{in_rate} -> {out_rate}: max(up, down) = {max(up, down)} > {MAX_FACTOR}")
    return up, down


def out_length(in_rate: int, out_rate: int, n_in: int) -> int:
    up, down = factors(in_rate, out_rate)
    return -(-n_in * up // down)


def prototype(in_rate: int, out_rate: int) -> np.ndarray:
    """h (fp64, length 2 half_len + 1): firwin's windowed sinc, unit DC gain, times up."""
    up, down = factors(in_rate, out_rate)
    M = max(up, down)
    half_len = 10 * M
    n = 2 * half_len + 1
    alpha = 0.5 * (n - 1)
    m = np.arange(n, dtype=np.float64) - alpha
    c = 1.0 / M
    h = c * np.sinc(c * m) * (np.i0(5.0 * np.sqrt(1.0 - (m / alpha) ** 2)) / np.i0(5.0))
    return h / h.sum() * up


def polyphase_taps(in_rate: int, out_rate: int):
    """(h, K, phase bank [up][K] with g_p[k] = h[p + k up], 0 past the end of h)."""
    up, _ = factors(in_rate, out_rate)
    h = prototype(in_rate, out_rate)
    K = -(-h.size // up)
    idx = np.arange(up)[:, None] + np.arange(K)[None, :] * up
    return h, K, np.where(idx < h.size, h[np.minimum(idx, h.size - 1)], 0.0)


def resample_ref(x, in_rate: int, out_rate: int, chunk: int = 4096):
    """x (B, T) -> (y (B, n_out) fp64, absdot (B, n_out) = sum_k |h_k x_k| over each output's terms)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None]
    b, t = x.shape
    n_out = out_length(in_rate, out_rate, t)
    if in_rate == out_rate:
        return x.copy(), np.abs(x)
    up, down = factors(in_rate, out_rate)
    half_len = 10 * max(up, down)
    _, K, bank = polyphase_taps(in_rate, out_rate)
    y = np.empty((b, n_out))
    absdot = np.empty((b, n_out))
    k = np.arange(K)
    for m0 in range(0, n_out, chunk):
        m = np.arange(m0, min(n_out, m0 + chunk), dtype=np.int64)
        q = m * down + half_len
        taps = bank[q % up]                          # [n][K]
        xi = (q // up)[:, None] - k[None, :]         # newest input first
        ok = (xi >= 0) & (xi < t)
        xv = np.where(ok[None], x[:, np.clip(xi, 0, t - 1)], 0.0)  # [B][n][K]
        prod = taps[None] * xv
        y[:, m0:m0 + m.size] = prod.sum(-1)
        absdot[:, m0:m0 + m.size] = np.abs(prod).sum(-1)
    return y, absdot
