"""The fp64 oracle of the time alignment, in NumPy, written from the specification alone: the cross-correlation
in the direct form with the sum of absolute products beside it, the energies, the pick, `refine`, the pick and the refinement restated
on a given row; `robust`, whether the pick has a margin over what the fp32 products may cost; the specification's matrix form in fp64
(`gemm_form`, for the identity); the shift; and the suite's inputs."""
import functools
import math

import numpy as np

U32 = 2.0 ** -24  # fp32 unit roundoff
U64 = 2.0 ** -53
S, R = 4096, 128  # samples of a segment, terms of one fp32 chain
MAX_LAG = 16384


def gamma_r():
    """An fp32 fmaf chain of R terms from 0: within gamma_R of its own sum of absolute products."""
    return R * U32 / (1 - R * U32)


def beta(n):
    """|r_library(d) - r_oracle(d)| <= beta A(d): gamma_R from the fp32 chains; 32 G + 8 fp64 roundings of the diagonal and segment sums;
    and the oracle's own pairwise fp64 sum of n exact products, log2(n) + 24 roundings at most (NumPy sums blocks of 128 in 8 lanes)."""
    g = -(-n // S)
    return gamma_r() + (32 * g + 8) * U64 + (math.ceil(math.log2(max(n, 2))) + 24) * U64


def xcorr(ref, est, max_lag):
    """-> (r, A), each (2 L + 1,) fp64: r(d) = sum_j ref[j] est[j + d] and A(d) = sum_j |ref[j]| |est[j + d]| over the overlap."""
    x, y = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    n = len(x)
    assert len(y) == n and 0 <= max_lag <= MAX_LAG
    r, a = np.zeros(2 * max_lag + 1), np.zeros(2 * max_lag + 1)
    for d in range(-max_lag, max_lag + 1):
        m = n - abs(d)
        if m <= 0:
            continue
        p = x[max(0, -d):max(0, -d) + m] * y[max(0, d):max(0, d) + m]  # (exact: two fp32 factors)
        r[d + max_lag], a[d + max_lag] = p.sum(), np.abs(p).sum()
    return r, a


def energies(ref, est):
    x, y = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    return float((x * x).sum()), float((y * y).sum())


def pick(r):
    """Index of d*: the largest |r|, among equals the smallest |d|, then the smallest d.  NaN entries are never taken."""
    max_lag = (len(r) - 1) // 2
    best, at = -1.0, max_lag
    for i in sorted(range(len(r)), key=lambda i: (abs(i - max_lag), i)):
        if abs(r[i]) > best:
            best, at = abs(r[i]), i
    return at


def refine(r, e_ref, e_est):
    """The pick and the refinement on a given row -> (lag, polarity, delay, correlation), in the specification's operations and order."""
    r = np.asarray(r, dtype=np.float64)
    max_lag = (len(r) - 1) // 2
    prod = np.float64(e_ref) * np.float64(e_est)
    if prod == 0.0:
        return 0, 0, 0.0, math.nan
    at = pick(r)
    s = np.float64(-1.0 if r[at] < 0.0 else 1.0)
    shift = np.float64(0.0)
    if 0 < at < 2 * max_lag:
        a, b, e = s * r[at - 1], s * r[at], s * r[at + 1]
        den = (a - 2.0 * b) + e
        if den < 0.0:
            shift = (0.5 * (a - e)) / den
    return at - max_lag, int(s), float(np.float64(at - max_lag) + shift), float(r[at] / np.sqrt(prod))


def robust(r, a, e, bt):
    """Whether the pick and the polarity are the same in any arithmetic within `bt` A(d) of `r`: |r(d*)| - max_{d != d*} |r(d)| > 2 bt max
    A, and |r(d*)| > bt A(d*).  `e` = (E_ref, E_est): with a silent side nothing is picked, and exact zeros are zeros in any arithmetic."""
    if e[0] * e[1] == 0.0:
        return True
    at = pick(r)
    others = np.delete(np.abs(r), at)
    runner_up = others.max() if others.size else 0.0
    return bool(abs(r[at]) - runner_up > 2 * bt * a.max() and abs(r[at]) > bt * a[at])


def oracle(ref, est, max_lag):
    r, a = xcorr(ref, est, max_lag)
    e = energies(ref, est)
    lag, polarity, delay, correlation = refine(r, *e)
    bt = beta(len(ref))
    return dict(r=r, A=a, e_ref=e[0], e_est=e[1], lag=lag, polarity=polarity, delay=delay, correlation=correlation, beta=bt,
                robust=robust(r, a, e, bt), margin=margin(r, e))


def margin(r, e):
    """(|r(d*)| - the runner-up) / sqrt(E_ref E_est); inf with a single lag, nan with a silent side."""
    if e[0] * e[1] == 0.0:
        return math.nan
    at = pick(r)
    others = np.delete(np.abs(r), at)
    return math.inf if not others.size else float((abs(r[at]) - others.max()) / math.sqrt(e[0] * e[1]))


def gemm_form(ref, est, max_lag):
    """The specification's matrix form, in fp64: per segment g, A[a][k] = ref[g S + 32 k + a] and B[k][c] = est[g S + 32 k + c - L] with
    out-of-range entries 0, C_g = A B, r_g(d) = sum_a C_g[a][a + d + L], r = sum_g r_g."""
    x, y = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    n, cols = len(x), 32 + 2 * max_lag
    r = np.zeros(2 * max_lag + 1)
    for g in range(-(-n // S)):
        seg = np.zeros(S)
        seg[:min(S, n - g * S)] = x[g * S:g * S + S]
        a = seg.reshape(R, 32).T  # [a][k]
        lo = g * S - max_lag
        idx = lo + np.arange(S - 32 + cols)
        span = np.where((idx >= 0) & (idx < n), y[np.clip(idx, 0, n - 1)], 0.0)
        b = np.lib.stride_tricks.sliding_window_view(span, cols)[::32][:R]  # [k][c] = span[32 k + c]
        c = a @ b
        r += np.array([sum(c[i, i + d] for i in range(32)) for d in range(2 * max_lag + 1)])
    return r


def fma32(a, b, c):
    """fmaf on fp32 arrays, correctly rounded: the product of two fp32 is exact in fp64; TwoSum gives the fp64 sum s and what it lost;
    s and the exact value round to the same fp32 unless s is the midpoint of two fp32 neighbours, where what was lost decides."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    t = s - p
    lost = (p - (s - t)) + (c - t)
    r = s.astype(np.float32)
    up, down = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
    r64 = r.astype(np.float64)
    r = np.where((s == 0.5 * (r64 + up.astype(np.float64))) & (lost > 0), up, r)
    return np.where((s == 0.5 * (r64 + down.astype(np.float64))) & (lost < 0), down, r)


def chain_form(ref, est, max_lag):
    """The specification's arithmetic itself: `gemm_form` with C_g the fp32 fmaf chain over k = 0 .. R - 1 from 0, the diagonals summed
    in fp64 in the order of a and the segments in the order of g.  The library's row equals this bit for bit."""
    x, y = np.asarray(ref, dtype=np.float32), np.asarray(est, dtype=np.float32)
    n, cols, lags = len(x), 32 + 2 * max_lag, 2 * max_lag + 1
    r = np.zeros(lags)
    for g in range(-(-n // S)):
        seg = np.zeros(S, dtype=np.float32)
        seg[:min(S, n - g * S)] = x[g * S:g * S + S]
        a = seg.reshape(R, 32)  # [k][a]
        idx = g * S - max_lag + np.arange(S - 32 + cols)
        span = np.where((idx >= 0) & (idx < n), y[np.clip(idx, 0, n - 1)], np.float32(0.0))
        b = np.lib.stride_tricks.sliding_window_view(span, cols)[::32][:R]  # [k][c]
        c = np.zeros((32, cols), dtype=np.float32)
        for k in range(R):
            c = fma32(a[k][:, None], b[k][None, :], c)
        r_g = np.zeros(lags)
        for i in range(32):
            r_g = r_g + c[i, i:i + lags].astype(np.float64)
        r = r + r_g
    return r


def shift_pair(ref, est, lag):
    """What apply_delay returns for one pair of n samples -> (ref_aligned, est_aligned, m), rows of n samples with zeros from m on."""
    n = len(ref)
    m = max(0, n - abs(lag))
    out_r, out_e = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    out_r[:m] = ref[max(0, -lag):max(0, -lag) + m]
    out_e[:m] = est[max(0, lag):max(0, lag) + m]
    return out_r, out_e, m


# ---- the suite's inputs: (ref, est) fp32 pairs ----------------------------------------------------------------------------------------------
def delayed(x, d):
    """x late by d samples (early for d < 0), zeros shifted in: out[j + d] = x[j]."""
    out = np.zeros_like(x)
    n = len(x)
    if abs(d) < n:
        out[max(0, d):n + min(0, d)] = x[max(0, -d):n - max(0, d)]
    return out


def white(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def coloured(n, seed):
    """White noise through y[j] = 0.9 y[j - 1] + x[j]: neighbouring lags correlate at 0.9."""
    x = 0.05 * np.random.default_rng(seed).standard_normal(n)
    y = np.empty(n)
    acc = 0.0
    for j in range(n):
        acc = 0.9 * acc + x[j]
        y[j] = acc
    return y.astype(np.float32)


TONES = np.linspace(100.0, 800.0, 12)
SINES_N = 24000  # 1.5 s: the shrinking overlap n - |d| tilts the peak by about 1 / (n w^2) samples, w the signal's mean angular frequency
SINES_DELAYS = (12.3, -7.49, 0.25)


def sines(n, delay, fs=16000, seed=7):
    """12 tones at 100 .. 800 Hz with seeded phases, evaluated at j and at j - delay: a band-limited signal late by a fraction of a sample."""
    phase = np.random.default_rng(seed).uniform(0, 2 * np.pi, len(TONES))
    j = np.arange(n, dtype=np.float64)
    at = lambda t: (0.05 * np.sin(2 * np.pi * TONES[:, None] * t[None, :] / fs + phase[:, None])).sum(axis=0)
    return at(j).astype(np.float32), at(j - delay).astype(np.float32)


def tone_noise(n, shift, seed=11, fs=16000):
    """200 Hz plus white noise, the estimate late by `shift`: a periodic r whose peaks one period apart differ by the noise alone."""
    x = (0.2 * np.sin(2 * np.pi * 200.0 * np.arange(n) / fs) + 0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    return x, delayed(x, shift)


def integers(n, seed=3):
    """Integer-valued samples in [-8, 8], the two sides drawn apart: every product and every partial sum is exact in fp32."""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, n).astype(np.float32), rng.integers(-8, 9, n).astype(np.float32)


def noisy_copy(n, shift, seed=0):
    """White noise and a copy of it late by `shift` with a tenth of other noise on top: the pair of the edge shapes."""
    ref = white(n, 100 + seed)
    return ref, (delayed(ref, shift) + np.float32(0.1) * white(n, 200 + seed)).astype(np.float32)


# name -> (n, max_lag, shift): the shapes at which the kernels take another path.  A segment is 4096 samples, a k row 32, a block of lags 224.
EDGES = {f"n = {n}": (n, 20, 3 if n > 8 else 0) for n in (1, 31, 32, 33, 4095, 4096, 4097, 8192 + 1)}
EDGES.update({f"L = {lag}": (5000, lag, (lag + 1) // 2) for lag in (0, 1, 15, 16, 17, 31, 32, 33)})
EDGES.update({
    "L above n: n = 70, L = 100": (70, 100, 3),
    "L = n = 33": (33, 33, -2),
    "lag at +L": (5000, 24, 24),
    "lag at -L": (5000, 24, -24),
    "223 lags: one block, all of it": (6000, 111, -90),
    "225 lags: a second block of one lag": (6000, 112, 112),
    "601 lags: three blocks": (6000, 300, -150),
    "n = 48000, L = 1600": (48000, 1600, 1234),
})


@functools.lru_cache(maxsize=None)
def known_cases():
    """name -> (ref, est, max_lag, true lag, true polarity): the inputs with known answers (white and coloured noise, an inverted copy,
    the sine mixture at its three delays).  Shared and never written to."""
    w, c, v = white(6000, 1), coloured(5000, 2), white(4500, 4)
    return {
        "white +37": (w, delayed(w, 37), 64, 37, 1),
        "coloured -48 at L = 48": (c, delayed(c, -48), 48, -48, 1),
        "inverted": (v, -delayed(v, 5), 20, 5, -1),
        "sines 12.3": sines(SINES_N, 12.3) + (32, 12, 1),
        "sines -7.49": sines(SINES_N, -7.49) + (32, -7, 1),
        "sines 0.25": sines(SINES_N, 0.25) + (32, 0, 1),
    }
