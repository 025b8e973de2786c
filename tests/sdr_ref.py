"""fp64 numpy oracle of the library's BSS Eval SDR (include/l3ac_hip.h, 'BSS Eval SDR').  It executes the specified
programme in the specified order: the 64 interleaved partial sums and their fold of the correlations and of the recursion's inner sums, the
Levinson recursion with a general right-hand side, the residual tap by tap, and the energies by segment, thread, wave and workgroup.  numpy's
elementwise fp64 operations round once each and do not contract.  Its inputs are fp32 samples; nothing here calls the library."""
import numpy as np

U = 2.0 ** -52  # one ulp of an fp64 value v is at most U |v|
SEGMENT = 4096
MAX_TAPS = 1024


def lane_sum(terms):
    """(..., M) terms -> (...): partial l takes the terms i = l mod 64 in increasing i from +0, then p[l] += p[l + h] for h = 32 .. 1.
    (Padding a partial with +0 terms does not change its bits: it starts at +0 and so is never -0.)"""
    terms = np.asarray(terms, dtype=np.float64)
    lead, m = terms.shape[:-1], terms.shape[-1]
    rows = -(-m // 64)
    padded = np.zeros(lead + (rows * 64,), dtype=np.float64)
    padded[..., :m] = terms
    s = np.zeros(lead + (64,), dtype=np.float64)
    for r in range(rows):
        s = s + padded[..., 64 * r:64 * r + 64]
    h = 32
    while h >= 1:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def correlate(u, v, lags):
    """corr(u, v)[k] = sum_{t=0}^{n-1-k} u[t] v[t+k], k = 0 .. lags-1, +0 for k >= n.  fp32 (n,) each -> (lags,) fp64."""
    u, v = np.asarray(u, dtype=np.float32).astype(np.float64), np.asarray(v, dtype=np.float32).astype(np.float64)
    n = len(u)
    assert len(v) == n and n >= 1
    tail = np.concatenate([v, np.zeros(lags, dtype=np.float64)])
    at = np.arange(lags)[:, None] + np.arange(n)[None, :]
    with np.errstate(all="ignore"):
        terms = np.where(at < n, u[None, :] * tail[at], 0.0)  # a term outside the clip is not there: +0, not u * 0
        return lane_sum(terms)


def toeplitz_solve(r, b):
    """G c = b with G[i][j] = r[|i - j|] by the Levinson recursion in the stated order -> {"x", "error" (E_{L-1}), "valid"}; x and error NaN
    for an invalid system."""
    r, b = np.asarray(r, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = len(r)
    assert len(b) == n and 1 <= n <= MAX_TAPS
    with np.errstate(all="ignore"):
        valid = bool(r[0] > 0.0)
        a = np.zeros(n, dtype=np.float64)
        a[0] = 1.0
        e = r[0]
        c = np.zeros(n, dtype=np.float64)
        c[0] = b[0] / r[0]
        for m in range(1, n):
            i = np.arange(1, m)
            acc = r[m] + lane_sum(a[i] * r[m - i])
            km = -acc / e
            new = a.copy()
            new[i] = a[i] + km * a[m - i]
            new[m] = km
            a = new
            e = e * (1.0 - km * km)
            valid = valid and bool(e > 0.0)  # (once false it stays false; what an invalid system computes afterwards is discarded)
            i = np.arange(0, m)
            lam = b[m] - lane_sum(c[i] * r[m - i])
            nu = lam / e
            c[i] = c[i] + nu * a[m - i]
            c[m] = nu
    if not valid:
        return {"x": np.full(n, np.nan), "error": np.nan, "valid": 0}
    return {"x": c, "error": float(e), "valid": 1}


def block_sum(per_thread):
    """(..., 256) -> (...): a xor tree inside each wave of 64 (lane 0's value is the fold's), then the four waves' results from +0 in wave
    order."""
    w = per_thread.reshape(per_thread.shape[:-1] + (4, 64))
    h = 32
    while h >= 1:
        w = w[..., :h] + w[..., h:2 * h]
        h //= 2
    s = np.zeros(per_thread.shape[:-1], dtype=np.float64)
    for k in range(4):
        s = s + w[..., k, 0]
    return s


def energy(values):
    """sum of values^2 over the outputs: segments of 4096; thread i of 256 takes t = 4096 q + i + 256 j in increasing j from +0; block_sum;
    the segments from +0 in increasing q.  (Squares are never -0, so padding with +0 changes no bit.)"""
    m = len(values)
    segs = -(-m // SEGMENT)
    padded = np.zeros(segs * SEGMENT, dtype=np.float64)
    with np.errstate(all="ignore"):
        padded[:m] = values * values
        grid = padded.reshape(segs, 16, 256)
        thread = np.zeros((segs, 256), dtype=np.float64)
        for j in range(16):
            thread = thread + grid[:, j, :]
        per_seg = block_sum(thread)
        total = 0.0
        for q in range(segs):
            total = total + per_seg[q]
    return float(total)


def residual(s, est, c):
    """y[t] = sum_k c[k] s[t-k] from +0 in increasing k over the k with 0 <= t-k < n, e[t] = (t < n ? est[t] : 0) - y[t], t = 0 .. n+L-2
    -> (T, D, y, e)."""
    s64, e64 = np.asarray(s, dtype=np.float32).astype(np.float64), np.asarray(est, dtype=np.float32).astype(np.float64)
    n, taps = len(s64), len(c)
    y = np.zeros(n + taps - 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(taps):
            y[k:k + n] = y[k:k + n] + c[k] * s64
        e = np.concatenate([e64, np.zeros(taps - 1, dtype=np.float64)]) - y
    return energy(y), energy(e), y, e


def sdr(s, est, filter_length=512, load=0.0):
    """One pair -> {"sdr_db", "target_energy", "error_energy", "prediction_error", "valid", "filter", "autocorr", "crosscorr"}."""
    r = correlate(s, s, filter_length)
    b = correlate(s, est, filter_length)
    if load != 0.0:
        r[0] = r[0] * (1.0 + load)
    sol = toeplitz_solve(r, b)
    out = {"autocorr": r, "crosscorr": b, "filter": sol["x"], "prediction_error": sol["error"], "valid": sol["valid"]}
    if not sol["valid"]:
        out.update(sdr_db=np.nan, target_energy=np.nan, error_energy=np.nan)
        return out
    t, d, _, _ = residual(s, est, sol["x"])
    with np.errstate(all="ignore"):
        out.update(sdr_db=float(10.0 * np.log10(np.float64(t) / np.float64(d))), target_energy=t, error_energy=d)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def white(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def resonator(n, seed):
    """White noise through the two-pole resonator 1.8, -0.9, scaled to a peak of 1."""
    w = np.random.default_rng(seed).standard_normal(n)
    x = np.zeros(n, dtype=np.float64)
    for t in range(n):
        x[t] = w[t] + (1.8 * x[t - 1] if t > 0 else 0.0) - (0.9 * x[t - 2] if t > 1 else 0.0)
    return (x / np.abs(x).max()).astype(np.float32)


def distorted(s, seed, noise_db=30.0):
    """0.5 s[t - 17] - 0.2 s[t - 3] plus white noise `noise_db` below the clip's own power: a linear distortion that sample-by-sample
    measures score as noise."""
    s64 = np.asarray(s, dtype=np.float64)
    n = len(s64)
    h = np.zeros(18)
    h[17], h[3] = 0.5, -0.2
    y = np.convolve(s64, h)[:n]
    sigma = np.sqrt(np.mean(s64 * s64)) * 10.0 ** (-noise_db / 20.0)
    return (y + sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def snr_db(s, est):
    s64, e64 = np.asarray(s, dtype=np.float64), np.asarray(est, dtype=np.float64)
    return float(10.0 * np.log10(np.sum(s64 * s64) / np.sum((s64 - e64) ** 2)))
