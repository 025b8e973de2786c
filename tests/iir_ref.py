"""The CPU oracle of the IIR filtering tests (numpy + scipy, no GPU, no library): scipy's sosfilt on fp64 (`reference`), the same
recursion as a plain loop in np.longdouble (`reference_long`), the yardstick E = what fp64 itself costs a case (`error`), the closed forms
of the Butterworth designs (`butter_formula`), and `restate`: the three phases of DESIGN.md section 3.24 in numpy fp64, operation for
operation those of kernels/iir.hip and kernels/pair.hpp, together with the pair-arithmetic design of M (`design_matrix`).

The product's error term comes from math.fma where the interpreter has it, else from Dekker's exact product: the same value (no
product here comes near fp64's overflow or underflow)."""
import functools
import math

import numpy as np
from scipy import signal

SEG = 256
FILTERS = {  # name -> order, cutoff in Hz, sample rate, kind
    "F1": (4, 50.0, 16000, "highpass"),
    "F2": (2, 20.0, 48000, "highpass"),  # the near-double pole that needs the pairs
    "F3": (8, 7000.0, 16000, "lowpass"),
    "F4": (5, 300.0, 16000, "highpass"),  # a first-order section inside
    "F5": (16, 3200.0, 16000, "lowpass"),  # the widest M
}
LENGTHS = (1, SEG - 1, SEG, SEG + 1, 64 * SEG - 1, 64 * SEG, 64 * SEG + 1, 130 * SEG + 7)


# ---- designs -------------------------------------------------------------------------------------------------------------------------------
def butter_formula(order, cutoff_hz, sample_rate, kind):
    """The definition of butter_sos, in numpy fp64: (ceil(order / 2), 6) rows b0 b1 b2 1 a1 a2."""
    hp = kind == "highpass"
    K = np.tan(np.pi * cutoff_hz / sample_rate)
    rows = []
    if order % 2:
        b = np.array([1.0, -1.0, 0.0]) if hp else np.array([K, K, 0.0])
        rows.append(np.concatenate([b / (1.0 + K), [1.0, (K - 1.0) / (K + 1.0), 0.0]]))
    for k in range(order // 2):
        q = 2.0 * np.sin(np.pi * (2 * k + 1) / (2.0 * order))
        a0 = 1.0 + q * K + K * K
        b = np.array([1.0, -2.0, 1.0]) if hp else np.array([K * K, 2.0 * K * K, K * K])
        rows.append(np.concatenate([b / a0, [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - q * K + K * K) / a0]]))
    return np.array(rows)


# ---- signals ---------------------------------------------------------------------------------------------------------------------------------
def clip_signal(n, fs, seed=5):
    """Five harmonics of 220 Hz at amplitudes 1 / k with 3 Hz amplitude modulation, seeded noise at 0.01 and a DC offset of 0.1, scaled
    by 0.25; one eighth of the clip is zeroed abruptly in its middle, so that the output there is a free decay.  fp32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = sum(np.sin(2 * np.pi * 220.0 * k * t + 2 * np.pi * rng.random()) / k for k in range(1, 6))
    x = 0.25 * x * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.01 * rng.standard_normal(n) + 0.1
    x[n // 2 - n // 16:n // 2 - n // 16 + n // 8] = 0.0
    return x.astype(np.float32)



# ---- the sequential filter -------------------------------------------------------------------------------------------------------------------
def reference(sos, x):
    """scipy.signal.sosfilt on fp64."""
    return signal.sosfilt(np.array(sos, dtype=np.float64), np.array(x, dtype=np.float64))


def reference_long(sos, x):
    """The same recursion as a plain loop over the samples in np.longdouble; x is one clip (n,) or clips side by side (clips, n): the
    loop is the same for each."""
    sos = np.asarray(sos, dtype=np.float64)
    x = np.asarray(x, dtype=np.longdouble)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    c = (sos / sos[:, 3:4]).astype(np.longdouble)
    s1 = [np.zeros(x.shape[0], dtype=np.longdouble) for _ in c]
    s2 = [np.zeros(x.shape[0], dtype=np.longdouble) for _ in c]
    y = np.empty_like(x)
    for i in range(x.shape[1]):
        v = x[:, i]
        for k, (b0, b1, b2, _, a1, a2) in enumerate(c):
            out = b0 * v + s1[k]
            s1[k] = b1 * v - a1 * out + s2[k]
            s2[k] = b2 * v - a2 * out
            v = out
        y[:, i] = v
    return y[0] if one else y


def error(a, b):
    """max |a - b| / max |b|: the yardstick of loudness' tests."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- pair arithmetic: pair.hpp, on numpy arrays or scalars -----------------------------------------------------------------------------------
_fma = np.frompyfunc(math.fma, 3, 1) if hasattr(math, "fma") else None


def _product_error(a, b, p):
    """a b - p exactly (fma(a, b, -p))."""
    if _fma is not None:
        return np.asarray(_fma(a, b, -p), dtype=np.float64)
    split = 134217729.0  # 2^27 + 1 (Dekker / Veltkamp)
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def pair_add(a, b):
    s = a[0] + b[0]
    bb = s - a[0]
    err = (a[0] - (s - bb)) + (b[0] - bb)
    return fast_two_sum(s, err + (a[1] + b[1]))


def pair_mul(a, b):
    p = a[0] * b[0]
    err = _product_error(a[0], b[0], p)
    return fast_two_sum(p, err + (a[0] * b[1] + a[1] * b[0]))


def pair_sub(a, b):
    return pair_add(a, (-b[0], -b[1]))


def _rows5(sos):
    sos = np.asarray(sos, dtype=np.float64)
    return (sos / sos[:, 3:4])[:, [0, 1, 2, 4, 5]]


def design_matrix(sos, seg=SEG):
    """sos_matrix_kernel: the cascade on `seg` zero samples from each unit state, in pair arithmetic (coefficients as (c, 0)); all the
    columns side by side -> (M hi, M lo), (2N, 2N) each, M[r][k] = state r reached from unit state k."""
    c = _rows5(sos)
    ns = 2 * len(c)
    zero = np.zeros(ns)
    st = [((np.arange(ns) == i).astype(np.float64), zero.copy()) for i in range(ns)]
    with np.errstate(all="ignore"):
        for _ in range(seg):
            v = (zero.copy(), zero.copy())
            for k, (b0, b1, b2, a1, a2) in enumerate(c):
                s1, s2 = st[2 * k], st[2 * k + 1]
                y = pair_add(pair_mul((b0, 0.0), v), s1)
                st[2 * k] = pair_add(pair_sub(pair_mul((b1, 0.0), v), pair_mul((a1, 0.0), y)), s2)
                st[2 * k + 1] = pair_sub(pair_mul((b2, 0.0), v), pair_mul((a2, 0.0), y))
                v = y
    return np.array([s[0] for s in st]), np.array([s[1] for s in st])


def _pass(c, xs, counts, start, want_y):
    """Phases A and C: every segment (row of xs) through the cascade from its row of `start`, its first counts[s] samples only -> (the
    end states, y)."""
    st = start.copy()
    y = np.zeros_like(xs)
    for j in range(xs.shape[1]):
        on = j < counts
        v = xs[:, j]
        for k, (b0, b1, b2, a1, a2) in enumerate(c):
            s1, s2 = st[:, 2 * k], st[:, 2 * k + 1]
            out = b0 * v + s1
            st[:, 2 * k] = np.where(on, b1 * v - a1 * out + s2, s1)
            st[:, 2 * k + 1] = np.where(on, b2 * v - a2 * out, s2)
            v = out
        if want_y:
            y[:, j] = np.where(on, v, 0.0)
    return st, y


def restate(sos, x, m_hi, m_lo, seg=SEG):
    """The three phases on one clip from rest, in numpy fp64 -> y (n,) fp64.  A: every segment from a zero state, its end state kept.
    B: start_{s+1} = M start_s + end_s over the complete segments, as pairs: row r of M times the state summed in column order from the
    first product, then the end state added.  C: every segment again from hi(start_s)."""
    c = _rows5(sos)
    ns = 2 * len(c)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    n_seg, n_whole = -(-n // seg), n // seg
    xs = np.zeros(n_seg * seg)
    xs[:n] = x
    xs = xs.reshape(n_seg, seg)
    counts = np.minimum(seg, n - seg * np.arange(n_seg))
    with np.errstate(all="ignore"):
        ends, _ = _pass(c, xs, counts, np.zeros((n_seg, ns)), False)
        starts = np.zeros((n_seg, ns))
        cur = (np.zeros(ns), np.zeros(ns))
        for s in range(n_seg):
            starts[s] = cur[0]
            if s >= n_whole:
                break
            acc = pair_mul((m_hi[:, 0], m_lo[:, 0]), (cur[0][0], cur[1][0]))
            for i in range(1, ns):
                acc = pair_add(acc, pair_mul((m_hi[:, i], m_lo[:, i]), (cur[0][i], cur[1][i])))
            cur = pair_add(acc, (ends[s], np.zeros(ns)))
        _, y = _pass(c, xs, counts, starts, True)
    return y.reshape(-1)[:n]


# ---- the cases the host and the GPU tests share ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_signals(name):
    """The test signal at every length of LENGTHS, at the filter's rate."""
    fs = FILTERS[name][2]
    return tuple(clip_signal(n, fs, seed=5 + i) for i, n in enumerate(LENGTHS))


@functools.lru_cache(maxsize=None)
def case_references(name, sos_bytes):
    """(reference, reference_long, E) per length for filter `name` with the coefficients `sos_bytes` (an (N, 6) fp64 array's bytes): the
    long loop runs once for all the lengths, the clips side by side (zeros after a clip's end change nothing before it)."""
    sos = np.frombuffer(sos_bytes, dtype=np.float64).reshape(-1, 6)
    xs = case_signals(name)
    side = np.zeros((len(xs), max(LENGTHS)))
    for i, x in enumerate(xs):
        side[i, :len(x)] = x
    long = reference_long(sos, side)
    out = []
    for i, x in enumerate(xs):
        ref, lng = reference(sos, x), long[i, :len(x)]
        out.append((ref, lng, error(ref, lng)))
    return tuple(out)
