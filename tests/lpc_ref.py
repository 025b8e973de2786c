"""fp64 numpy oracle of the library's linear prediction and envelope measures (include/l3ac_hip.h, 'linear prediction'; DESIGN.md section
3.18).  It executes the specified programme in the specified order: the 64 interleaved partial sums and their fold, the Levinson-Durbin
recursion, the quadratic forms, the cepstrum recursion, the sort and the trimmed sum.  Every function works on all the frames of one clip
at once; the order of the operations inside a frame is the stated one (numpy's elementwise fp64 operations round once each and do not
contract).  Its inputs are fp32 samples and the library's own fp32 window; nothing here calls the library."""
import numpy as np

DB = 4.342944819032518  # 10 / ln 10
U = 2.0 ** -52          # one ulp of an fp64 value v is at most U |v|
LLR_MAX, IS_MAX, CD_MAX = 2.0, 100.0, 10.0


def defaults(fs):
    frame = (30 * fs + 500) // 1000
    return (10 if fs < 10000 else 16), frame, frame // 4


def window_design(n):
    """The fp64 design of the asymmetric Hann window."""
    i = np.arange(n, dtype=np.float64)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (i + 1.0) / (n + 1.0)))


def window(n, kind="hann"):
    return window_design(n).astype(np.float32) if kind == "hann" else np.ones(n, dtype=np.float32)


def n_frames(samples, n, hop):
    return 0 if samples < n else 1 + (samples - n) // hop


def frames_xw(x, w, n, hop):
    """(F, N) fp64: the windowed frames of one clip of fp32 samples, each product exact."""
    x = np.asarray(x, dtype=np.float32)
    f = n_frames(len(x), n, hop)
    idx = np.arange(f)[:, None] * hop + np.arange(n)[None, :]
    return x[idx].astype(np.float64) * np.asarray(w, dtype=np.float32).astype(np.float64)[None, :]


def lane_sum(terms):
    """(F, M) terms -> (F,): partial l takes the terms i = l mod 64 in increasing i from +0, then s[l] += s[l + h] for h = 32 .. 1.
    (Padding a partial with +0 terms does not change its bits: it starts at +0 and so is never -0.)"""
    f, m = terms.shape
    rows = -(-m // 64)
    padded = np.zeros((f, rows * 64), dtype=np.float64)
    padded[:, :m] = terms
    s = np.zeros((f, 64), dtype=np.float64)
    for r in range(rows):
        s = s + padded[:, 64 * r:64 * r + 64]
    h = 32
    while h >= 1:
        s = s[:, :h] + s[:, h:2 * h]
        h //= 2
    return s[:, 0]


def autocorr(xw, p):
    """(F, N) -> (F, p + 1)."""
    n = xw.shape[1]
    return np.stack([lane_sum(xw[:, :n - k] * xw[:, k:]) for k in range(p + 1)], axis=1)


def levinson(r):
    """(F, p + 1) -> a (F, p + 1), reflection (F, p), error (F,), valid (F,) bool; NaN in a, reflection and error of an invalid frame."""
    f, p1 = r.shape
    p = p1 - 1
    a = np.zeros((f, p1), dtype=np.float64)
    a[:, 0] = 1.0
    refl = np.zeros((f, p), dtype=np.float64)
    with np.errstate(all="ignore"):
        valid = r[:, 0] > 0.0
        e = r[:, 0].copy()
        for m in range(1, p + 1):
            acc = r[:, m].copy()
            for i in range(1, m):
                acc = acc + a[:, i] * r[:, m - i]
            km = -acc / e
            new = a.copy()
            for i in range(1, m):
                new[:, i] = a[:, i] + km * a[:, m - i]
            new[:, m] = km
            a = new
            refl[:, m - 1] = km
            e = e * (1.0 - km * km)
            valid = valid & (e > 0.0)  # (once false it stays false; what an invalid frame computes afterwards is discarded)
    a[~valid] = np.nan
    refl[~valid] = np.nan
    return a, refl, np.where(valid, e, np.nan), valid


def quad(a, r):
    """q(a, r) = sum_i a[i] (sum_j r[|i - j|] a[j]), both sums from +0 in increasing index.  (F, p + 1) each -> (F,)."""
    f, p1 = a.shape
    with np.errstate(all="ignore"):
        q = np.zeros(f, dtype=np.float64)
        for i in range(p1):
            inner = np.zeros(f, dtype=np.float64)
            for j in range(p1):
                inner = inner + r[:, abs(i - j)] * a[:, j]
            q = q + a[:, i] * inner
    return q


def cepstrum(a):
    """c[1..p] of 1 / A: (F, p + 1) -> (F, p + 1) with column 0 unused (zero)."""
    f, p1 = a.shape
    c = np.zeros((f, p1), dtype=np.float64)
    with np.errstate(all="ignore"):
        c[:, 1] = -a[:, 1]
        for m in range(2, p1):
            s = np.zeros(f, dtype=np.float64)
            for k in range(1, m):
                s = s + ((np.float64(k) / np.float64(m)) * c[:, k]) * a[:, m - k]
            c[:, m] = -a[:, m] - s
    return c


def clamp(v, lo, hi):
    """v < lo -> lo, v > hi -> hi, NaN stays."""
    with np.errstate(all="ignore"):
        return np.where(v < lo, lo, np.where(v > hi, hi, v))


def lpc(x, fs=16000, order=None, frame=None, hop=None, kind="hann", w=None):
    d = defaults(fs)
    p, n = d[0] if order is None else order, d[1] if frame is None else frame
    hop = n // 4 if hop is None else hop
    w = window(n, kind) if w is None else w
    xw = frames_xw(x, w, n, hop)
    r = autocorr(xw, p)
    a, refl, err, valid = levinson(r)
    return {"a": a, "reflection": refl, "error": err, "autocorr": r, "valid": valid.astype(np.int32), "xw": xw}


def frame_values(ref, est, llr_max=LLR_MAX, is_max=IS_MAX, cd_max=CD_MAX):
    """The frames' forms and clamped values from ``lpc`` of each side (dicts with "a", "autocorr", "valid", "xw")."""
    both = (ref["valid"] != 0) & (est["valid"] != 0)
    with np.errstate(all="ignore"):
        num, g_r, g_e = quad(est["a"], ref["autocorr"]), quad(ref["a"], ref["autocorr"]), quad(est["a"], est["autocorr"])
        num, g_r, g_e = (np.where(both, v, np.nan) for v in (num, g_r, g_e))
        ratio = num / g_r
        raw_llr, log_g = np.log(ratio), np.log(g_e / g_r)
        raw_sum = (g_r / g_e) * ratio + log_g
        raw_is = raw_sum - 1.0
        llr = clamp(raw_llr, 0.0, llr_max)
        is_d = clamp(raw_is, 0.0, is_max)
        d = cepstrum(ref["a"])[:, 1:] - cepstrum(est["a"])[:, 1:]
        sq = np.zeros(len(both), dtype=np.float64)
        for m in range(d.shape[1]):
            sq = sq + d[:, m] * d[:, m]
        raw_cd = DB * np.sqrt(2.0 * sq)
        cd = clamp(raw_cd, 0.0, cd_max)
        llr, is_d, cd = (np.where(both, v, np.nan) for v in (llr, is_d, cd))
        sig = ref["autocorr"][:, 0]
        diff = ref["xw"] - est["xw"]
        noise = lane_sum(diff * diff)
        counted = sig > 0.0
        raw_snr = 10.0 * np.log10(sig / noise)
        snr = np.where(noise == 0.0, 35.0, clamp(raw_snr, -10.0, 35.0))
        snr = np.where(counted, snr, np.nan)
        # DESIGN.md section 3.18, "the log stage": the forms are bit-exact, log and log10 are within 1 ulp of the truth on either side
        # (2 ulp apart), sqrt within 1 ulp apart; every later operation adds one ulp of its result; a clamp widens nothing
        bounds = {"llr": 2.0 * U * np.abs(raw_llr), "is": 2.0 * U * np.abs(log_g) + U * np.abs(raw_sum) + U * np.abs(raw_is),
                  "cd": 2.0 * U * np.abs(raw_cd), "snr": np.where(noise == 0.0, 0.0, 3.0 * U * np.abs(raw_snr))}
    return {"llr": llr, "is": is_d, "cd": cd, "snr": snr, "both": both, "counted": counted,
            "forms": np.stack([num, g_r, g_e, sig, noise], axis=1), "bounds": bounds}


def mean_bound(values, bounds, k):
    """What a mean over k of ``values`` may differ by when each value may differ by its bound: the largest bound (the sorted sequence moves
    by no more than its entries do), plus one ulp of a partial sum per addition and one for the division."""
    if k == 0 or len(values) == 0:
        return 0.0
    return float(np.max(bounds) + (k + 1) * U * np.max(np.abs(values)))


def trim_count(trim, v):
    return int(np.floor(np.float64(trim) * np.float64(v) + 0.5))


def trimmed_mean(values, trim):
    """The V values sorted ascending, the first k = floor(trim V + 0.5) summed in that order from +0, over k; NaN for V = 0 or k = 0."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    k = trim_count(trim, len(v))
    if len(v) == 0 or k == 0:
        return np.nan
    s = np.float64(0.0)
    for x in v[:k]:
        s = s + x
    return s / np.float64(k)


def ordered_mean(values):
    if len(values) == 0:
        return np.nan
    s = np.float64(0.0)
    for x in values:
        s = s + x
    return s / np.float64(len(values))


def pair_values(fv, trim=0.95):
    """The pair's four values and three counts from ``frame_values``' result."""
    both, counted = fv["both"], fv["counted"]
    k = trim_count(trim, int(both.sum()))
    b = fv["bounds"]
    return {"llr": trimmed_mean(fv["llr"][both], trim), "is_distance": trimmed_mean(fv["is"][both], trim),
            "cepstral_distance_db": trimmed_mean(fv["cd"][both], trim), "seg_snr_db": ordered_mean(fv["snr"][counted]),
            "frames": len(both), "lpc_frames": int(both.sum()), "snr_frames": int(counted.sum()),
            "bounds": {"llr": mean_bound(fv["llr"][both], b["llr"][both], k), "is_distance": mean_bound(fv["is"][both], b["is"][both], k),
                       "cepstral_distance_db": mean_bound(fv["cd"][both], b["cd"][both], k),
                       "seg_snr_db": mean_bound(fv["snr"][counted], b["snr"][counted], int(counted.sum()))}}


def metrics(ref, est, fs=16000, order=None, frame=None, hop=None, kind="hann", trim=0.95, llr_max=LLR_MAX, is_max=IS_MAX, cd_max=CD_MAX):
    """One pair of fp32 clips of equal length -> (pair values, frame values)."""
    a, b = lpc(ref, fs, order, frame, hop, kind), lpc(est, fs, order, frame, hop, kind)
    fv = frame_values(a, b, llr_max, is_max, cd_max)
    return pair_values(fv, trim), fv


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def resonator(samples, fs, seed, poles=((500.0, 0.97), (1500.0, 0.95), (2500.0, 0.93)), noise=1e-3):
    """White noise through a cascade of two-pole resonators, scaled to a peak of 0.5, plus a little white noise: speech-like envelopes."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(samples + 200)
    for f0, rad in poles:
        b1, b2 = 2.0 * rad * np.cos(2.0 * np.pi * f0 / fs), -rad * rad
        out = np.zeros_like(y)
        for i in range(len(y)):
            out[i] = y[i] + (b1 * out[i - 1] if i >= 1 else 0.0) + (b2 * out[i - 2] if i >= 2 else 0.0)
        y = out
    y = y[200:]
    y = 0.5 * y / np.abs(y).max()
    return (y + noise * rng.standard_normal(samples)).astype(np.float32)


def sine_plus_noise(samples, fs, seed, freq=440.0, noise=1e-4):
    rng = np.random.default_rng(seed)
    t = np.arange(samples, dtype=np.float64)
    return (0.5 * np.sin(2.0 * np.pi * freq * t / fs) + noise * rng.standard_normal(samples)).astype(np.float32)


def add_noise(x, snr_db, seed):
    """x plus white noise at ``snr_db`` below x's own power."""
    rng = np.random.default_rng(seed)
    x64 = np.asarray(x, dtype=np.float64)
    g = np.sqrt(np.mean(x64 * x64) / 10.0 ** (snr_db / 10.0))
    return (x64 + g * rng.standard_normal(len(x64))).astype(np.float32)
