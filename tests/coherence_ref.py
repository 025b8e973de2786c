"""The fp64 oracle of the coherence measures in NumPy: the radix-2 network of tests/bands_ref.py on the library's
twiddle table, the frame energies and level classes, the cross-spectral sums in the stated order, the coherence, the band mapping and the
class values, with the error bounds of what lies behind a ``log10`` or an ``exp``; and a plain ``numpy.fft`` restatement of CSII that shares
nothing with it but the formulas.  Tests only; no GPU import here."""
import numpy as np

from tests.bands_ref import LOG10_ULP, SLACK, runs, spectrum
from tests.lpc_ref import U, frames_xw, lane_sum, n_frames, window  # noqa: F401

EXP_ULP = 1.0 + 1.0  # the device's and NumPy's exp, 1 ulp each as HIP's and glibc's documentation state

CENTRES = (150.0, 250.0, 350.0, 450.0, 570.0, 700.0, 840.0, 1000.0, 1170.0, 1370.0, 1600.0, 1850.0, 2150.0, 2500.0, 2900.0, 3400.0, 4000.0, 4800.0,
           5800.0, 7000.0, 8500.0)
LOWER = (100.0, 200.0, 300.0, 400.0, 510.0, 630.0, 770.0, 920.0, 1080.0, 1270.0, 1480.0, 1720.0, 2000.0, 2320.0, 2700.0, 3150.0, 3700.0, 4400.0,
         5300.0, 6400.0, 7700.0)
UPPER = LOWER[1:] + (9500.0,)
IMPORTANCE = (0.0103, 0.0261, 0.0419) + (0.0577,) * 14 + (0.0460, 0.0343, 0.0226, 0.0110)


def sii_table(fs=None):
    """(centres, bandwidths, importances) of the bands whose upper edge is at or below fs / 2; all 21 without a rate."""
    keep = 21 if fs is None else sum(1 for u in UPPER if u <= fs / 2.0)
    return CENTRES[:keep], tuple(u - l for u, l in zip(UPPER, LOWER))[:keep], IMPORTANCE[:keep]


def group_frames(n_fft):
    return 16 if n_fft <= 256 else (8 if n_fft <= 1024 else (4 if n_fft == 2048 else 2))


def chunk_frames(n_fft):
    """The frames whose products are summed in one chain: four groups."""
    return 4 * group_frames(n_fft)


# ---- the level classes ----------------------------------------------------------------------------------------------------------------------
def classify(xw):
    """(F, N) windowed frames of the reference -> (E (F,), classes (F,) int32, counts (4,)).  E_t as 64 interleaved partials over j, S the
    same over t, M = S / F; every threshold product rounds once."""
    f = xw.shape[0]
    if f == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(4, dtype=np.int32)
    with np.errstate(all="ignore"):
        e = lane_sum(xw * xw)
        s = lane_sum(e[None, :])[0]
        mean = s / np.float64(f)
        mid, low = np.float64(0.1) * mean, np.float64(0.001) * mean
        cls = np.where(e >= mean, 0, np.where(e >= mid, 1, np.where(e >= low, 2, 3))).astype(np.int32)
    if s == 0.0:
        cls[:] = 3
    return e, cls, np.bincount(cls, minlength=4).astype(np.int32)


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------------
def products(ref, est):
    """``bands_ref.spectrum`` of each side -> (F, 4, h): Pxx, Pyy, Cre, Cim of every frame and bin, each product and sum rounded on its own."""
    xr, xi, yr, yi = ref["re"], ref["im"], est["re"], est["im"]
    with np.errstate(all="ignore"):
        return np.stack([xr * xr + xi * xi, yr * yr + yi * yi, xr * yr + xi * yi, xi * yr - xr * yi], axis=1)


def class_sums(prod, cls, n_fft):
    """(F, 4, h) products -> (4 classes, 4, h): the frames of a chunk in order from +0, then the chunks in order from +0."""
    f, _, h = prod.shape
    chunk = chunk_frames(n_fft)
    total = np.zeros((4, 4, h), dtype=np.float64)
    with np.errstate(all="ignore"):
        for c0 in range(0, f, chunk):
            acc = np.zeros((4, 4, h), dtype=np.float64)
            for t in range(c0, min(c0 + chunk, f)):
                acc[cls[t]] = acc[cls[t]] + prod[t]
            total = total + acc
    return total


def all_frames(sums):
    with np.errstate(all="ignore"):
        return (sums[0] + sums[1]) + (sums[2] + sums[3])


def msc(s):
    """(4, h) sums Sxx, Syy, Sxy_re, Sxy_im -> g (h,)."""
    with np.errstate(all="ignore"):
        den = s[0] * s[1]
        ratio = (s[2] * s[2] + s[3] * s[3]) / den
        return np.where(den == 0.0, 0.0, np.where(ratio > 1.0, 1.0, ratio))


# ---- the band mapping -----------------------------------------------------------------------------------------------------------------------
def band_map(s, weights, importance):
    """(4, h) sums -> dict: N, D, T (bands,), the value, and the bounds of T and the value against another evaluation whose N and D have
    the same bits: log10 within LOG10_ULP ulps, the product with 10, the sum with 15, the quotient by 30; then per band the product with
    I_i and one rounding a partial sum, and the last quotient."""
    g = msc(s)
    nb = len(weights)
    imp = np.asarray(importance, dtype=np.float64)
    n, d = np.zeros(nb), np.zeros(nb)
    with np.errstate(all="ignore"):
        sig, dis = g * s[1], (1.0 - g) * s[1]
        for i, (lo, hi) in enumerate(runs(weights)):
            a, b = np.float64(0.0), np.float64(0.0)
            for k in range(lo, hi):
                a, b = a + weights[i, k] * sig[k], b + weights[i, k] * dis[k]
            n[i], d[i] = a, b
        db = 10.0 * np.log10(n / d)
        cl = np.where(db < -15.0, -15.0, np.where(db > 15.0, 15.0, db))
        t = (cl + 15.0) / 30.0
        fixed = (n == 0.0) | ((d == 0.0) & (n > 0.0))
        t = np.where(n == 0.0, 0.0, np.where((d == 0.0) & (n > 0.0), 1.0, t))
        # a clamped value moves by no more than the value before the clamp
        d_t = np.where(fixed, 0.0, SLACK * (((LOG10_ULP + 1.0) * U * np.abs(db) + U * np.abs(cl + 15.0)) / 30.0 + U * np.abs(t)))
        num, den = np.float64(0.0), np.float64(0.0)
        for i in range(nb):
            num, den = num + imp[i] * t[i], den + imp[i]
        value = num / den
        d_num = np.sum(imp * d_t) + (nb + 1) * U * np.sum(np.abs(imp * t))
        d_value = SLACK * (d_num / den + U * np.abs(value))
    return {"n": n, "d": d, "t": t, "value": value, "d_t": d_t, "d_value": d_value}


def index3(low, mid, d_low=0.0, d_mid=0.0):
    """I3, the intelligibility and their bounds from the low and mid values and theirs."""
    with np.errstate(all="ignore"):
        a, b = 1.84 * low, 9.99 * mid
        first = -3.47 + a
        i3 = first + b
        e = np.exp(-i3)
        s = 1.0 + e
        r = 1.0 / s
        d_i3 = SLACK * (1.84 * d_low + 9.99 * d_mid + U * (abs(a) + abs(b) + abs(first) + abs(i3)))
        d_e = SLACK * (e * d_i3 + EXP_ULP * U * e)
        d_r = SLACK * ((d_e + U * s) / (s * s) + U * r)
    return i3, r, d_i3, d_r


# ---- a pair -----------------------------------------------------------------------------------------------------------------------------------
def pair(ref, est, n, hop, n_fft, tw, weights=None, importance=None, kind="hann"):
    """One pair of fp32 clips of equal length -> dict of everything the library reports for it."""
    a, b = spectrum(ref, n, hop, n_fft, tw, kind), spectrum(est, n, hop, n_fft, tw, kind)
    e, cls, counts = classify(a["xw"])
    f, h = len(e), n_fft // 2
    sums = class_sums(products(a, b), cls, n_fft) if f else np.zeros((4, 4, h))
    rows = [sums[0], sums[1], sums[2], sums[3], all_frames(sums)]
    row_frames = list(counts) + [f]
    nan_if = lambda count, v: v if count >= 2 else np.full_like(v, np.nan)
    out = {"frames": f, "level_frames": counts, "frame_class": cls, "frame_energy": e, "sums": sums,
           "msc": nan_if(f, msc(rows[4])), "msc_levels": np.stack([nan_if(row_frames[c], msc(rows[c])) for c in range(4)])}
    if weights is None:
        return out
    maps = [band_map(rows[r], weights, importance) for r in (0, 1, 2, 4)]  # high, mid, low, all frames
    counts4 = [row_frames[r] for r in (0, 1, 2, 4)]
    value = [m["value"] if c >= 2 else np.nan for m, c in zip(maps, counts4)]
    bound = [m["d_value"] if c >= 2 else 0.0 for m, c in zip(maps, counts4)]
    i3, intel, d_i3, d_intel = index3(value[2], value[1], bound[2], bound[1])
    out.update(band_signal=np.stack([m["n"] for m in maps]), band_distortion=np.stack([m["d"] for m in maps]),
               band_value=np.stack([m["t"] for m in maps]), band_value_bound=np.stack([m["d_t"] for m in maps]),
               csii_high=value[0], csii_mid=value[1], csii_low=value[2], csii=value[3], i3=i3, intelligibility=intel,
               bounds={"csii_high": bound[0], "csii_mid": bound[1], "csii_low": bound[2], "csii": bound[3], "i3": d_i3 if np.isfinite(i3) else 0.0,
                       "intelligibility": d_intel if np.isfinite(i3) else 0.0})
    return out


# ---- the plain restatement ------------------------------------------------------------------------------------------------------------------
def plain_csii(ref, est, n, hop, n_fft, weights, importance, kind="hann"):
    """CSII from ``numpy.fft`` and ``numpy.sum``: no stated order anywhere.  -> {"csii", "csii_high", "csii_mid", "csii_low", "i3",
    "intelligibility", "level_frames"}."""
    w = window(n, kind)
    x, y = frames_xw(ref, w, n, hop), frames_xw(est, w, n, hop)
    h = n_fft // 2
    fx, fy = np.fft.fft(x, n_fft, axis=1)[:, :h], np.fft.fft(y, n_fft, axis=1)[:, :h]
    e = np.sum(x * x, axis=1)
    mean = e.mean()
    cls = np.where(e >= mean, 0, np.where(e >= 0.1 * mean, 1, np.where(e >= 0.001 * mean, 2, 3)))
    imp = np.asarray(importance, dtype=np.float64)
    out = {"level_frames": np.bincount(cls, minlength=4)}
    for name, pick in (("csii_high", cls == 0), ("csii_mid", cls == 1), ("csii_low", cls == 2), ("csii", cls >= 0)):
        if pick.sum() < 2:
            out[name] = np.nan
            continue
        sxx, syy = np.sum(np.abs(fx[pick]) ** 2, axis=0), np.sum(np.abs(fy[pick]) ** 2, axis=0)
        sxy = np.sum(fx[pick] * np.conj(fy[pick]), axis=0)
        with np.errstate(all="ignore"):
            g = np.where(sxx * syy == 0.0, 0.0, np.minimum(np.abs(sxy) ** 2 / (sxx * syy), 1.0))
            sig, dis = weights @ (g * syy), weights @ ((1.0 - g) * syy)
            t = (np.clip(10.0 * np.log10(sig / dis), -15.0, 15.0) + 15.0) / 30.0
            t = np.where(sig == 0.0, 0.0, np.where((dis == 0.0) & (sig > 0.0), 1.0, t))
        out[name] = float(np.sum(imp * t) / np.sum(imp))
    out["i3"] = -3.47 + 1.84 * out["csii_low"] + 9.99 * out["csii_mid"]
    out["intelligibility"] = 1.0 / (1.0 + np.exp(-out["i3"]))
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def envelope(samples, period=4000):
    """0.02 + 0.98 (0.5 - 0.5 cos(2 pi n / period))^2: a level that sweeps 34 dB, so that every level class occurs."""
    i = np.arange(samples, dtype=np.float64)
    return 0.02 + 0.98 * (0.5 - 0.5 * np.cos(2.0 * np.pi * i / period)) ** 2
