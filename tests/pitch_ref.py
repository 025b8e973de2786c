"""The fp64 oracle of the pitch tracker and the F0 metrics, in NumPy, written from the specification alone: the
difference function summed in fp64 in the direct form, the cumulative-mean-normalised difference, the pick, the parabolic refinement;
`pick_from_cmnd`, the pick and the refinement restated on a given row; `robust`, whether every comparison the pick makes on a row has a
margin over what the fp32 difference function may cost; the pair metrics; and the suite's inputs."""
import math

import numpy as np

U32 = 2.0 ** -24  # fp32 unit roundoff
U64 = 2.0 ** -53


def lags(fs, fmin=60.0, fmax=500.0, hop=None, window=None):
    """The geometry -> dict(fs, tau_min, tau_max, T, W, hop, span)."""
    tau_min, tau_max = math.floor(fs / fmax), math.ceil(fs / fmin)
    w = tau_max if window is None else int(window)
    return dict(fs=fs, tau_min=tau_min, tau_max=tau_max, T=tau_max + 1, W=w, hop=fs // 100 if hop is None else int(hop), span=w + tau_max + 1)


def frames(n, g):
    return 0 if n < g["span"] else 1 + (n - g["span"]) // g["hop"]


def nominal_time(t, g):
    return (t * g["hop"] + g["span"] / 2) / g["fs"]


def gamma(g):
    """|d_fp32 - d| <= gamma d for any order of the sum: a rounding of the difference, squared, and at most W roundings of the sum."""
    k = (g["W"] + 2) * U32
    return k / (1 - k)


def beta(g):
    """|c_library - c_oracle| <= beta c: 2 gamma / (1 - gamma) from the fp32 difference function (d and S each within gamma), plus the fp64
    roundings of both sides (W terms of the oracle's d, T of each prefix, the product and the quotient)."""
    gm = gamma(g)
    return 2 * gm / (1 - gm) + 4 * (g["W"] + g["T"] + 8) * U64


def difference(x, g):
    """(F, T + 1) fp64: d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2 of every frame."""
    x = np.asarray(x, dtype=np.float64)
    n_frames, w, t = frames(len(x), g), g["W"], g["T"]
    d = np.zeros((n_frames, t + 1))
    for f in range(n_frames):
        seg = x[f * g["hop"]:f * g["hop"] + g["span"]]
        shifted = np.lib.stride_tricks.sliding_window_view(seg, w)[:t + 1]  # row tau = seg[tau : tau + W]
        d[f] = ((seg[None, :w] - shifted) ** 2).sum(axis=1)
    return d


def cmnd(d):
    """c(0) = 1; c(tau) = d(tau) tau / S(tau), S the running sum of d(1 ..), and exactly 1 where S(tau) = 0."""
    d = np.atleast_2d(d)
    s = np.cumsum(d[:, 1:], axis=1)
    tau = np.arange(1, d.shape[1], dtype=np.float64)
    c = np.ones_like(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        c[:, 1:] = np.where(s == 0.0, 1.0, d[:, 1:] * tau / s)
    return c


def pick_from_cmnd(c, g, threshold=0.1):
    """One row c[0 .. T] -> (tau*, voiced, f0, aperiodicity): the specification's pick and refinement, in the library's order of operations."""
    tau_min, tau_max = g["tau_min"], g["tau_max"]
    c = [float(v) for v in c]
    star, voiced = None, 0
    for tau in range(tau_min, tau_max + 1):
        if c[tau] < threshold:
            star, voiced = tau, 1
            break
    if voiced:
        while star + 1 <= tau_max and c[star + 1] < c[star]:
            star += 1
    else:
        star = tau_min
        for tau in range(tau_min, tau_max + 1):
            if c[tau] < c[star]:
                star = tau
    a, b, e = c[star - 1], c[star], c[star + 1]
    den = a - 2.0 * b + e
    shift = 0.0
    if den > 0.0:
        sh = 0.5 * (a - e) / den
        if abs(sh) <= 1.0:
            shift = sh
    return star, voiced, g["fs"] / (star + shift), b


def robust(c, d, bt, g, threshold=0.1):
    """Whether every comparison the pick makes on the oracle's row c (from the difference row d) keeps its outcome under a relative error
    of `bt` in every entry.  Entries with S(tau) = 0 are exact ones on both sides.  For an unvoiced frame only the threshold comparisons
    count: which of its near-equal minima is the argmin is pinned against the library's own row instead."""
    tau_min, tau_max = g["tau_min"], g["tau_max"]
    exact = np.concatenate(([True], np.cumsum(d[1:]) == 0.0))
    err = np.where(exact, 0.0, bt * np.abs(c))

    def below_threshold_is_safe(tau):
        return abs(c[tau] - threshold) > err[tau]

    def descent_is_safe(tau):  # c(tau + 1) < c(tau)
        return (exact[tau] and exact[tau + 1]) or abs(c[tau + 1] - c[tau]) > err[tau + 1] + err[tau]

    star, voiced, _, _ = pick_from_cmnd(c, g, threshold)
    if not voiced:
        return all(below_threshold_is_safe(tau) for tau in range(tau_min, tau_max + 1))
    first = next(tau for tau in range(tau_min, tau_max + 1) if c[tau] < threshold)
    if not all(below_threshold_is_safe(tau) for tau in range(tau_min, first + 1)):
        return False
    return all(descent_is_safe(tau) for tau in range(first, min(star, tau_max - 1) + 1))


def oracle(x, fs, fmin=60.0, fmax=500.0, threshold=0.1, hop=None, window=None):
    """One clip -> dict(g, d, cmnd, tau, voiced, f0, aperiodicity, robust), rows per frame."""
    g = lags(fs, fmin, fmax, hop, window)
    d = difference(x, g)
    c = cmnd(d) if len(d) else np.ones((0, g["T"] + 1))
    picks = [pick_from_cmnd(row, g, threshold) for row in c]
    bt = beta(g)
    return dict(g=g, d=d, cmnd=c, tau=np.array([p[0] for p in picks], dtype=np.int64), voiced=np.array([p[1] for p in picks], dtype=np.int32),
                f0=np.array([p[2] for p in picks], dtype=np.float64), aperiodicity=np.array([p[3] for p in picks], dtype=np.float64),
                robust=np.array([robust(cr, dr, bt, g, threshold) for cr, dr in zip(c, d)], dtype=bool))


def metrics(f0_ref, v_ref, f0_est, v_est, n_frames):
    """The pair metrics of one clip over its first n_frames frames -> dict, the counts as ints."""
    f0_ref, f0_est = np.asarray(f0_ref, dtype=np.float64)[:n_frames], np.asarray(f0_est, dtype=np.float64)[:n_frames]
    vr, ve = np.asarray(v_ref)[:n_frames] != 0, np.asarray(v_est)[:n_frames] != 0
    both = vr & ve
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = f0_est[both] / f0_ref[both]
        gross = int((np.abs(ratio - 1.0) > 0.2).sum())
        flips = int((vr != ve).sum())
        cents = 1200.0 * np.log2(ratio)
        n_both = int(both.sum())
        nan = float("nan")
        return dict(frames=int(n_frames), voiced_reference=int(vr.sum()), voiced_estimate=int(ve.sum()), voiced_both=n_both,
                    vde=flips / n_frames if n_frames else nan, gpe=gross / n_both if n_both else nan,
                    ffe=(flips + gross) / n_frames if n_frames else nan,
                    f0_rmse_cents=math.sqrt(float((cents * cents).sum()) / n_both) if n_both else nan)


def rmse_bound(n_both, log2_ulps=1.0):
    """Relative bound between two fp64 evaluations of f0_rmse_cents on the same tracks.  Per side and term: the
    ratio is one IEEE division on both sides alike; log2 within `log2_ulps` ulp, that is 2 log2_ulps U64 relative; the product by 1200
    and the square one rounding each, the square doubling what its argument carries: (4 log2_ulps + 3) U64.  n_both - 1 additions of
    non-negative terms in any order and the quotient: n_both U64 more.  The root halves that and adds its own rounding.  Two sides:
    k = n_both + 4 log2_ulps + 5 roundings in all, k U64 / (1 - k U64)."""
    k = (n_both + 4 * log2_ulps + 5) * U64
    return k / (1 - k)


# ---- the suite's inputs ------------------------------------------------------------------------------------------------------------------------
GLIDE_F0, GLIDE_OCTAVES = 110.0, 1.5


def glide_f0(t, scale=1.0):
    return scale * GLIDE_F0 * 2.0 ** (GLIDE_OCTAVES * t)


def glide(n, fs, rng, scale=1.0):
    """Six harmonics of f0 = scale 110 2^(1.5 t), harmonic k at amplitude 0.7^k and phase offset k, peak-normalised to 0.5, plus noise 30 dB
    below half scale."""
    t = np.arange(n) / fs
    phase = 2 * np.pi * scale * GLIDE_F0 * (2.0 ** (GLIDE_OCTAVES * t) - 1.0) / (GLIDE_OCTAVES * math.log(2.0))
    x = sum(0.7 ** k * np.sin(k * phase + k) for k in range(1, 7))
    return 0.5 * x / np.max(np.abs(x)) + 0.5 * 10.0 ** (-30.0 / 20.0) * rng.standard_normal(n)


def clip(fs, seed, scale=1.0):
    """2 s: the glide, white noise at 0.1, digital silence, two tones (220.5 Hz and its octave) with noise at -40 dB; fp32."""
    rng = np.random.default_rng(seed)
    n = fs // 2
    t = np.arange(n) / fs
    tones = 0.25 * np.sin(2 * np.pi * 220.5 * t) + 0.125 * np.sin(2 * np.pi * 441.0 * t + 1.0) + 0.01 * rng.standard_normal(n)
    return np.concatenate((glide(n, fs, rng, scale), 0.1 * rng.standard_normal(n), np.zeros(n), tones)).astype(np.float32)
