"""The fp64 oracle of the critical-band measures in NumPy: the radix-2 network on the library's twiddle table, the
band sums, the peak walks and the three measures in the stated orders, with the error bounds of what lies behind a ``log10`` or a ``pow``;
and the long-double designs of the two host tables.  Tests only; no GPU import here."""
import numpy as np

from tests.lpc_ref import U, clamp, frames_xw, lane_sum, mean_bound, n_frames, ordered_mean, trim_count, trimmed_mean, window  # noqa: F401

FLOOR = 1e-10
ERR_FLOOR = 2.0 ** -52
# What the device's and NumPy's log10 and pow may each be off by, in ulps of the result (HIP's and glibc's documentation state 1 ulp for
# both functions in double precision; nobody has measured gfx950): a device value and an oracle value differ by up to their sum.
LOG10_ULP = 1.0 + 1.0
POW_ULP = 1.0 + 1.0
SLACK = 1.01  # the terms of second order in U that the first-order propagation below leaves out

CENTRES = (50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70,
           1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63)
WIDTHS = (70.0,) * 7 + (77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255,
                        276.072, 298.126, 321.465, 346.136)


def default_fft(n):
    n_fft = 16
    while n_fft < 2 * n:
        n_fft *= 2
    return n_fft


# ---- the long-double designs of the host tables ---------------------------------------------------------------------------------------------
def twiddle_design(n_fft):
    """(n_fft / 2, 2) long double: (cos, -sin) of 2 pi m / n_fft, the angle taken straight (no mirroring)."""
    pi = 4.0 * np.arctan(np.longdouble(1.0))
    a = 2.0 * pi * np.arange(n_fft // 2, dtype=np.longdouble) / np.longdouble(n_fft)
    return np.stack([np.cos(a), -np.sin(a)], axis=1)


def weights_design(fs, n_fft, centres=CENTRES, widths=WIDTHS):
    """(bands, n_fft / 2) long double, thresholded."""
    h = n_fft // 2
    nyquist = fs / 2.0
    k = np.arange(h, dtype=np.longdouble)
    narrowest = np.longdouble(min(widths))
    rows = []
    for c, w in zip(centres, widths):
        f0, bw = np.float64(c) / nyquist * h, np.float64(w) / nyquist * h
        x = (k - np.longdouble(np.floor(f0))) / np.longdouble(bw)
        v = np.exp(np.longdouble(-11.0) * (x * x) + np.log(narrowest) - np.log(np.longdouble(w)))
        v[v <= np.exp(np.longdouble(-30.0) / (np.longdouble(2.0) * np.longdouble("2.303")))] = 0.0
        rows.append(v)
    return np.stack(rows)


# ---- the transform --------------------------------------------------------------------------------------------------------------------------
def bit_reverse(n_fft):
    bits = n_fft.bit_length() - 1
    idx = np.arange(n_fft)
    rev = np.zeros(n_fft, dtype=np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    return rev


def fft(xw, n_fft, tw):
    """(F, N) fp64 frames -> (re, im), (F, n_fft) fp64 each: the radix-2 decimation-in-time network of section 3.22 on the twiddle table
    ``tw`` (n_fft / 2, 2).  Every product and every sum is one NumPy operation: rounded on its own."""
    f, n = xw.shape
    re = np.zeros((f, n_fft), dtype=np.float64)
    im = np.zeros((f, n_fft), dtype=np.float64)
    re[:, bit_reverse(n_fft)[:n]] = xw
    span = 2
    with np.errstate(all="ignore"):
        while span <= n_fft:
            hf = span // 2
            w = tw[np.arange(hf) * (n_fft // span)]
            wr, wi = w[:, 0][None, None, :], w[:, 1][None, None, :]
            r3, i3 = re.reshape(f, n_fft // span, span), im.reshape(f, n_fft // span, span)
            ar, ai, br, bi = r3[:, :, :hf], i3[:, :, :hf], r3[:, :, hf:], i3[:, :, hf:]
            tr = wr * br - wi * bi
            ti = wr * bi + wi * br
            re = np.concatenate([ar + tr, ar - tr], axis=2).reshape(f, n_fft)
            im = np.concatenate([ai + ti, ai - ti], axis=2).reshape(f, n_fft)
            span *= 2
    return re, im


def spectrum(x, n, hop, n_fft, tw, kind="hann"):
    """One clip -> dict: "re", "im", "power", "magnitude" (F, n_fft / 2) and "magnitude_sum" (F,)."""
    xw = frames_xw(x, window(n, kind), n, hop)
    h = n_fft // 2
    re, im = fft(xw, n_fft, tw)
    re, im = re[:, :h], im[:, :h]
    with np.errstate(all="ignore"):
        p = re * re + im * im
        a = np.sqrt(p)
        s = lane_sum(a) if len(a) else np.zeros(0)
    return {"re": re, "im": im, "power": p, "magnitude": a, "magnitude_sum": s, "xw": xw}


def runs(weights):
    """[(lo, hi)]: band i's non-zero weights are [lo, hi)."""
    out = []
    for row in weights:
        nz = np.nonzero(row)[0]
        out.append((int(nz[0]), int(nz[-1]) + 1))
    return out


def band_sum(values, weights):
    """(F, h) values -> (F, bands): one chain over the band's run of non-zero weights in increasing k from +0."""
    f = values.shape[0]
    out = np.zeros((f, len(weights)), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i, (lo, hi) in enumerate(runs(weights)):
            acc = np.zeros(f, dtype=np.float64)
            for k in range(lo, hi):
                acc = acc + weights[i, k] * values[:, k]
            out[:, i] = acc
    return out


# ---- the peak walk ----------------------------------------------------------------------------------------------------------------------------
def peak_walk(e_lin):
    """(bands,) band energies -> (peak band of i = 0 .. bands - 2, the first band of the largest energy).  Decided on the energies."""
    nb = len(e_lin)
    rising = lambda m: bool(e_lin[m + 1] > e_lin[m])
    peaks = np.zeros(nb - 1, dtype=np.int32)
    for i in range(nb - 1):
        m = i
        if rising(i):
            while m <= nb - 2 and rising(m):
                m += 1
            peaks[i] = m
        else:
            while m >= 0 and not rising(m):
                m -= 1
            peaks[i] = m + 1
    am = 0
    for i in range(1, nb):
        if e_lin[i] > e_lin[am]:
            am = i
    return peaks, am


# ---- the measures -----------------------------------------------------------------------------------------------------------------------------
def wss_side(band_p):
    """(F, bands) band sums of P -> dict of the side's e (dB), slopes, weights, peaks, argmax and the bounds of e, slope and weight."""
    f, nb = band_p.shape
    with np.errstate(all="ignore"):
        e_lin = np.where(band_p > FLOOR, band_p, FLOOR)
        e = 10.0 * np.log10(e_lin)
    d_e = (LOG10_ULP + 1.0) * U * np.abs(e)  # the logarithm, and the product with 10 on each side
    peaks = np.zeros((f, nb - 1), dtype=np.int32)
    am = np.zeros(f, dtype=np.int32)
    for t in range(f):
        peaks[t], am[t] = peak_walk(e_lin[t])
    rows = np.arange(f)
    e_i, d_i = e[:, :-1], d_e[:, :-1]
    e_max, d_max = e[rows, am][:, None], d_e[rows, am][:, None]
    e_pk, d_pk = np.take_along_axis(e, peaks.astype(np.int64), axis=1), np.take_along_axis(d_e, peaks.astype(np.int64), axis=1)
    with np.errstate(all="ignore"):
        den1 = (20.0 + e_max) - e_i
        den2 = (1.0 + e_pk) - e_i
        a, b = 20.0 / den1, 1.0 / den2
        w = a * b
        slope = e[:, 1:] - e_i
        d_den1 = d_max + d_i + U * (np.abs(20.0 + e_max) + np.abs(den1))
        d_den2 = d_pk + d_i + U * (np.abs(1.0 + e_pk) + np.abs(den2))
        d_w = np.abs(w) * (d_den1 / np.abs(den1) + d_den2 / np.abs(den2) + 3.0 * U)  # two quotients and a product
        d_slope = d_e[:, 1:] + d_i + U * np.abs(slope)
    return {"e": e, "slope": slope, "w": w, "peaks": peaks, "argmax": am, "d_w": d_w, "d_slope": d_slope}


def frame_values(ref, est, weights, gamma=0.2, normalize=True):
    """The frames' band sums, decisions, values and bounds from ``spectrum`` of each side."""
    nb, h = weights.shape
    f = ref["power"].shape[0]
    out = {"magnitude_sum": np.stack([ref["magnitude_sum"], est["magnitude_sum"]], axis=1)}
    with np.errstate(all="ignore"):
        m = [band_sum(s["magnitude"] / s["magnitude_sum"][:, None] if normalize else s["magnitude"], weights) for s in (ref, est)]
        e = [band_sum(s["power"], weights) for s in (ref, est)]
        out["band_magnitude"], out["band_power"] = np.stack(m, axis=1), np.stack(e, axis=1)
        counted = (ref["magnitude_sum"] > 0.0) & (est["magnitude_sum"] > 0.0)
        # fwSegSNR
        d = m[0] - m[1]
        dd = d * d
        err = np.where(dd > ERR_FLOOR, dd, ERR_FLOOR)
        w = np.power(m[0], gamma)
        snr = 10.0 * np.log10((m[0] * m[0]) / err)
        t = w * snr
        num, den = np.zeros(f), np.zeros(f)
        for i in range(nb):
            num, den = num + t[:, i], den + w[:, i]
        ratio = num / den
        fw = np.where(counted, clamp(ratio, -10.0, 35.0), np.nan)
        # a term: pow, the logarithm, the product with 10, the product of the two; then the sums' roundings, band by band
        d_t = (POW_ULP + LOG10_ULP + 2.0) * U * np.abs(t)
        d_num = d_t.sum(axis=1) + nb * U * np.abs(t).sum(axis=1)
        d_den = (POW_ULP + nb) * U * den
        b_fw = SLACK * (d_num / den + np.abs(num) * d_den / (den * den) + U * np.abs(ratio))
        # WSS
        sides = [wss_side(e[0]), wss_side(e[1])]
        ww = (sides[0]["w"] + sides[1]["w"]) / 2.0
        sd = sides[0]["slope"] - sides[1]["slope"]
        sdd = sd * sd
        term = ww * sdd
        w_num, w_den = np.zeros(f), np.zeros(f)
        for i in range(nb - 1):
            w_num, w_den = w_num + term[:, i], w_den + ww[:, i]
        wss = w_num / w_den
        d_ww = (sides[0]["d_w"] + sides[1]["d_w"]) / 2.0 + U * np.abs(ww)
        d_sd = sides[0]["d_slope"] + sides[1]["d_slope"] + U * np.abs(sd)
        d_sdd = 2.0 * np.abs(sd) * d_sd + d_sd * d_sd + U * sdd
        d_term = d_ww * sdd + np.abs(ww) * d_sdd + d_ww * d_sdd + U * np.abs(term)
        d_wnum = d_term.sum(axis=1) + nb * U * np.abs(term).sum(axis=1)
        d_wden = d_ww.sum(axis=1) + nb * U * np.abs(ww).sum(axis=1)
        b_wss = SLACK * (d_wnum / np.abs(w_den) + np.abs(w_num) * d_wden / (w_den * w_den) + U * np.abs(wss))
        # LSD
        lr = 10.0 * np.log10(np.where(ref["power"] > FLOOR, ref["power"], FLOOR))
        le = 10.0 * np.log10(np.where(est["power"] > FLOOR, est["power"], FLOOR))
        ld = lr - le
        ldd = ld * ld
        total = lane_sum(ldd) if f else np.zeros(0)
        q = total / h
        lsd = np.sqrt(q)
        d_ld = (LOG10_ULP + 1.0) * U * (np.abs(lr) + np.abs(le)) + U * np.abs(ld)
        d_ldd = 2.0 * np.abs(ld) * d_ld + d_ld * d_ld + U * ldd
        d_q = (d_ldd.sum(axis=1) + (-(-h // 64) + 7) * U * total) / h
        b_lsd = SLACK * (np.where(q > 4.0 * d_q, 0.6 * d_q / np.where(q > 0, np.sqrt(q), 1.0), np.sqrt(d_q)) + U * lsd)
    out.update(counted=counted, fw=fw, wss=wss, lsd=lsd, peaks=np.stack([sides[0]["peaks"], sides[1]["peaks"]], axis=1),
               argmax=np.stack([sides[0]["argmax"], sides[1]["argmax"]], axis=1),
               bounds={"fw": np.where(counted, b_fw, 0.0), "wss": b_wss, "lsd": b_lsd})
    return out


def pair_values(fv, trim=0.95):
    """The pair's three values and two counts from ``frame_values``' result."""
    counted = fv["counted"]
    frames = len(counted)
    k = trim_count(trim, frames)
    b = fv["bounds"]
    order = np.argsort(fv["wss"], kind="stable")
    return {"fw_seg_snr_db": ordered_mean(fv["fw"][counted]), "wss": trimmed_mean(fv["wss"], trim), "lsd_db": ordered_mean(fv["lsd"]),
            "frames": frames, "snr_frames": int(counted.sum()),
            "bounds": {"fw_seg_snr_db": mean_bound(fv["fw"][counted], b["fw"][counted], int(counted.sum())),
                       "wss": mean_bound(fv["wss"][order][:max(k, 1)] if frames else fv["wss"], b["wss"], k),
                       "lsd_db": mean_bound(fv["lsd"], b["lsd"], frames)}}


def metrics(ref, est, n, hop, n_fft, tw, weights, kind="hann", gamma=0.2, normalize=True, trim=0.95):
    """One pair of fp32 clips of equal length -> (pair values, frame values)."""
    fv = frame_values(spectrum(ref, n, hop, n_fft, tw, kind), spectrum(est, n, hop, n_fft, tw, kind), weights, gamma, normalize)
    return pair_values(fv, trim), fv
