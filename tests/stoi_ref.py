"""fp64 numpy oracle of the library's STOI / ESTOI (include/l3ac_hip.h, 'speech intelligibility').  Its inputs are
the fp32 samples and the library's own fp32 tables (the window and the window-folded basis), which are part of the spec; the tables'
fp64 designs and the band runs are restated here too, for the host test that compares them.  `restate32` is the same chain in numpy
float32 throughout, the yardstick of what fp32 arithmetic costs."""
import numpy as np

EPS = 2.0 ** -52
U32 = 2.0 ** -24
FRAME, HOP, N_FFT, BANDS, SEG = 256, 128, 512, 15, 30
RANGE_DB = 40.0
SENTINEL = 1e-5
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)


def frames(n):
    """A(n): analysis frames of a clip of n samples; frame f starts at 128 f < n - 256."""
    return 0 if n <= FRAME else -((FRAME - n) // HOP)


def window_design():
    """hanning(258)[1 + j], j = 0..255, in fp64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(FRAME) + 1.0) / 257.0)


def basis_design():
    """[514][256] fp64: row 2k = w cos(2 pi (jk mod 512) / 512), row 2k + 1 = -w sin(...)."""
    j = np.arange(FRAME, dtype=np.int64)
    k = np.arange(N_FFT // 2 + 1, dtype=np.int64)
    ang = 2.0 * np.pi / N_FFT * ((k[:, None] * j[None, :]) % N_FFT).astype(np.float64)
    out = np.empty((N_FFT + 2, FRAME))
    out[0::2] = window_design() * np.cos(ang)
    out[1::2] = -window_design() * np.sin(ang)
    return out


def band_runs():
    """[(lo, hi)] of the 15 third-octave bands: the bins nearest to 150 * 2^((2i -+ 1) / 6) Hz, bin k at k * 10000 / 512 Hz."""
    f = np.arange(N_FFT // 2 + 1) * 10000.0 / N_FFT
    return [(int(np.argmin((f - 150.0 * 2.0 ** ((2 * i - 1) / 6.0)) ** 2)), int(np.argmin((f - 150.0 * 2.0 ** ((2 * i + 1) / 6.0)) ** 2)))
            for i in range(BANDS)]


def frame_matrix(x, count):
    """[count][256]: frame f = x[128 f .. 128 f + 256)."""
    if count == 0:
        return np.zeros((0, FRAME), dtype=x.dtype)
    return np.stack([x[HOP * f:HOP * f + FRAME] for f in range(count)])


def keep_mask(ref, window, dtype=np.float64):
    """(mask [F] bool, margin): the frames whose level 20 log10(sqrt(e_f) + eps) is above the clip's maximum - 40, and the smallest
    distance in dB of any frame's level from that threshold (inf without frames)."""
    x = np.asarray(ref, dtype=dtype)
    count = frames(x.shape[0])
    if count == 0:
        return np.zeros(0, dtype=bool), np.inf
    fr = frame_matrix(x, count) * np.asarray(window, dtype=dtype)
    level = dtype(20.0) * np.log10(np.sqrt(np.sum(fr * fr, axis=1, dtype=dtype)) + dtype(EPS))
    threshold = level.max() - dtype(RANGE_DB)
    return level > threshold, float(np.min(np.abs(level - threshold)))


def overlap_add(x, window, mask, dtype=np.float64):
    """(s, sabs): the kept frames of x, windowed and added at hop 128 in the order of q; sabs = the sum of the terms' magnitudes."""
    x = np.asarray(x, dtype=dtype)
    w = np.asarray(window, dtype=dtype)
    kept = np.flatnonzero(mask)
    s = np.zeros(HOP * (len(kept) - 1) + FRAME if len(kept) else 0, dtype=dtype)
    sabs = np.zeros_like(s)
    for q, f in enumerate(kept):
        term = w * x[HOP * f:HOP * f + FRAME]
        s[HOP * q:HOP * q + FRAME] += term
        sabs[HOP * q:HOP * q + FRAME] += np.abs(term)
    return s, sabs


def spectra(s, basis):
    """([T][257] re, [T][257] im, frames [T][256]) of the rebuilt signal: the fp32 basis applied to s[128 t .. 128 t + 256), T = A(len(s))."""
    fr = frame_matrix(s, frames(s.shape[0]))
    out = fr @ np.asarray(basis, dtype=s.dtype).T
    return out[:, 0::2], out[:, 1::2], fr


def band_power(re, im, runs=None):
    p = re * re + im * im
    return np.stack([p[:, lo:hi].sum(axis=1) for lo, hi in (runs or band_runs())], axis=1) if p.shape[0] else np.zeros((0, BANDS), dtype=p.dtype)


def _row_normalise(v, eps):
    v = v - v.mean(axis=-1, keepdims=True)
    return v / (np.sqrt((v * v).sum(axis=-1, keepdims=True)) + eps)


def _ratio(v):
    """Smallest centred norm / norm over the non-zero rows (last axis) of v; inf when every row is zero."""
    n = np.sqrt((v * v).sum(axis=-1))
    c = v - v.mean(axis=-1, keepdims=True)
    nc = np.sqrt((c * c).sum(axis=-1))
    return float(np.min(nc[n > 0] / n[n > 0])) if (n > 0).any() else np.inf


def intelligibility(bx, by, dtype=np.float64):
    """Steps 5 and 6 on band cells [T][15] of the reference (bx) and the estimate (by): (stoi, estoi, conditioning).  conditioning = the
    smallest ratio of centred norm to norm over every non-zero segment row (STOI and ESTOI) and column (ESTOI)."""
    bx, by = np.asarray(bx, dtype=dtype), np.asarray(by, dtype=dtype)
    t = bx.shape[0]
    if t < SEG:
        return SENTINEL, SENTINEL, np.inf
    eps = dtype(EPS)
    d_stoi, d_estoi, cond = [], [], np.inf
    for m in range(SEG, t + 1):
        x, y = bx[m - SEG:m].T, by[m - SEG:m].T  # [15][30]: rows are bands
        c = np.sqrt((x * x).sum(axis=1, keepdims=True)) / (np.sqrt((y * y).sum(axis=1, keepdims=True)) + eps)
        yp = np.minimum(c * y, dtype(CLIP) * x)
        xn = _row_normalise(x, eps)
        d_stoi.append((xn * _row_normalise(yp, eps)).sum(dtype=dtype) / dtype(BANDS))
        yn = _row_normalise(y, eps)
        d_estoi.append((_row_normalise(xn.T, eps) * _row_normalise(yn.T, eps)).sum(dtype=dtype) / dtype(SEG))
        cond = min(cond, _ratio(x), _ratio(y), _ratio(yp), _ratio(xn.T), _ratio(yn.T))
    return float(np.mean(np.asarray(d_stoi, dtype=dtype), dtype=dtype)), float(np.mean(np.asarray(d_estoi, dtype=dtype), dtype=dtype)), cond


def oracle(ref, est, window, basis):
    """The whole spec in fp64 on the fp32 samples and tables, one clip pair.  Returns a dict: mask, margin, frames (T), bands_ref,
    bands_est ([T][15]), power_ref, power_est (band powers), dpower_ref, dpower_est (the a-priori bound on an fp32 evaluation's
    |bands^2 - power|, see `power_bound`), stoi, estoi, conditioning."""
    ref, est = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)  # (fp32 samples convert exactly)
    mask, margin = keep_mask(ref, window)
    out = {"mask": mask, "margin": margin, "frames": max(int(mask.sum()) - 1, 0)}
    for name, x in (("ref", ref), ("est", est)):
        s, sabs = overlap_add(x, window, mask)
        re, im, fr = spectra(s, basis)
        power = band_power(re, im)
        out["power_" + name], out["bands_" + name] = power, np.sqrt(power)
        out["dpower_" + name] = power_bound(re, im, fr, frame_matrix(sabs, fr.shape[0]), basis)
    out["stoi"], out["estoi"], out["conditioning"] = intelligibility(out["bands_ref"], out["bands_est"])
    return out


def power_bound(re, im, fr, fr_abs, basis):
    """The bound on |cell^2 - band power| of an evaluation in fp32: the overlap-add's two products and one add (each sample off by at
    most 2 u (|t0| + |t1|)), the fp32 dot product of 256 terms ((256 + 2) u sum |b_j s_j| per part, plus the samples' own error through
    |b_j|), re^2 + im^2 as fma(re, re, im im) (3 u), the band's sum of n terms ((n + 2) u), and the square root's rounding (u on the
    value, 2 u + u^2 on its square)."""
    b = np.abs(np.asarray(basis, dtype=np.float64))
    ds = 2.0 * U32 * fr_abs
    d = (FRAME + 2) * U32 * ((np.abs(fr) + ds) @ b.T) + ds @ b.T
    d_re, d_im = d[:, 0::2], d[:, 1::2]
    p = re * re + im * im
    dp = 2 * np.abs(re) * d_re + d_re ** 2 + 2 * np.abs(im) * d_im + d_im ** 2
    dp = dp + 3 * U32 * (p + dp)
    out = np.zeros((p.shape[0], BANDS))
    for i, (lo, hi) in enumerate(band_runs()):
        total, dtotal = p[:, lo:hi].sum(axis=1), dp[:, lo:hi].sum(axis=1)
        dsum = dtotal + (hi - lo + 2) * U32 * (total + dtotal)
        out[:, i] = dsum + (2 * U32 + U32 * U32) * (total + dsum)
    return out


def restate32(ref, est, window, basis):
    """(stoi, estoi, frames) of one pair with every step in numpy float32, the DFT as frames32 @ basis32.T."""
    f32 = np.float32
    ref, est = np.asarray(ref, dtype=f32), np.asarray(est, dtype=f32)
    mask, _ = keep_mask(ref, window, f32)
    cells = []
    for x in (ref, est):
        s, _ = overlap_add(x, window, mask, f32)
        re, im, _ = spectra(s, np.asarray(basis, dtype=f32))
        cells.append(np.sqrt(band_power(re, im)))
        assert cells[-1].dtype == f32
    st, es, _ = intelligibility(cells[0], cells[1], f32)
    return st, es, max(int(mask.sum()) - 1, 0)
