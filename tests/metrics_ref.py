"""fp64 numpy restatement of the library's quality metrics (include/l3ac_hip.h, 'quality metrics').  Its inputs
are the library's own fp32 tables (the window-folded DFT basis and the mel weights), which are part of the spec; the tables' fp64
designs are restated here too, for the host test that compares them."""
import numpy as np

EPS = 2.0 ** -24


def frames(n, hop):
    return 1 + n // hop


def basis_design(n_fft):
    """[n_fft + 2][n_fft] fp64: row 2k = w cos(2 pi (jk mod n_fft) / n_fft), row 2k + 1 = -w sin(...), w the periodic Hann."""
    j = np.arange(n_fft, dtype=np.int64)
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi / n_fft * j)
    ang = 2.0 * np.pi / n_fft * ((k[:, None] * j[None, :]) % n_fft).astype(np.float64)
    out = np.empty((n_fft + 2, n_fft))
    out[0::2] = w * np.cos(ang)
    out[1::2] = -w * np.sin(ang)
    return out


def mel_design(sample_rate, n_fft, n_mels):
    """[n_mels][n_fft/2 + 1] fp64: HTK scale, n_mels + 2 points equally spaced in mel from 0 to sample_rate / 2, triangles, no normalisation."""
    mel_max = 2595.0 * np.log10(1.0 + 0.5 * sample_rate / 700.0)
    p = 700.0 * (10.0 ** ((mel_max * np.arange(n_mels + 2) / (n_mels + 1)) / 2595.0) - 1.0)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sample_rate / n_fft
    up = (f[None, :] - p[:-2, None]) / (p[1:-1, None] - p[:-2, None])
    down = (p[2:, None] - f[None, :]) / (p[2:, None] - p[1:-1, None])
    return np.maximum(0.0, np.minimum(up, down))


def frame_matrix(x, n_fft, hop):
    """[F(n)][n_fft] fp64: frame f = samples [f hop - n_fft/2, f hop + n_fft/2) of x, zeros outside."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    pad = np.concatenate([np.zeros(n_fft // 2), x, np.zeros(n_fft)])
    return np.stack([pad[f * hop:f * hop + n_fft] for f in range(frames(n, hop))])


def stft_ref(x, n_fft, hop, basis):
    """(X complex128 [F][n_fft/2 + 1], absdot [F][n_fft/2 + 1][2]): the spectrum on the fp32 `basis`, and sum_j |basis x| per real and imaginary part
    (the scale of the a-priori bound of an fp32 dot product)."""
    fr = frame_matrix(x, n_fft, hop)
    b = np.asarray(basis, dtype=np.float64)
    out = fr @ b.T
    absdot = np.abs(fr) @ np.abs(b).T
    return out[:, 0::2] + 1j * out[:, 1::2], np.stack([absdot[:, 0::2], absdot[:, 1::2]], axis=-1)


def stft_explicit(x, n_fft, hop):
    """The definition, without any table: X[f][k] = sum_j w[j] x_f[j] exp(-2 pi i j k / n_fft) in fp64."""
    fr = frame_matrix(x, n_fft, hop)
    j = np.arange(n_fft)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / n_fft)
    k = np.arange(n_fft // 2 + 1)
    e = np.exp(-2j * np.pi * ((j[:, None] * k[None, :]) % n_fft) / n_fft)
    return (fr * w) @ e


def log_mel_ref(spec, weights):
    """(L [F][n_mels], M [F][n_mels]) from a complex spectrum and the fp32 weights, in fp64."""
    p = spec.real ** 2 + spec.imag ** 2
    m = p @ np.asarray(weights, dtype=np.float64).T
    return np.log10(np.maximum(m, 1e-10)), m


def log_mel_bound(spec, d_re, d_im, weights):
    """The bound on |L_fp32 - L| propagated from the per-part STFT bounds d_re, d_im: (dL, excluded), excluded = cells with M - dM <= 1e-10."""
    w = np.asarray(weights, dtype=np.float64)
    re, im = np.abs(spec.real), np.abs(spec.imag)
    p = re ** 2 + im ** 2
    dp = 2 * re * d_re + d_re ** 2 + 2 * im * d_im + d_im ** 2 + 3 * EPS * p
    m = p @ w.T
    nz = int((w != 0).sum(axis=1).max())
    dm = dp @ w.T + (nz + 2) * EPS * m
    excluded = m - dm <= 1e-10
    lo = np.where(excluded, 1.0, m - dm)
    l = np.log10(np.maximum(m, 1e-10))
    return np.log10(m + dm + (m + dm == 0)) - np.log10(lo) + 8 * EPS * np.abs(l), excluded


def signal_metrics_ref(r, e):
    """(mse, snr_db, si_sdr_db) of one pair in fp64; residuals taken directly; IEEE division."""
    r = np.asarray(r, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    n = r.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sum((r - e) ** 2)
        mse = d / n
        snr = 10.0 * np.log10(np.float64(np.sum(r * r)) / d)
        rc, ec = r - r.mean(), e - e.mean()
        alpha = np.float64(np.sum(rc * ec)) / np.float64(np.sum(rc * rc))
        si = 10.0 * np.log10(alpha * alpha * np.sum(rc * rc) / np.sum((ec - alpha * rc) ** 2))
    return float(mse), float(snr), float(si)
