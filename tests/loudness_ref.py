"""The fp64 oracle of DESIGN.md section 3.14 (BS.1770-4 integrated loudness of mono clips, and the gain), written from the spec alone:
the K-weighting coefficients by De Man's closed forms in numpy fp64, the filter as ``scipy.signal.sosfilt`` on fp64, the block and gate
arithmetic as the spec writes it.  A second filter in ``np.longdouble`` (a plain Python loop, transposed direct form II) supplies the
yardstick E of a case: the worst relative difference between the two filters' step energies, i.e. what fp64 itself costs there."""
import numpy as np
from scipy.signal import sosfilt

assert np.finfo(np.longdouble).nmant >= 63, "tests/loudness_ref.py needs an extended-precision np.longdouble (x87: 63 mantissa bits)"

MIN_RATE, MAX_RATE = 8000, 192000
ABS_GATE = -70.0
# the table ITU-R BS.1770-4 prints for 48 kHz: b0 b1 b2 a0 a1 a2 of the two stages
TABLE_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                      [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])


def supported(fs: int) -> bool:
    return fs % 10 == 0 and MIN_RATE <= fs <= MAX_RATE


def coeffs(fs: int) -> np.ndarray:
    """(2, 6) fp64: b0 b1 b2 a0 a1 a2 of the shelf and of the high-pass at the rate fs."""
    assert supported(fs)
    f0, g, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = np.tan(np.pi * f0 / fs)
    vh = 10.0 ** (g / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / q + k * k
    shelf = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0, 1.0, 2.0 * (k * k - 1.0) / a0,
             (1.0 - k / q + k * k) / a0]
    f0, q = 38.13547087602444, 0.5003270373238773
    k = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + k / q + k * k
    high = [1.0, -2.0, 1.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]
    return np.array([shelf, high], dtype=np.float64)


def blocks(n: int, fs: int) -> int:
    return max(n // (fs // 10) - 3, 0)


def _tdf2(sos, x, state, dtype):
    """The cascade over x from `state` (s1, s2 of stage 1, s1, s2 of stage 2), one sample at a time in `dtype` -> (y, end state)."""
    c = [[dtype(v) for v in row] for row in sos]
    s = [dtype(v) for v in state]
    y = np.empty(len(x), dtype=dtype)
    for i, v in enumerate(x):
        v = dtype(v)
        for k, (b0, b1, b2, _, a1, a2) in enumerate(c):
            out = b0 * v + s[2 * k]
            s[2 * k] = b1 * v - a1 * out + s[2 * k + 1]
            s[2 * k + 1] = b2 * v - a2 * out
            v = out
        y[i] = v
    return y, np.array(s, dtype=dtype)


def state_matrix(sos, step: int) -> np.ndarray:
    """M (4, 4): column k is the cascade's state after `step` zero-input samples from the unit state e_k."""
    m = np.empty((4, 4))
    zeros = np.zeros(step)
    for k in range(4):
        m[:, k] = _tdf2(sos, zeros, np.eye(4)[k], np.float64)[1]
    return m


def step_energies(y, step: int):
    """e_s = sum of y^2 over each whole step, summed in the order of the samples, in y's own precision."""
    s = len(y) // step
    e = np.zeros(s, dtype=y.dtype)
    sq = (y[:s * step] * y[:s * step]).reshape(s, step)
    for j in range(step):
        e = e + sq[:, j]
    return e


def energies64(x, fs: int) -> np.ndarray:
    return step_energies(sosfilt(coeffs(fs), np.asarray(x, dtype=np.float64)), fs // 10)


def energies_long(x, fs: int) -> np.ndarray:
    y, _ = _tdf2(coeffs(fs), np.asarray(x, dtype=np.float64), np.zeros(4), np.longdouble)
    return step_energies(y, fs // 10)


def yardstick(x, fs: int) -> float:
    """E: the worst relative difference of the fp64 filter's step energies from the long-double filter's (steps of exactly zero energy in
    both are left out)."""
    e64, el = energies64(x, fs).astype(np.longdouble), energies_long(x, fs)
    keep = (el != 0) & (e64 != 0)
    return float(np.max(np.abs(e64[keep] - el[keep]) / el[keep])) if keep.any() else 0.0


def lkfs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(np.asarray(z, dtype=np.float64))


def oracle(x, fs: int) -> dict:
    """Everything the library returns for one clip, and the margins of its blocks from the two gates (inf where no block is near one)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1 and supported(fs)
    step = fs // 10
    e = energies64(x, fs)
    j_count = blocks(len(x), fs)
    z = np.array([(((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / (4.0 * step) for j in range(j_count)], dtype=np.float64)
    l = lkfs(z) if j_count else np.zeros(0)
    absolute = l > ABS_GATE
    out = {"energies": e, "z": z, "momentary": l, "blocks": j_count, "peak": float(np.max(np.abs(x)).astype(np.float64)),
           "abs_margin": float(np.min(np.abs(l - ABS_GATE))) if j_count else np.inf, "rel_margin": np.inf, "gamma": None}
    passing = np.zeros(j_count, dtype=bool)
    if absolute.any():
        gamma = float(lkfs(np.sum(z[absolute]) / absolute.sum())) - 10.0
        passing = absolute & (l > gamma)
        out["gamma"] = gamma
        out["rel_margin"] = float(np.min(np.abs(l[absolute] - gamma)))
    out["gated"] = int(passing.sum())
    out["lufs"] = float(lkfs(np.sum(z[passing]) / passing.sum())) if passing.any() else -np.inf
    return out


def gain_db(lufs: float, peak: float, target: float, peak_limit_db=None) -> float:
    if lufs == -np.inf:
        return 0.0
    g = target - lufs
    if peak_limit_db is not None and peak > 0:
        g = min(g, peak_limit_db - 20.0 * np.log10(peak))
    return float(g)
