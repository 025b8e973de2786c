"""The fp64 oracle of DESIGN.md section 3.25 (EBU R128: block loudness series, EBU Tech 3342 loudness range, true peak), written from the
specs on top of the loudness oracle's step energies (tests/loudness_ref.py) and the sample-rate conversion oracle (tests/resample_ref.py),
both imported unchanged.  The gates report their margins as ``loudness_ref.oracle`` does."""
import numpy as np

from tests import loudness_ref as L
from tests import resample_ref as RS

SHORT_STEPS = 30  # 3 s
MAX_BLOCKS = 16384


def factor(fs: int) -> int:
    """The oversampling factor of the true-peak meter."""
    if 8000 <= fs < 96000:
        return 4
    if 96000 <= fs <= 192000:
        return 2
    raise ValueError(f"sample_rate {fs} outside 8000..192000")


def block_count(n: int, fs: int, window_steps: int) -> int:
    return max(n // (fs // 10) - window_steps + 1, 0)


def left_to_right(e, window_steps: int, step: int) -> np.ndarray:
    """z_k = (((e_k + e_{k+1}) + ...) + e_{k+W-1}) / (W step) in fp64, in that order."""
    e = np.asarray(e, dtype=np.float64)
    k = max(e.shape[0] - window_steps + 1, 0)
    z = e[:k].copy()
    for i in range(1, window_steps):
        z = z + e[i:i + k]
    return z / (float(window_steps) * float(step))


def series(x, fs: int, window_steps: int) -> dict:
    """The blocks of W steps, one a step: their mean squares and loudness, from the fp64 step energies."""
    e = L.energies64(x, fs)
    z = left_to_right(e, window_steps, fs // 10)
    return {"energies": e, "z": z, "lufs": L.lkfs(z) if z.size else np.zeros(0)}


def percentile_indices(g: int):
    """EBU Tech 3342's 10th and 95th percentile of g sorted values as 0-based picks: round((g - 1) p / 100), halves up, in integers."""
    assert g >= 1
    return ((g - 1) * 10 + 50) // 100, ((g - 1) * 95 + 50) // 100


def picks(z_gated) -> tuple:
    """(low, high) in LUFS of the gated blocks' mean squares."""
    z = np.sort(np.asarray(z_gated, dtype=np.float64))
    lo, hi = percentile_indices(z.size)
    return float(L.lkfs(z[lo])), float(L.lkfs(z[hi]))


def loudness_range(x, fs: int) -> dict:
    """EBU Tech 3342 on short-term blocks of 3 s every 100 ms, and the margins of the blocks from the two gates (inf where none is near)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1 and L.supported(fs)
    st = series(x, fs, SHORT_STEPS)
    z, l = st["z"], st["lufs"]
    mom = series(x, fs, 4)["lufs"]
    out = {"z": z, "l": l, "blocks": int(z.size), "above_absolute": 0, "gated": 0, "lra": 0.0, "low_lufs": -np.inf, "high_lufs": -np.inf,
           "abs_margin": float(np.min(np.abs(l - L.ABS_GATE))) if z.size else np.inf, "rel_margin": np.inf, "gamma": None,
           "short_term_max": float(l.max()) if l.size else -np.inf, "momentary_max": float(mom.max()) if mom.size else -np.inf}
    absolute = l > L.ABS_GATE
    out["above_absolute"] = int(absolute.sum())
    if not absolute.any():
        return out
    gamma = float(L.lkfs(np.sum(z[absolute]) / absolute.sum())) - 20.0
    passing = absolute & (l > gamma)
    out["gamma"], out["rel_margin"], out["gated"] = gamma, float(np.min(np.abs(l[absolute] - gamma))), int(passing.sum())
    if passing.any():
        out["low_lufs"], out["high_lufs"] = picks(z[passing])
        out["lra"] = out["high_lufs"] - out["low_lufs"]
    return out


def true_peak(x, fs: int) -> dict:
    """max(|x|, |resample_ref(x, fs, L fs)|) of one clip in fp64, with the oversampled signal and each output's sum of |tap x| (the
    yardstick of an fp32 dot product)."""
    x = np.asarray(x)
    assert x.ndim == 1
    up = factor(fs)
    y, absdot = RS.resample_ref(x[None], fs, up * fs)
    peak = float(np.max(np.abs(x.astype(np.float64))))
    return {"factor": up, "y": y[0], "absdot": absdot[0], "peak": peak, "oversampled": float(np.max(np.abs(y[0]))),
            "true_peak": max(peak, float(np.max(np.abs(y[0]))))}
