"""The critical-band measures without a GPU: the twiddle table and the default band filters against long-double designs, the oracle's
radix-2 network (tests/bands_ref.py) against numpy.fft, its peak walk on hand-made band profiles, the scratch formula, every bad argument
refused — through the ABI with pointers that are never dereferenced and through Python on CPU tensors — before any device work, and the
exports against the header."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import bands_ref as R

C = _capi.C
EINVAL = -1
FFTS = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def twiddles(n_fft):
    lib = _capi.load_library()
    out = np.zeros(n_fft, dtype=np.float64)
    assert lib.l3ac_bands_twiddles(n_fft, out.ctypes.data, n_fft) == n_fft
    return out.reshape(n_fft // 2, 2)


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", FFTS)
def test_twiddles_are_their_long_double_design_rounded_once(n_fft):
    """The design here reduces the angle to the nearest quarter turn (|angle| <= pi / 4, signed), the library mirrors it into [0, pi / 4]:
    two reductions, one value.  An unreduced cos near pi / 2 would carry the argument's own rounding, a third of an fp64 ulp of the result."""
    t = twiddles(n_fft)
    pi = 4.0 * np.arctan(np.longdouble(1.0))
    m = np.arange(n_fft // 2)
    q = (4 * m + n_fft // 2) // n_fft  # the nearest quarter turn: 0, 1 or 2
    a = 2.0 * pi * (m - q * (n_fft // 4)).astype(np.longdouble) / np.longdouble(n_fft)
    c, s = np.cos(a), np.sin(a)
    cos = np.where(q == 0, c, np.where(q == 1, -s, -c))
    sin = np.where(q == 0, s, np.where(q == 1, c, -s))
    design = np.stack([cos, -sin], axis=1)
    ulp = np.spacing(np.abs(design.astype(np.float64))).astype(np.longdouble)
    assert (np.abs(t.astype(np.longdouble) - design) <= ulp).all()
    assert t[0].tolist() == [1.0, 0.0] and t[n_fft // 4].tolist() == [0.0, -1.0]
    assert not np.signbit(t[0, 1]) and not np.signbit(t[n_fft // 4, 0])
    assert np.abs(t - R.twiddle_design(n_fft).astype(np.float64)).max() <= 2.0 ** -52  # (and the straight design, absolutely)
    lib = _capi.load_library()
    assert lib.l3ac_bands_twiddles(n_fft, None, 0) == n_fft
    guard = np.full(4, 7.0)
    assert lib.l3ac_bands_twiddles(n_fft, guard.ctypes.data, n_fft - 1) == n_fft and (guard == 7.0).all()  # too small: untouched


def test_critical_bands_is_the_published_table():
    centre, width = l3ac_amd.critical_bands()
    assert centre.dtype == width.dtype == torch.float64 and centre.shape == width.shape == (25,)
    assert tuple(centre.tolist()) == R.CENTRES and tuple(width.tolist()) == R.WIDTHS
    assert centre[-1] < 4000.0  # the table stops below 4 kHz


@pytest.mark.parametrize("fs,n_fft", [(8000, 512), (16000, 1024), (16000, 64), (16000, 4096), (48000, 2048)])
def test_default_weights_are_their_long_double_design_rounded_once(fs, n_fft):
    w = l3ac_amd.band_weights(fs, n_fft).numpy()
    design = R.weights_design(fs, n_fft)
    assert w.shape == (25, n_fft // 2) and w.dtype == np.float64
    assert ((w == 0.0) == (design == 0.0)).all()
    assert (np.abs(w.astype(np.longdouble) - design) <= np.spacing(design.astype(np.float64)).astype(np.longdouble)).all()
    assert (w >= 0).all() and w.max() <= 1.0 and (w.max(axis=1) > 0).all()
    for lo, hi in R.runs(w):  # a band's non-zero weights are one run
        assert hi > lo
    for i, (lo, hi) in enumerate(R.runs(w)):
        assert (w[i, lo:hi] > 0).all() and (w[i, :lo] == 0).all() and (w[i, hi:] == 0).all()
    assert w[0].max() == 1.0  # the narrowest band's gain is 1 at its centre bin


def test_a_custom_table_reaches_where_the_default_does_not():
    w = l3ac_amd.band_weights(16000, 1024, ([1000.0, 4000.0, 7000.0], [200.0, 400.0, 800.0])).numpy()
    assert w.shape == (3, 512) and [int(np.argmax(r)) for r in w] == [64, 256, 448]
    assert l3ac_amd.band_weights(16000, 1024).numpy()[:, 256:].max() == 0.0  # the default weights nothing above 4 kHz


def test_band_weights_refuses_bad_tables():
    for bands, word in ((([100.0, 8000.0], [70.0, 70.0]), "centre_hz"), (([100.0, -1.0], [70.0, 70.0]), "centre_hz"),
                        (([100.0, 200.0], [70.0, 0.0]), "bandwidth_hz"), (([100.0, 200.0], [70.0, -5.0]), "bandwidth_hz"),
                        (([100.0, 200.0], [70.0, float("nan")]), "bandwidth_hz"), (([100.0, 200.0], [1.0, 1000.0]), "no non-zero weight"),
                        (([100.0], [70.0]), "bands"), (([100.0] * 65, [70.0] * 65), "bands"), (([100.0, 200.0], [70.0]), "bandwidths"),
                        ("table", "bands"), (([100.0, "x"], [70.0, 70.0]), "bands")):
        with pytest.raises(ValueError, match=word):
            l3ac_amd.band_weights(16000, 1024, bands)
    for kw in (dict(sample_rate=7999), dict(sample_rate=192001), dict(n_fft=8), dict(n_fft=8192), dict(n_fft=1000)):
        with pytest.raises(ValueError):
            l3ac_amd.band_weights(**kw)
    lib = _capi.load_library()
    two = (C.c_double * 2)(100.0, 200.0)
    assert lib.l3ac_band_weights(16000, 1024, 2, None, two, None, 0) == EINVAL and b"null" in lib.l3ac_last_error()
    assert lib.l3ac_band_weights(16000, 1024, 2, two, two, None, 0) == 2 * 512


def test_default_fft():
    assert [_capi.load_library().l3ac_bands_default_fft(n) for n in (2, 8, 9, 240, 480, 512, 513, 1323, 2048)] == \
        [16, 16, 32, 512, 1024, 1024, 2048, 4096, 4096] == [R.default_fft(n) for n in (2, 8, 9, 240, 480, 512, 513, 1323, 2048)]
    for n in (1, 0, 2049):
        assert _capi.load_library().l3ac_bands_default_fft(n) < 0 and b"frame" in _capi.load_library().l3ac_last_error()


# ---- the oracle against independent mathematics -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n", [(16, 5), (16, 16), (64, 40), (128, 128), (1024, 480), (4096, 2048)])
def test_oracle_network_is_numpys_fft_within_the_derived_bound(n_fft, n):
    """A radix-2 transform in fp64 with twiddles correct to rounding returns y^ with ||y^ - y||_2 <= log2(n_fft) eta ||y||_2, eta = mu +
    gamma_4 (sqrt 2 + mu) < 7 u for mu = u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, theorem 24.2), and ||y||_2 =
    sqrt(n_fft) ||xw||_2.  A bin is off by no more than the whole vector; numpy's transform has its own error of the same size: twice."""
    rng = np.random.default_rng(n_fft + n)
    x = (0.5 * rng.standard_normal(n + 3 * max(n // 4, 1))).astype(np.float32)
    got = R.spectrum(x, n, max(n // 4, 1), n_fft, twiddles(n_fft))
    assert got["re"].shape == (4, n_fft // 2)
    padded = np.zeros((4, n_fft))
    padded[:, :n] = got["xw"]
    want = np.fft.fft(padded, axis=1)[:, :n_fft // 2]
    bound = 2.0 * 7.0 * np.log2(n_fft) * 2.0 ** -53 * np.sqrt(n_fft) * np.linalg.norm(got["xw"], axis=1)
    err = np.abs((got["re"] + 1j * got["im"]) - want).max(axis=1)
    assert (err <= bound).all(), (err / bound).max()
    assert (bound < 1e-10).all()  # (a bound that says something: the bins themselves are of order sqrt(n) ||xw|| / sqrt(n_fft) >= 0.1)
    assert np.array_equal(got["power"], got["re"] ** 2 + got["im"] ** 2) and np.array_equal(got["magnitude"], np.sqrt(got["power"]))


def test_oracle_network_on_exact_frames():
    tw = twiddles(64)
    const = R.spectrum(np.full(64, 0.375, dtype=np.float32), 64, 16, 64, tw, kind="rect")
    assert const["re"][0, 0] == 24.0 and (const["re"][0, 1:] == 0.0).all() and (const["im"][0] == 0.0).all()
    alt = 0.375 * (-1.0) ** np.arange(64)
    alt = R.spectrum(alt.astype(np.float32), 64, 16, 64, tw, kind="rect")
    assert (alt["re"][0] == 0.0).all() and (alt["im"][0] == 0.0).all() and alt["magnitude_sum"][0] == 0.0


def test_oracle_peak_walk_on_hand_made_profiles():
    walk = lambda profile: (R.peak_walk(np.array(profile, dtype=np.float64))[0].tolist(), R.peak_walk(np.array(profile, dtype=np.float64))[1])
    assert walk([1, 2, 3, 4, 5]) == ([4, 4, 4, 4], 4)              # rising throughout: the peak at the upper end
    assert walk([5, 4, 3, 2, 1]) == ([0, 0, 0, 0], 0)              # falling throughout: the walk runs off the lower end, the peak is band 0
    assert walk([1, 3, 3, 3, 2]) == ([1, 1, 1, 1], 1)              # a plateau is not rising: its first band is the peak, and the first maximum
    assert walk([1, 5, 2, 1, 4, 6, 3]) == ([1, 1, 1, 5, 5, 5], 5)  # two peaks: each slope takes the one in its direction
    assert walk([2, 2, 2]) == ([0, 0], 0)                          # all equal (the floor of a silent frame)
    assert walk([3, 1, 2]) == ([0, 2], 0)                          # a peak at either end
    nan = float("nan")
    assert walk([nan, nan, nan]) == ([0, 0], 0)                    # nothing compares: every walk still ends inside the table


def test_oracle_measures_on_a_pair_and_on_itself():
    fs, n, hop, n_fft = 16000, 480, 120, 1024
    from tests.lpc_ref import add_noise, resonator
    ref = resonator(3000, fs, seed=7)
    w = l3ac_amd.band_weights(fs, n_fft).numpy()
    tw = twiddles(n_fft)
    own, fv = R.metrics(ref, ref.copy(), n, hop, n_fft, tw, w)
    assert own["fw_seg_snr_db"] == 35.0 and own["wss"] == 0.0 and own["lsd_db"] == 0.0 and own["snr_frames"] == own["frames"] == 22
    assert (fv["bounds"]["wss"] < 1e-9).all() and (fv["bounds"]["lsd"] < 1e-6).all()
    noisy, _ = R.metrics(ref, add_noise(ref, 10.0, 1), n, hop, n_fft, tw, w)
    clean, fv = R.metrics(ref, add_noise(ref, 30.0, 1), n, hop, n_fft, tw, w)
    assert noisy["fw_seg_snr_db"] < clean["fw_seg_snr_db"] < 35.0 and noisy["wss"] > clean["wss"] > 0.0 and noisy["lsd_db"] > clean["lsd_db"] > 0.0
    assert (fv["bounds"]["fw"] < 1e-11).all() and (fv["bounds"]["wss"] < 1e-9).all() and (fv["bounds"]["lsd"] < 1e-11).all()
    silent, _ = R.metrics(np.zeros(1000, dtype=np.float32), np.zeros(1000, dtype=np.float32), n, hop, n_fft, tw, w)
    assert silent["snr_frames"] == 0 and np.isnan(silent["fw_seg_snr_db"]) and silent["lsd_db"] == 0.0 and silent["wss"] == 0.0


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------
def test_scratch_sizes():
    lib = _capi.load_library()
    up = lambda v: 256 * -(-v // 256)
    for b, t, n, hop, n_fft, nb in ((1, 1, 5, 1, 16, 2), (3, 4000, 480, 120, 1024, 25), (65, 500, 33, 1, 64, 64), (2, 16384 * 2 + 98, 100, 2, 256, 3)):
        f = R.n_frames(t, n, hop)
        assert lib.l3ac_frame_spectrum_scratch_bytes(b, t, n, hop, n_fft) == up(4 * b)
        assert lib.l3ac_band_metrics_scratch_bytes(b, t, n, hop, n_fft, nb) == up(4 * b) + up(24 * b * f) + up(4 * b * f), (b, t, n, hop)
    assert lib.l3ac_band_metrics_scratch_bytes(2, 16384 * 2 + 100, 100, 2, 256, 25) < 0 and b"16385 frames" in lib.l3ac_last_error()
    assert lib.l3ac_frame_spectrum_scratch_bytes(2, 16384 * 2 + 100, 100, 2, 256) == 256  # the spectrum itself has no frame cap
    for bad, word in (((0, 100, 64, 16, 128, 25), b"batch"), ((65536, 100, 64, 16, 128, 25), b"batch"), ((1, 0, 64, 16, 128, 25), b"max_samples"),
                      ((1, 100, 1, 16, 128, 25), b"frame"), ((1, 100, 2049, 16, 4096, 25), b"frame"), ((1, 100, 64, 0, 128, 25), b"hop"),
                      ((1, 100, 64, -2, 128, 25), b"hop"), ((1, 100, 64, 16, 8, 25), b"n_fft"), ((1, 100, 64, 16, 8192, 25), b"n_fft"),
                      ((1, 100, 64, 16, 100, 25), b"n_fft"), ((1, 100, 65, 16, 64, 25), b"n_fft"), ((1, 100, 64, 16, 128, 1), b"bands"),
                      ((1, 100, 64, 16, 128, 65), b"bands"), ((1, 100, 64, 16, 128, 0), b"bands")):
        assert lib.l3ac_band_metrics_scratch_bytes(*bad) < 0 and word in lib.l3ac_last_error(), bad
        if word != b"bands":
            assert lib.l3ac_frame_spectrum_scratch_bytes(*bad[:5]) < 0 and word in lib.l3ac_last_error(), bad


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, n, hop, n_fft, nb = 4096, 3000, 240, 60, 512, 25
    need = lib.l3ac_frame_spectrum_scratch_bytes(2, t, n, hop, n_fft)
    ok = (C.c_int32 * 2)(3000, 100)
    geometry = (dict(n=1), dict(n=2049, n_fft=4096), dict(n=513), dict(hop=0), dict(hop=-1), dict(n_fft=8), dict(n_fft=8192), dict(n_fft=768),
                dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=(C.c_int32 * 2)(0, 5)), dict(lens=(C.c_int32 * 2)(3000, 3001)),
                dict(lens=(C.c_int32 * 2)(-7, 5)), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=0))

    def spectrum(audio=fake, stride=t, batch=2, t=t, lens=ok, n=n, hop=hop, n_fft=n_fft, window=fake, tw=fake, spec=fake, scratch=fake, nbytes=need):
        return lib.l3ac_frame_spectrum(audio, stride, batch, t, lens, n, hop, n_fft, window, tw, spec, None, None, None, None, scratch, nbytes, None)

    # refused on the arguments alone, whatever the pointers: nothing is launched or dereferenced
    for kw in geometry + (dict(stride=t - 1), dict(audio=None), dict(tw=None), dict(spec=None), dict(nbytes=need - 1)):
        assert spectrum(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert spectrum(n=2049, n_fft=4096) == EINVAL and b"frame" in lib.l3ac_last_error()
    assert spectrum(n=513) == EINVAL and b"n_fft 512 is below the frame 513" in lib.l3ac_last_error()
    assert spectrum(n_fft=768) == EINVAL and b"power of two" in lib.l3ac_last_error()
    assert spectrum(hop=0) == EINVAL and b"hop" in lib.l3ac_last_error()
    assert spectrum(nbytes=need - 1) == EINVAL and b"scratch" in lib.l3ac_last_error()
    assert spectrum(lens=(C.c_int32 * 2)(3000, 0)) == EINVAL and b"samples[1]" in lib.l3ac_last_error()

    def energies(audio=fake, stride=t, batch=2, t=t, lens=ok, n=n, hop=hop, n_fft=n_fft, window=fake, tw=fake, wt=fake, nb=nb, power=fake, mag=fake,
                 scratch=fake, nbytes=need):
        return lib.l3ac_band_energies(audio, stride, batch, t, lens, n, hop, n_fft, window, tw, wt, nb, power, mag, None, scratch, nbytes, None)

    for kw in geometry + (dict(stride=t - 1), dict(audio=None), dict(tw=None), dict(wt=None), dict(power=None), dict(mag=None), dict(nb=0), dict(nb=1),
                          dict(nb=65), dict(nbytes=need - 1)):
        assert energies(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert energies(nb=65) == EINVAL and b"bands" in lib.l3ac_last_error()

    need = lib.l3ac_band_metrics_scratch_bytes(2, t, n, hop, n_fft, nb)
    nan = float("nan")

    def metrics(ref=fake, rs=t, est=fake, es=t, batch=2, t=t, lens=ok, n=n, hop=hop, n_fft=n_fft, window=fake, tw=fake, wt=fake, nb=nb, gamma=0.2,
                norm=1, trim=0.95, out=fake, counts=fake, scratch=fake, nbytes=need):
        return lib.l3ac_band_metrics(ref, rs, est, es, batch, t, lens, n, hop, n_fft, window, tw, wt, nb, gamma, norm, trim, out, counts, None, None,
                                     None, None, None, scratch, nbytes, None)

    for kw in geometry + (dict(rs=t - 1), dict(es=t - 1), dict(ref=None), dict(est=None), dict(tw=None), dict(wt=None), dict(out=None),
                          dict(counts=None), dict(nb=0), dict(nb=1), dict(nb=65), dict(gamma=nan), dict(gamma=float("inf")), dict(norm=2),
                          dict(norm=-1), dict(trim=0.0), dict(trim=-0.5), dict(trim=1.0001), dict(trim=nan), dict(nbytes=need - 1),
                          dict(t=16384 * 2 + 100, n=100, hop=2, rs=40000, es=40000, nbytes=1 << 30)):
        assert metrics(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert metrics(trim=0.0) == EINVAL and b"trim" in lib.l3ac_last_error()
    assert metrics(gamma=nan) == EINVAL and b"gamma" in lib.l3ac_last_error()
    assert metrics(norm=2) == EINVAL and b"normalize" in lib.l3ac_last_error()
    assert metrics(nbytes=need - 1) == EINVAL and b"scratch" in lib.l3ac_last_error()
    assert metrics(t=16384 * 2 + 100, n=100, hop=2, rs=40000, es=40000, nbytes=1 << 30) == EINVAL and b"frames" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 3000)
    calls = (lambda **kw: l3ac_amd.frame_spectrum(x, **kw), lambda **kw: l3ac_amd.band_energies(x, **kw), lambda **kw: l3ac_amd.band_metrics(x, x, **kw))
    for kw in (dict(frame=1), dict(frame=2049), dict(frame=513, n_fft=512), dict(hop=0), dict(n_fft=8), dict(n_fft=8192), dict(n_fft=1000),
               dict(sample_rate=7999), dict(sample_rate=192001), dict(window="hamming"), dict(window=None), dict(frame="long"),
               dict(lengths=[0, 5]), dict(lengths=[3001, 5]), dict(lengths=[5]), dict(lengths=[2.5, 5])):
        for call in calls:
            with pytest.raises(ValueError):  # the parameter first, on CPU tensors
                call(**kw)
    with pytest.raises(ValueError, match="n_fft"):
        l3ac_amd.frame_spectrum(x, n_fft=1000)
    with pytest.raises(ValueError, match="window"):
        l3ac_amd.band_metrics(x, x, window="hamming")
    for kw in (dict(bands=([100.0, 9000.0], [70.0, 70.0])), dict(bands=([100.0], [70.0])), dict(bands=([100.0, 200.0], [70.0, 0.0])), dict(bands=7)):
        for call in calls[1:]:
            with pytest.raises(ValueError):
                call(**kw)
    with pytest.raises(ValueError, match="centre_hz"):  # the default table reaches 3.6 kHz: below Nyquist at 8 kHz, but a table to 7 kHz is not
        l3ac_amd.band_metrics(x, x, sample_rate=8000, bands=([1000.0, 7000.0], [200.0, 800.0]))
    for kw in (dict(trim=0.0), dict(trim=1.5), dict(trim=float("nan")), dict(trim=-1.0)):
        with pytest.raises(ValueError, match="trim"):
            l3ac_amd.band_metrics(x, x, **kw)
    for bad in (float("nan"), float("inf"), "big"):
        with pytest.raises(ValueError, match="gamma"):
            l3ac_amd.band_metrics(x, x, gamma=bad)
    with pytest.raises(ValueError, match="differ in shape"):
        l3ac_amd.band_metrics(x, torch.zeros(2, 3001))
    with pytest.raises(ValueError, match="batch, samples"):
        l3ac_amd.frame_spectrum(torch.zeros(3000))
    with pytest.raises(ValueError, match="16385 frames"):
        l3ac_amd.band_metrics(torch.zeros(1, 16384 * 2 + 100), torch.zeros(1, 16384 * 2 + 100), frame=100, hop=2)
    for call in (lambda: l3ac_amd.frame_spectrum(x), lambda: l3ac_amd.frame_spectrum(x.numpy()), lambda: l3ac_amd.band_energies(x, window="rect"),
                 lambda: l3ac_amd.band_metrics(x, x), lambda: l3ac_amd.band_metrics(x, x, lengths=[3000, 100], return_frames=True),
                 lambda: l3ac_amd.frame_spectrum(torch.zeros(1, 16384 * 2 + 100), frame=100, hop=2)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_exports_and_abi_version():
    for name in ("frame_spectrum", "band_energies", "band_metrics", "band_weights", "critical_bands"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    assert _capi.load_library().l3ac_abi_version() == 5
    assert "DESIGN.md section 3.22" in header
    assert "256 ceil(24 batch F / 256)" in header  # the closed form of the metrics scratch is stated
    assert "bands" in inspect.signature(l3ac_amd.L3AC.evaluate).parameters
    assert inspect.signature(l3ac_amd.L3AC.evaluate).parameters["bands"].default is False
    text = (Path(__file__).resolve().parents[1] / "INTEGRATION.md").read_text()
    for name in ("l3ac_bands_twiddles", "l3ac_band_weights", "l3ac_frame_spectrum", "l3ac_band_metrics_scratch_bytes", "l3ac_band_metrics"):
        assert name in text
    source = (Path(__file__).resolve().parents[1] / "l3ac_amd" / "csrc" / "kernels" / "bands.hip").read_text()
    assert "#pragma clang fp contract(off)" in source and not re.search(r"\batomic[A-Z]\w*\s*\(|__hip_atomic|__atomic_", source)  # no atomics
