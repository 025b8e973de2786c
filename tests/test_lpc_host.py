"""Linear prediction and the envelope measures without a GPU: the window against its fp64 design, the frame geometry and the defaults, the
oracle (tests/lpc_ref.py) against independent mathematics — the Toeplitz solve, the FFT cepstrum, LLR >= 0 — the trimming count, every bad
argument refused — through the ABI with pointers that are never dereferenced and through Python on CPU tensors — before any device work,
and the exports against the header."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import lpc_ref as R

C = _capi.C
EINVAL = -1


# ---- the window, the geometry, the defaults -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5, 63, 64, 65, 240, 480, 1323, 8192])
def test_window_is_its_fp64_design_rounded_once(n):
    w = l3ac_amd.lpc_window(n).numpy()
    design = R.window_design(n)
    assert w.shape == (n,) and w.dtype == np.float32
    assert (np.abs(w.astype(np.float64) - design) <= np.spacing(design.astype(np.float32)).astype(np.float64)).all()  # 1 fp32 ulp
    assert (w > 0).all() and (w <= 1).all()
    assert design[0] == 0.5 * (1.0 - np.cos(2.0 * np.pi / (n + 1.0)))  # i + 1 over N + 1: no zero at either end
    lib = _capi.load_library()
    assert lib.l3ac_lpc_window(n, None, 0) == n
    guard = np.full(4, 7.0, dtype=np.float32)
    assert lib.l3ac_lpc_window(n, guard.ctypes.data, n - 1) == n and (guard == 7.0).all()  # too small: untouched


def test_window_refuses_unsupported_frames():
    lib = _capi.load_library()
    for n in (1, 0, -3, 8193):
        assert lib.l3ac_lpc_window(n, None, 0) < 0 and b"frame" in lib.l3ac_last_error()
        with pytest.raises(ValueError, match="frame"):
            l3ac_amd.lpc_window(n)


@pytest.mark.parametrize("n,hop", [(240, 60), (65, 7), (100, 100), (17, 40)])
def test_frame_counts_at_their_edges(n, hop):
    assert l3ac_amd.lpc_frames(n - 1, n, hop) == 0
    assert l3ac_amd.lpc_frames(n, n, hop) == 1
    assert l3ac_amd.lpc_frames(n + hop - 1, n, hop) == 1
    assert l3ac_amd.lpc_frames(n + hop, n, hop) == 2
    assert l3ac_amd.lpc_frames(0, n, hop) == 0
    for s in (n - 1, n, n + hop - 1, n + hop, 5 * n + 3):
        assert l3ac_amd.lpc_frames(s, n, hop) == R.n_frames(s, n, hop)
    for bad in ((-1, n, hop), (100, 1, hop), (100, 8193, hop), (100, n, 0)):
        with pytest.raises(ValueError):
            l3ac_amd.lpc_frames(*bad)


def test_defaults():
    assert l3ac_amd.lpc_defaults(8000) == (10, 240, 60)
    assert l3ac_amd.lpc_defaults(16000) == (16, 480, 120)
    assert l3ac_amd.lpc_defaults(22050) == (16, 662, 165)  # (30 * 22050 + 500) // 1000 = 662: 661.5 rounds up
    assert l3ac_amd.lpc_defaults(44100) == (16, 1323, 330)
    assert l3ac_amd.lpc_defaults(9999)[0] == 10 and l3ac_amd.lpc_defaults(10000)[0] == 16
    for fs in (8000, 16000, 22050, 44100, 192000):
        assert l3ac_amd.lpc_defaults(fs) == R.defaults(fs)
    for fs in (7999, 192001, 0, -16000):
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.lpc_defaults(fs)


# ---- the oracle against independent mathematics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n", [(4, 65), (10, 240), (16, 480), (32, 100)])
def test_oracle_levinson_solves_the_toeplitz_system(p, n):
    x = R.resonator(n + 3 * (n // 4), 16000, seed=p)
    got = R.lpc(x, 16000, p, n, n // 4)
    assert got["valid"].all() and len(got["valid"]) == 4
    for f in range(4):
        r = got["autocorr"][f]
        toeplitz = r[np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])]
        want = np.linalg.solve(toeplitz, -r[1:])
        cond = np.linalg.cond(toeplitz)
        assert np.abs(got["a"][f, 1:] - want).max() <= 1e-13 * cond * max(1.0, np.abs(want).max())
        assert got["a"][f, 0] == 1.0 and (np.abs(got["reflection"][f]) < 1.0).all() and got["reflection"][f, -1] == got["a"][f, -1]
        assert abs(got["error"][f] - (r[0] + got["a"][f, 1:] @ r[1:])) <= 1e-12 * cond * got["error"][f]  # E_p = r[0] + sum a[i] r[i]
        assert abs(R.quad(got["a"][f:f + 1], got["autocorr"][f:f + 1])[0] - got["error"][f]) <= 1e-12 * cond * got["error"][f]  # q(a, r) = E_p
    direct = np.array([[got["xw"][f, :n - k] @ got["xw"][f, k:] for k in range(p + 1)] for f in range(4)])
    assert np.abs(got["autocorr"] - direct).max() <= 1e-13 * got["autocorr"][:, 0].max()  # the stated order against BLAS's


def test_oracle_marks_silent_frames_invalid_and_keeps_their_autocorr():
    x = R.resonator(600, 8000, seed=3)
    x[100:400] = 0.0
    got = R.lpc(x, 8000, 10, 100, 25)
    silent = [f for f in range(len(got["valid"])) if 100 <= 25 * f and 25 * f + 100 <= 400]
    assert silent and not got["valid"][silent].any() and got["valid"][0] == 1
    assert np.isnan(got["a"][silent]).all() and np.isnan(got["error"][silent]).all() and (got["autocorr"][silent] == 0.0).all()


def test_oracle_cepstrum_is_the_fft_cepstrum_of_one_over_a():
    rng = np.random.default_rng(8)
    for p in (1, 4, 10, 16, 32):
        radius, angle = rng.uniform(0.3, 0.9, p), rng.uniform(0.0, np.pi, p)
        roots = np.concatenate([radius[:p // 2] * np.exp(1j * angle[:p // 2]), radius[:p // 2] * np.exp(-1j * angle[:p // 2]),
                                radius[p // 2:p - p // 2] * np.sign(rng.standard_normal(p - 2 * (p // 2)))])
        a = np.real(np.poly(roots))  # minimum phase: every root inside the unit circle
        assert len(a) == p + 1 and a[0] == 1.0
        c = R.cepstrum(a[None, :])[0]
        n_fft = 1 << 14
        spec = np.fft.fft(a, n_fft)
        log_spec = np.log(np.abs(spec)) + 1j * np.unwrap(np.angle(spec))  # (the phase of a minimum-phase A is continuous and periodic)
        want = np.real(np.fft.ifft(-log_spec))  # the cepstrum of 1 / A; aliasing ~ 0.9^16384
        assert np.abs(c[1:] - want[1:p + 1]).max() <= 1e-12 * max(1.0, np.abs(want[1:p + 1]).max())


def test_llr_is_not_negative_before_clamping_on_random_pairs():
    for seed, (p, n, fs) in enumerate([(4, 64, 8000), (10, 240, 8000), (16, 480, 16000), (32, 100, 16000)]):
        ref = R.resonator(n + 5 * (n // 4), fs, seed=20 + seed)
        est = R.add_noise(ref, 10.0, seed=40 + seed)
        a, b = R.lpc(ref, fs, p, n, n // 4), R.lpc(est, fs, p, n, n // 4)
        assert a["valid"].all() and b["valid"].all()
        num, g_r = R.quad(b["a"], a["autocorr"]), R.quad(a["a"], a["autocorr"])
        assert (num > 0).all() and (g_r > 0).all() and (np.log(num / g_r) >= 0.0).all()  # a_r minimises a' R_r a over a[0] = 1
        fv = R.frame_values(a, b, llr_max=1e9, is_max=1e9, cd_max=1e9)
        assert (fv["is"] >= 0).all() and (fv["cd"] > 0).all()


def test_trim_count_and_trimmed_mean():
    assert [R.trim_count(0.95, v) for v in (0, 1, 10, 30)] == [0, 1, 10, 29]  # floor(0.95 V + 0.5): 0.5, 1.45, 10.0, 29.0
    assert [R.trim_count(1.0, v) for v in (1, 10, 30)] == [1, 10, 30]
    assert [R.trim_count(0.04, v) for v in (1, 10, 30)] == [0, 0, 1]
    vals = np.array([5.0, 1.0, 3.0, 2.0, 4.0, 100.0, 0.5, 0.25, 7.0, 6.0])
    assert R.trimmed_mean(vals, 1.0) == np.sort(vals).cumsum()[-1] / 10.0
    assert R.trimmed_mean(vals, 0.85) == (0.25 + 0.5 + 1.0 + 2.0 + 3.0 + 4.0 + 5.0 + 6.0 + 7.0) / 9.0
    assert np.isnan(R.trimmed_mean(np.array([]), 0.95)) and np.isnan(R.trimmed_mean(np.array([3.0]), 0.04))


def test_oracle_on_the_sanity_inputs():
    """The inputs of the GPU suite's sanity test satisfy it with room to spare, and the ill-conditioned pair stays valid."""
    fs, p, n, hop = 8000, 10, 240, 60
    ref = R.resonator(3000, fs, seed=7)
    m20, _ = R.metrics(ref, R.add_noise(ref, 20.0, 1), fs, p, n, hop)
    m40, _ = R.metrics(ref, R.add_noise(ref, 40.0, 1), fs, p, n, hop)
    assert m20["lpc_frames"] == m20["frames"] == R.n_frames(3000, n, hop)
    assert m20["llr"] > 2.0 * m40["llr"] > 0.0
    assert abs(m20["seg_snr_db"] - 20.0) < 0.5  # (the GPU test allows 1 dB)
    assert 34.0 < m40["seg_snr_db"] <= 35.0  # 40 dB is above the clamp of a frame
    sine = R.lpc(R.sine_plus_noise(1500, fs, seed=2), fs, p, n, hop)
    assert sine["valid"].all() and (sine["error"] / sine["autocorr"][:, 0]).max() < 1e-5  # ill-conditioned, still valid


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def test_scratch_sizes():
    lib = _capi.load_library()
    up = lambda v: 256 * -(-v // 256)
    for b, t, p, n, hop in ((1, 1, 4, 5, 1), (3, 4000, 10, 240, 60), (65, 500, 32, 33, 1), (2, 16384 * 2 + 98, 16, 100, 2)):
        f = R.n_frames(t, n, hop)
        assert lib.l3ac_lpc_scratch_bytes(b, t, 16000, p, n, hop) == up(4 * b)
        assert lib.l3ac_lpc_metrics_scratch_bytes(b, t, 16000, p, n, hop) == up(4 * b) + up(32 * b * f) + up(4 * b * f), (b, t, p, n, hop)
    assert lib.l3ac_lpc_metrics_scratch_bytes(2, 16384 * 2 + 98, 16000, 16, 100, 2) > 0  # exactly 16384 frames
    assert lib.l3ac_lpc_metrics_scratch_bytes(2, 16384 * 2 + 100, 16000, 16, 100, 2) < 0 and b"16385 frames" in lib.l3ac_last_error()
    assert lib.l3ac_lpc_scratch_bytes(2, 16384 * 2 + 100, 16000, 16, 100, 2) == 256  # lpc itself has no frame cap
    for bad, word in (((0, 100, 16000, 4, 64, 16), b"batch"), ((65536, 100, 16000, 4, 64, 16), b"batch"), ((1, 0, 16000, 4, 64, 16), b"max_samples"),
                      ((1, 100, 7999, 4, 64, 16), b"sample_rate"), ((1, 100, 192001, 4, 64, 16), b"sample_rate"), ((1, 100, 16000, 0, 64, 16), b"order"),
                      ((1, 100, 16000, 33, 64, 16), b"order"), ((1, 100, 16000, 16, 16, 4), b"frame"), ((1, 100, 16000, 4, 8193, 16), b"frame"),
                      ((1, 100, 16000, 4, 64, 0), b"hop"), ((1, 100, 16000, 4, 64, -2), b"hop")):
        for fn in (lib.l3ac_lpc_scratch_bytes, lib.l3ac_lpc_metrics_scratch_bytes):
            assert fn(*bad) < 0 and word in lib.l3ac_last_error(), bad


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, fs, p, n, hop = 4096, 3000, 8000, 10, 240, 60
    need = lib.l3ac_lpc_scratch_bytes(2, t, fs, p, n, hop)
    ok = (C.c_int32 * 2)(3000, 100)

    def lpc(audio=fake, stride=t, batch=2, t=t, lens=ok, fs=fs, p=p, n=n, hop=hop, window=fake, a=fake, k=fake, e=fake, r=fake, valid=fake, frames=None,
            scratch=fake, nbytes=need):
        return lib.l3ac_lpc(audio, stride, batch, t, lens, fs, p, n, hop, window, a, k, e, r, valid, frames, scratch, nbytes, None)

    # refused on the arguments alone, whatever the pointers: nothing is launched or dereferenced
    for kw in (dict(p=0), dict(p=33), dict(p=-1), dict(p=10, n=10), dict(p=32, n=32), dict(n=8193), dict(n=0), dict(hop=0), dict(hop=-1), dict(fs=7999),
               dict(fs=192001), dict(batch=0), dict(batch=65536), dict(t=0), dict(stride=t - 1), dict(lens=(C.c_int32 * 2)(0, 5)),
               dict(lens=(C.c_int32 * 2)(3000, 3001)), dict(lens=(C.c_int32 * 2)(-7, 5)), dict(audio=None), dict(a=None), dict(k=None), dict(e=None),
               dict(r=None), dict(valid=None), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=need - 1), dict(nbytes=0)):
        assert lpc(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert lpc(p=33) == EINVAL and b"order" in lib.l3ac_last_error()
    assert lpc(p=10, n=10) == EINVAL and b"frame" in lib.l3ac_last_error()
    assert lpc(hop=0) == EINVAL and b"hop" in lib.l3ac_last_error()
    assert lpc(fs=7999) == EINVAL and b"sample_rate" in lib.l3ac_last_error()
    assert lpc(nbytes=need - 1) == EINVAL and b"scratch" in lib.l3ac_last_error()
    assert lpc(lens=(C.c_int32 * 2)(3000, 0)) == EINVAL and b"samples[1]" in lib.l3ac_last_error()

    need = lib.l3ac_lpc_metrics_scratch_bytes(2, t, fs, p, n, hop)
    nan = float("nan")

    def metrics(ref=fake, rs=t, est=fake, es=t, batch=2, t=t, lens=ok, fs=fs, p=p, n=n, hop=hop, window=fake, trim=0.95, llr=2.0, is_=100.0, cd=10.0,
                out=fake, counts=fake, vals=None, forms=None, scratch=fake, nbytes=need):
        return lib.l3ac_lpc_metrics(ref, rs, est, es, batch, t, lens, fs, p, n, hop, window, trim, llr, is_, cd, out, counts, vals, forms, scratch, nbytes,
                                    None)

    for kw in (dict(p=0), dict(p=33), dict(p=10, n=10), dict(n=8193), dict(hop=0), dict(fs=7999), dict(fs=192001), dict(batch=0), dict(batch=65536),
               dict(t=0), dict(rs=t - 1), dict(es=t - 1), dict(lens=(C.c_int32 * 2)(0, 5)), dict(lens=(C.c_int32 * 2)(3000, 3001)), dict(trim=0.0),
               dict(trim=-0.5), dict(trim=1.0001), dict(trim=nan), dict(llr=-1.0), dict(llr=nan), dict(llr=float("inf")), dict(is_=-1e-9), dict(is_=nan),
               dict(cd=-3.0), dict(cd=nan), dict(ref=None), dict(est=None), dict(out=None), dict(counts=None), dict(scratch=None),
               dict(scratch=fake + 128), dict(nbytes=need - 1), dict(nbytes=0), dict(t=16384 * 2 + 100, n=100, hop=2, rs=40000, es=40000, nbytes=1 << 30)):
        assert metrics(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert metrics(trim=0.0) == EINVAL and b"trim" in lib.l3ac_last_error()
    assert metrics(llr=nan) == EINVAL and b"llr_max" in lib.l3ac_last_error()
    assert metrics(is_=-1.0) == EINVAL and b"is_max" in lib.l3ac_last_error()
    assert metrics(cd=nan) == EINVAL and b"cd_max" in lib.l3ac_last_error()
    assert metrics(nbytes=need - 1) == EINVAL and b"scratch" in lib.l3ac_last_error()
    assert metrics(t=16384 * 2 + 100, n=100, hop=2, rs=40000, es=40000, nbytes=1 << 30) == EINVAL and b"frames" in lib.l3ac_last_error()
    out = (C.c_int32 * 3)()
    assert lib.l3ac_lpc_defaults(16000, None) == EINVAL and lib.l3ac_lpc_defaults(16000, out) == 0 and list(out) == [16, 480, 120]


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 3000)
    for kw in (dict(order=0), dict(order=33), dict(order=10, frame=10), dict(frame=8193), dict(hop=0), dict(sample_rate=7999), dict(sample_rate=192001),
               dict(window="hamming"), dict(window=None), dict(order="many")):
        with pytest.raises(ValueError):  # the parameter first, on CPU tensors
            l3ac_amd.lpc(x, **kw)
        with pytest.raises(ValueError):
            l3ac_amd.lpc_metrics(x, x, **kw)
    with pytest.raises(ValueError, match="order"):
        l3ac_amd.lpc(x, order=33)
    with pytest.raises(ValueError, match="window"):
        l3ac_amd.lpc(x, window="hamming")
    for kw in (dict(trim=0.0), dict(trim=1.5), dict(trim=float("nan")), dict(trim=-1.0)):
        with pytest.raises(ValueError, match="trim"):
            l3ac_amd.lpc_metrics(x, x, **kw)
    for name in ("llr_max", "is_max", "cd_max"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                l3ac_amd.lpc_metrics(x, x, **{name: bad})
    for kw in (dict(lengths=[0, 5]), dict(lengths=[3001, 5]), dict(lengths=[5]), dict(lengths=[1, 2, 3]), dict(lengths=[2.5, 5])):
        with pytest.raises(ValueError, match="lengths"):
            l3ac_amd.lpc(x, **kw)
        with pytest.raises(ValueError, match="lengths"):
            l3ac_amd.lpc_metrics(x, x, **kw)
    with pytest.raises(ValueError, match="differ in shape"):
        l3ac_amd.lpc_metrics(x, torch.zeros(2, 3001))
    with pytest.raises(ValueError, match="differ in shape"):
        l3ac_amd.lpc_metrics(x, torch.zeros(3, 3000))
    with pytest.raises(ValueError, match="batch, samples"):
        l3ac_amd.lpc(torch.zeros(3000))
    with pytest.raises(ValueError, match="16385 frames"):
        l3ac_amd.lpc_metrics(torch.zeros(1, 16384 * 2 + 100), torch.zeros(1, 16384 * 2 + 100), frame=100, hop=2)
    for call in (lambda: l3ac_amd.lpc(x), lambda: l3ac_amd.lpc(x.numpy()), lambda: l3ac_amd.lpc(x, lengths=[1, 3000], window="rect"),
                 lambda: l3ac_amd.lpc_metrics(x, x), lambda: l3ac_amd.lpc_metrics(x, x, lengths=[3000, 100], return_frames=True),
                 lambda: l3ac_amd.lpc_metrics(torch.zeros(1, 16384 * 2 + 98), torch.zeros(1, 16384 * 2 + 98), frame=100, hop=2)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_exports_and_abi_version():
    for name in ("lpc", "lpc_metrics", "lpc_frames", "lpc_defaults", "lpc_window"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5
    assert "DESIGN.md section 3.18" in header
    assert "256 ceil(32 batch F / 256)" in header  # the closed form of the metrics scratch is stated
    assert "lpc" in inspect.signature(l3ac_amd.L3AC.evaluate).parameters
    text = (Path(__file__).resolve().parents[1] / "INTEGRATION.md").read_text()
    for name in ("l3ac_lpc_window", "l3ac_lpc_metrics_scratch_bytes", "l3ac_lpc_metrics"):
        assert name in text
