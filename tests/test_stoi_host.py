"""STOI / ESTOI without a GPU: the library's two fp32 tables against their fp64 designs, the band runs against the formula, the frame
count, the oracle's spectra (tests/stoi_ref.py) against numpy's FFT, and that every bad argument is refused — through the ABI and
through Python — before any device work."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import stoi_ref as S

RUNS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
        (138, 174), (174, 219)]


def ulp32(v):
    """The spacing of fp32 at |v| (at least that of the smallest normal)."""
    return np.spacing(np.maximum(np.abs(v), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def window():
    lib = _capi.load_library()
    assert lib.l3ac_stoi_window(None, 0) == 256
    w = torch.full((256,), 7.0)
    assert lib.l3ac_stoi_window(w.data_ptr(), 255) == 256 and (w == 7.0).all()  # a short buffer: the length, nothing written
    assert lib.l3ac_stoi_window(w.data_ptr(), 256) == 256
    return w


def test_tables_are_their_fp64_designs_rounded_once():
    w = window().double().numpy()
    want_w = S.window_design()
    # one rounding to fp32 of a design whose own fp64 error (a few 2^-53 absolute, entries <= 1) can move the rounding by one step
    assert (np.abs(w - want_w) <= ulp32(want_w) + 1e-15).all()
    assert w.min() > 0 and np.allclose(want_w, np.hanning(258)[1:-1], rtol=0, atol=1e-15)
    basis = l3ac_amd.stoi_basis()
    assert basis.shape == (514, 256) and basis.dtype == torch.float32
    got, want = basis.double().numpy(), S.basis_design()
    assert (np.abs(got - want) <= ulp32(want) + 1e-15).all()
    assert (got[0] == w).all()  # row 0, w cos(0), is the window: the kernels read it there
    assert np.abs(got[[1, 513]]).max() < 1e-15  # the sine rows of DC and of bin 256 (j k mod 512 is 0 or 256 there)
    lib = _capi.load_library()
    assert lib.l3ac_stoi_basis(None, 0) == 514 * 256
    buf = torch.full((514 * 256,), 7.0)
    assert lib.l3ac_stoi_basis(buf.data_ptr(), 514 * 256 - 1) == 514 * 256 and (buf == 7.0).all()


def test_band_runs_follow_the_formula():
    assert l3ac_amd.stoi_bands() == S.band_runs() == RUNS
    f = np.arange(257) * 10000.0 / 512
    for i, (lo, hi) in enumerate(RUNS):  # recomputed without argmin: no bin is nearer to the band edge than the one named
        for k, edge in ((lo, 150.0 * 2.0 ** ((2 * i - 1) / 6.0)), (hi, 150.0 * 2.0 ** ((2 * i + 1) / 6.0))):
            assert abs(f[k] - edge) == np.abs(f - edge).min() and abs(f[k] - edge) < np.abs(np.delete(f, k) - edge).min()
    assert all(RUNS[i][1] == RUNS[i + 1][0] for i in range(14))


def test_frame_count():
    lib = _capi.load_library()
    for n, a in [(1, 0), (256, 0), (257, 1), (384, 1), (385, 2), (4096, 30), (4097, 31), (1 << 40, ((1 << 40) - 256) // 128)]:
        assert lib.l3ac_stoi_frames(n) == a == l3ac_amd.stoi_frames(n) == S.frames(n), n
        assert all(128 * f < n - 256 for f in range(min(a, 40))) and not 128 * a < n - 256  # the frame that ends at n is not taken
    for n in (0, -1):
        assert lib.l3ac_stoi_frames(n) < 0 and lib.l3ac_last_error()
        with pytest.raises(ValueError):
            l3ac_amd.stoi_frames(n)


def test_oracle_spectra_match_numpy_fft():
    rng = np.random.default_rng(3)
    s = 0.1 * rng.standard_normal(128 * 9 + 256) + 0.3 * np.sin(0.21 * np.arange(128 * 9 + 256))
    w = S.window_design()
    re, im, fr = S.spectra(s, S.basis_design())
    want = np.fft.rfft(fr * w, 512, axis=1)
    assert re.shape == want.shape == (S.frames(s.shape[0]), 257) and S.frames(s.shape[0]) == 9
    assert np.abs(re + 1j * im - want).max() <= 1e-9 * np.abs(want).max()
    # and on the library's fp32 tables the spectra are those of the fp32 window, to fp32 accuracy of the tables
    re32, im32, _ = S.spectra(s, l3ac_amd.stoi_basis().double().numpy())
    assert np.abs(re32 + 1j * im32 - want).max() <= 1e-6 * np.abs(want).max()


def test_oracle_on_a_pair_it_can_check_by_hand():
    """A stationary pair: the estimate a scaled copy of the reference is fully intelligible, independent noise is not."""
    rng = np.random.default_rng(5)
    t = np.arange(8000)
    x = ((1 + 0.8 * np.sin(2 * np.pi * 4 * t / 10000)) * sum(np.sin(2 * np.pi * 170 * h * t / 10000 + h) / h for h in range(1, 20))
         + 0.05 * rng.standard_normal(8000)).astype(np.float32)
    w, basis = window().numpy(), l3ac_amd.stoi_basis().numpy()
    same = S.oracle(x, (0.5 * x).astype(np.float32), w, basis)
    assert same["mask"].all() and same["frames"] == S.frames(8000) - 1 and abs(same["stoi"] - 1) < 1e-9 and abs(same["estoi"] - 1) < 1e-9
    noise = S.oracle(x, rng.standard_normal(8000).astype(np.float32), w, basis)
    assert abs(noise["stoi"]) < 0.4 and abs(noise["estoi"]) < 0.4
    short = S.oracle(x[:4096], x[:4096], w, basis)
    assert short["frames"] == 29 and short["stoi"] == short["estoi"] == 1e-5
    st, es, fr = S.restate32(x, (x + 0.3 * rng.standard_normal(8000)).astype(np.float32), w, basis)
    ref = S.oracle(x, (x + 0.3 * rng.standard_normal(8000)).astype(np.float32), w, basis)
    assert fr == ref["frames"]


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake = 4096
    need = lib.l3ac_stoi_scratch_bytes(2, 5000)
    assert need > 0 and lib.l3ac_stoi_scratch_bytes(3, 5000) > need and lib.l3ac_stoi_scratch_bytes(2, 100) > 0
    assert lib.l3ac_stoi_scratch_bytes(0, 5000) < 0 and lib.l3ac_stoi_scratch_bytes(65536, 5000) < 0 and lib.l3ac_stoi_scratch_bytes(2, 0) < 0
    assert lib.l3ac_stoi_scratch_bytes(1, (1 << 31) - 4096) < 0 and b"too long" in lib.l3ac_last_error()
    assert lib.l3ac_stoi_bands(None) == -1
    ok = (_capi.C.c_int32 * 2)(300, 5000)

    def call(ref=fake, ref_stride=5000, est=fake, est_stride=5000, batch=2, t=5000, lens=ok, basis=fake, out=fake, frames=fake, bands=None,
             scratch=fake, nbytes=need):
        return lib.l3ac_stoi(ref, ref_stride, est, est_stride, batch, t, lens, basis, out, frames, bands, scratch, nbytes, None)

    # refused on the arguments alone (EINVAL = -1), whatever the pointers: nothing is launched or dereferenced
    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(t=(1 << 31) - 4096), dict(lens=(_capi.C.c_int32 * 2)(0, 5000)),
               dict(lens=(_capi.C.c_int32 * 2)(300, 5001)), dict(nbytes=need - 1), dict(ref_stride=4999), dict(est_stride=4999), dict(ref=None),
               dict(est=None), dict(basis=None), dict(basis=fake + 4), dict(out=None), dict(frames=None), dict(scratch=None), dict(scratch=fake + 128)):
        assert call(**kw) == -1 and lib.l3ac_last_error(), kw
    assert call(nbytes=need - 1) == -1 and b"scratch" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 5000)
    for rate in (0, -16000, 10001 * 1024 + 1):  # the resampler's refusals: parameters first, on CPU tensors
        with pytest.raises(ValueError):
            l3ac_amd.stoi(x, x, sample_rate=rate)
    for call in (lambda: l3ac_amd.stoi(x, x), lambda: l3ac_amd.stoi(x, x, sample_rate=10000), lambda: l3ac_amd.stoi(x.numpy(), x.numpy()),
                 lambda: l3ac_amd.stoi(x, x, 10000, lengths=[1, 2])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_evaluate_checks_before_any_device_work():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):  # the network is not on a GPU
        codec.evaluate(torch.zeros(1, 8000), intelligibility=True)


def test_exports_and_abi_version():
    for name in ("stoi", "stoi_frames", "stoi_basis", "stoi_bands"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    assert _capi.load_library().l3ac_abi_version() == 5
