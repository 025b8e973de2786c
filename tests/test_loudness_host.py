"""Loudness without a GPU: the library's K-weighting design against the standard's table and against the oracle's closed forms
(tests/loudness_ref.py), the state-advance matrix against the oracle's recursion, the block count, the oracle itself on the
standard's compliance sine, and that every bad argument is refused — through the ABI and through Python — before any device work."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import loudness_ref as R


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_coefficients_at_48k_are_the_standards_table():
    """Within 1e-14: the table's 14 printed decimals give at most 5e-15, fp64 rounding of the closed forms 8.9e-16."""
    sos, m = l3ac_amd.loudness_coeffs(48000)
    assert sos.shape == (2, 6) and m.shape == (4, 4) and sos.dtype == m.dtype == torch.float64 and not sos.is_cuda
    assert np.abs(sos.numpy() - R.TABLE_48K).max() <= 1e-14
    assert np.abs(R.coeffs(48000) - R.TABLE_48K).max() <= 1e-14
    lib = _capi.load_library()
    assert lib.l3ac_loudness_coeffs(48000, None, 0) == 28
    buf = torch.full((28,), 7.0, dtype=torch.float64)
    assert lib.l3ac_loudness_coeffs(48000, buf.data_ptr(), 27) == 28 and (buf == 7.0).all()  # a short buffer: the length, nothing written


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 96000])
def test_coefficients_follow_the_closed_forms(fs):
    sos, _ = l3ac_amd.loudness_coeffs(fs)
    want = R.coeffs(fs)
    assert (sos.numpy()[:, 3] == 1.0).all() and (sos.numpy()[1, :3] == [1.0, -2.0, 1.0]).all()
    assert ulps(sos.numpy(), want).max() <= 4, ulps(sos.numpy(), want)


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 48000])
def test_state_matrix_is_the_recursion_from_unit_states(fs):
    sos, m = l3ac_amd.loudness_coeffs(fs)
    want = R.state_matrix(sos.numpy(), fs // 10)  # the oracle's recursion on the library's own coefficients
    assert np.abs(m.numpy() - want).max() <= 1e-15
    assert np.abs(m.numpy()).max() < 1e-3 and np.abs(m.numpy()[2:, 2:]).min() > 1e-12  # 100 ms of decay: small, not zero
    assert np.abs(R.state_matrix(R.coeffs(fs), fs // 10) - want).max() <= 1e-15


def test_block_count():
    lib = _capi.load_library()
    for fs in (8000, 16000, 44100):
        step = fs // 10
        for n, j in ((4 * step - 1, 0), (4 * step, 1), (4 * step + 1, 1), (5 * step - 1, 1), (5 * step, 2), (1, 0), (30 * step, 27)):
            assert lib.l3ac_loudness_blocks(n, fs) == j == l3ac_amd.loudness_blocks(n, fs) == R.blocks(n, fs), (n, fs)
    assert lib.l3ac_loudness_blocks(1 << 40, 48000) == (1 << 40) // 4800 - 3
    for n, fs in ((0, 16000), (-1, 16000), (16000, 11025), (16000, 7990), (16000, 192010)):
        assert lib.l3ac_loudness_blocks(n, fs) < 0 and lib.l3ac_last_error()
        with pytest.raises(ValueError):
            l3ac_amd.loudness_blocks(n, fs)


def test_oracle_reads_the_compliance_sine():
    """A 0 dBFS 997 Hz sine of 5 s at 48 kHz: the standard says -3.01 LKFS."""
    x = np.sin(2 * np.pi * 997.0 * np.arange(5 * 48000) / 48000.0).astype(np.float32)
    o = R.oracle(x, 48000)
    assert abs(o["lufs"] + 3.01) <= 0.01 and o["blocks"] == o["gated"] == 47 and abs(o["peak"] - 1.0) < 1e-6
    assert R.oracle(np.zeros(48000, dtype=np.float32), 48000)["lufs"] == -np.inf
    # the two filters of the oracle agree to what fp64 costs
    assert 0 < R.yardstick(x[:9600], 48000) < 1e-12


def test_oracle_gain():
    assert R.gain_db(-np.inf, 0.5, -23.0, -1.0) == 0.0
    assert R.gain_db(-20.0, 0.5, -23.0) == -3.0 and R.gain_db(-20.0, 0.5, -10.0, -1.0) == -1.0 - 20.0 * np.log10(0.5)
    assert R.gain_db(-20.0, 0.0, -10.0, -1.0) == 10.0


BAD_RATES = (11025, 7990, 192010)


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, fs = 4096, 48000, 16000
    need = lib.l3ac_loudness_scratch_bytes(2, t, fs)
    assert need > 0 and lib.l3ac_loudness_scratch_bytes(3, t, fs) > need and lib.l3ac_loudness_scratch_bytes(2, 1, fs) > 0
    for kw in ((0, t, fs), (65536, t, fs), (2, 0, fs), (2, 1 << 31, fs)) + tuple((2, t, r) for r in BAD_RATES):
        assert lib.l3ac_loudness_scratch_bytes(*kw) < 0 and lib.l3ac_last_error(), kw
    for r in BAD_RATES:
        assert lib.l3ac_loudness_coeffs(r, None, 0) < 0 and b"sample_rate" in lib.l3ac_last_error()
    ok = (_capi.C.c_int32 * 2)(300, t)

    def call(audio=fake, stride=t, batch=2, t=t, lens=ok, fs=fs, stats=fake, counts=fake, mom=None, scratch=fake, nbytes=need):
        return lib.l3ac_loudness(audio, stride, batch, t, lens, fs, stats, counts, mom, scratch, nbytes, None)

    # refused on the arguments alone (EINVAL = -1), whatever the pointers: nothing is launched or dereferenced
    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=(_capi.C.c_int32 * 2)(0, t)), dict(lens=(_capi.C.c_int32 * 2)(300, t + 1)),
               dict(stride=t - 1), dict(audio=None), dict(stats=None), dict(counts=None), dict(scratch=None), dict(scratch=fake + 128),
               dict(nbytes=need - 1)) + tuple(dict(fs=r) for r in BAD_RATES):
        assert call(**kw) == -1 and lib.l3ac_last_error(), kw
    assert call(nbytes=need - 1) == -1 and b"scratch" in lib.l3ac_last_error()
    assert call(stride=t - 1) == -1 and b"stride" in lib.l3ac_last_error()
    assert call(fs=11025) == -1 and b"sample_rate" in lib.l3ac_last_error()
    assert call(lens=(_capi.C.c_int32 * 2)(300, t + 1)) == -1 and b"samples[1]" in lib.l3ac_last_error()

    def gain(stats=fake, batch=2, target=-23.0, limit=math.nan, out=fake):
        return lib.l3ac_loudness_gain(stats, batch, target, limit, out, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(target=math.nan), dict(target=math.inf), dict(target=-math.inf), dict(stats=None),
               dict(out=None)):
        assert gain(**kw) == -1 and lib.l3ac_last_error(), kw
    assert gain(target=math.nan) == -1 and b"target" in lib.l3ac_last_error()

    def apply(audio=fake, stride=t, out=fake, out_stride=t, batch=2, t=t, lens=ok, g=fake, g_stride=1):
        return lib.l3ac_apply_gain(audio, stride, out, out_stride, batch, t, lens, g, g_stride, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=(_capi.C.c_int32 * 2)(0, t)), dict(lens=(_capi.C.c_int32 * 2)(300, t + 1)),
               dict(stride=t - 1), dict(out_stride=t - 1), dict(audio=None), dict(out=None), dict(g=None), dict(g_stride=0)):
        assert apply(**kw) == -1 and lib.l3ac_last_error(), kw


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 48000)
    for rate in BAD_RATES + (0, -16000):  # parameters first, on CPU tensors
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.loudness(x, sample_rate=rate)
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.normalize_loudness(x, sample_rate=rate)
        with pytest.raises(ValueError):
            l3ac_amd.loudness_coeffs(rate)
    stats = {"lufs": torch.zeros(2, dtype=torch.float64), "peak": torch.ones(2, dtype=torch.float64)}
    for target in (math.nan, math.inf, "loud"):
        with pytest.raises(ValueError, match="target_lufs"):
            l3ac_amd.loudness_gain(stats, target_lufs=target)
        with pytest.raises(ValueError, match="target_lufs"):
            l3ac_amd.normalize_loudness(x, target_lufs=target)
    with pytest.raises(ValueError, match="peak_limit_db"):
        l3ac_amd.loudness_gain(stats, peak_limit_db=math.nan)
    for call in (lambda: l3ac_amd.loudness(x), lambda: l3ac_amd.loudness(x.numpy(), 48000), lambda: l3ac_amd.loudness(x, lengths=[0, 1]),
                 lambda: l3ac_amd.loudness(x, lengths=[1, 48001]), lambda: l3ac_amd.loudness_gain(stats), lambda: l3ac_amd.loudness_gain({}),
                 lambda: l3ac_amd.apply_gain(x, torch.ones(2, dtype=torch.float64)), lambda: l3ac_amd.normalize_loudness(x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_evaluate_checks_before_any_device_work():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):  # the network is not on a GPU
        codec.evaluate(torch.zeros(1, 8000), loudness=True)
    codec.config.sample_rate = 11025  # a rate the K-weighting is not defined for: refused first
    try:
        with pytest.raises(ValueError, match="sample_rate"):
            codec.evaluate(torch.zeros(1, 8000), loudness=True)
    finally:
        codec.config.sample_rate = 16000


def test_exports_and_abi_version():
    for name in ("loudness", "loudness_gain", "apply_gain", "normalize_loudness", "loudness_coeffs", "loudness_blocks"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    assert _capi.load_library().l3ac_abi_version() == 5
