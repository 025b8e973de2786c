"""EBU R128 without a GPU: the oracle (tests/r128_ref.py) on the two level-step signals of EBU Tech 3342, the
percentile picks, the oversampling factor, the shared filter design, the exports and the ABI, and that every bad argument is refused —
through the ABI with fake pointers and through Python on CPU tensors — before any device work."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi, build
from tests import r128_ref as R
from tests import resample_ref as RS

REPO = Path(__file__).resolve().parents[1]
NEW = ("l3ac_r128_scratch_bytes", "l3ac_r128_series", "l3ac_r128_range", "l3ac_true_peak_factor", "l3ac_true_peak_tile",
       "l3ac_true_peak_scratch_bytes", "l3ac_true_peak")


def two_levels(first_db, second_db, fs=8000, seconds=20):
    """A 1 kHz sine, `seconds` at first_db dBFS and then `seconds` at second_db."""
    n = seconds * fs
    x = np.sin(2 * np.pi * 1000.0 * np.arange(2 * n) / fs)
    x[:n] *= 10.0 ** (first_db / 20.0)
    x[n:] *= 10.0 ** (second_db / 20.0)
    return x.astype(np.float32)


@pytest.mark.parametrize("levels, want", [((-20.0, -30.0), 10.0), ((-20.0, -15.0), 5.0)])
def test_oracle_reads_the_tech_3342_level_steps(levels, want):
    """Tech 3342's minimum requirement cases 1 and 2: LRA 10 +- 1 and 5 +- 1 LU there; the oracle gives 10.0000003 and 4.9999997."""
    o = R.loudness_range(two_levels(*levels), 8000)
    print(f"\n[r128] {levels}: oracle LRA {o['lra']:.7f} LU, {o['gated']} of {o['blocks']} blocks")
    assert abs(o["lra"] - want) <= 0.01
    assert o["blocks"] == o["above_absolute"] == o["gated"] == 400 - 29
    assert abs(o["short_term_max"] - (max(levels) - 3.01)) < 0.1  # a sine at A dBFS reads about A - 3 LUFS at 1 kHz


def test_oracle_edges():
    silent = R.loudness_range(np.zeros(5 * 8000, dtype=np.float32), 8000)
    assert silent["blocks"] == 21 and silent["above_absolute"] == silent["gated"] == 0 and silent["lra"] == 0.0
    assert silent["low_lufs"] == silent["high_lufs"] == silent["short_term_max"] == silent["momentary_max"] == -np.inf
    short = R.loudness_range(two_levels(-20.0, -20.0, seconds=1), 8000)  # 2 s: momentary blocks, no short-term one
    assert short["blocks"] == 0 and short["lra"] == 0.0 and short["short_term_max"] == -np.inf and np.isfinite(short["momentary_max"])
    e = np.arange(1.0, 8.0)
    assert np.array_equal(R.left_to_right(e, 4, 10), np.array([((e[k] + e[k + 1]) + e[k + 2]) + e[k + 3] for k in range(4)]) / 40.0)
    assert np.array_equal(R.left_to_right(e, 1, 10), e / 10.0) and R.left_to_right(e, 8, 10).size == 0
    assert R.block_count(30 * 800 - 1, 8000, 30) == 0 and R.block_count(30 * 800, 8000, 30) == 1 and R.block_count(31 * 800, 8000, 30) == 2


def test_percentile_picks():
    want = {1: (0, 0), 2: (0, 1), 10: (1, 9), 11: (1, 10), 100: (10, 94), 101: (10, 95)}
    for g, picks in want.items():
        assert R.percentile_indices(g) == picks, g
        # Tech 3342's own statement, 1-based with halves rounded up: round((g - 1) p / 100 + 1)
        assert picks == tuple(int(np.floor((g - 1) * p / 100.0 + 0.5)) for p in (10, 95)), g
    assert R.picks([4.0, 1.0]) == (float(R.L.lkfs(1.0)), float(R.L.lkfs(4.0)))


def test_true_peak_factor():
    lib = _capi.load_library()
    for fs, want in ((8000, 4), (16000, 4), (44100, 4), (95999, 4), (96000, 2), (192000, 2)):
        assert lib.l3ac_true_peak_factor(fs) == want == l3ac_amd.true_peak_factor(fs) == R.factor(fs), fs
    for fs in (7999, 192001, 0, -16000):
        assert lib.l3ac_true_peak_factor(fs) < 0 and b"sample_rate" in lib.l3ac_last_error(), fs
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.true_peak_factor(fs)
    tile = lib.l3ac_true_peak_tile()
    assert tile >= 64 and tile % 4 == 0


@pytest.mark.parametrize("fs", [8000, 96000])
def test_the_oversampler_is_the_resample_bank(fs):
    """The taps of the true-peak kernel come from the design behind l3ac_resample_bank: that bank for fs -> L fs holds L phases of 21 taps,
    each the fp32 rounding of the oracle's prototype."""
    lib = _capi.load_library()
    up = R.factor(fs)
    n = lib.l3ac_resample_bank(fs, up * fs, None, 0)
    ke = n // (4 * up)
    assert n == up * 4 * ke and ke >= 24
    bank = torch.zeros(n, dtype=torch.float32)
    assert lib.l3ac_resample_bank(fs, up * fs, bank.data_ptr(), n) == n
    _, k, taps = RS.polyphase_taps(fs, up * fs)
    assert k == 21
    rows = bank.view(up, 4, ke).numpy()
    for p in range(up):
        assert np.array_equal(rows[p, 0, :21], taps[p, ::-1].astype(np.float32)) and not rows[p, 0, 21:].any()
        for v in range(1, 4):  # the same taps behind v zeros
            assert np.array_equal(rows[p, v, v:v + 21], rows[p, 0, :21]) and not rows[p, v, :v].any()


def test_oracle_true_peak_of_the_quarter_rate_sine():
    """A sine at fs / 4 sampled 45 degrees off its crests: the samples reach 0.3536 of an amplitude of 0.5."""
    x = (0.5 * np.sin(2 * np.pi * 0.25 * np.arange(2000) + np.pi / 4)).astype(np.float32)
    o = R.true_peak(x, 16000)
    assert abs(o["peak"] - 0.35355) < 1e-5 and abs(o["true_peak"] - 0.5067) < 1e-4 and abs(np.abs(o["y"][400:-400]).max() - 0.5009) < 1e-4
    assert o["factor"] == 4 and o["y"].shape == (8000,)


BAD_RATES = (11025, 7990, 192010)


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, fs = 4096, 48000, 16000
    ok = (_capi.C.c_int32 * 2)(300, t)
    bad_lens = ((_capi.C.c_int32 * 2)(0, t), (_capi.C.c_int32 * 2)(300, t + 1))

    need = lib.l3ac_r128_scratch_bytes(2, t, fs)
    assert need == lib.l3ac_loudness_scratch_bytes(2, t, fs) > 0
    for kw in ((0, t, fs), (65536, t, fs), (2, 0, fs), (2, 1 << 31, fs)) + tuple((2, t, r) for r in BAD_RATES):
        assert lib.l3ac_r128_scratch_bytes(*kw) < 0 and lib.l3ac_last_error(), kw

    def series(audio=fake, stride=t, batch=2, t=t, lens=ok, fs=fs, window=30, lufs=fake, ms=None, en=None, blocks=None, scratch=fake, nbytes=need):
        return lib.l3ac_r128_series(audio, stride, batch, t, lens, fs, window, lufs, ms, en, blocks, scratch, nbytes, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=bad_lens[0]), dict(lens=bad_lens[1]), dict(stride=t - 1), dict(audio=None),
               dict(lufs=None), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=need - 1), dict(window=0), dict(window=601),
               dict(window=-1)) + tuple(dict(fs=r) for r in BAD_RATES):
        assert series(**kw) == -1 and lib.l3ac_last_error(), kw
    assert series(window=601) == -1 and b"window_steps" in lib.l3ac_last_error()
    assert series(nbytes=need - 1) == -1 and b"l3ac_r128_scratch_bytes" in lib.l3ac_last_error()
    assert series(lens=bad_lens[1]) == -1 and b"samples[1]" in lib.l3ac_last_error()
    assert series(fs=11025) == -1 and b"sample_rate" in lib.l3ac_last_error()

    def rng(audio=fake, stride=t, batch=2, t=t, lens=ok, fs=fs, stats=fake, counts=fake, scratch=fake, nbytes=need):
        return lib.l3ac_r128_range(audio, stride, batch, t, lens, fs, stats, counts, scratch, nbytes, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=bad_lens[0]), dict(lens=bad_lens[1]), dict(stride=t - 1), dict(audio=None),
               dict(stats=None), dict(counts=None), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=need - 1)) + tuple(dict(fs=r) for r in BAD_RATES):
        assert rng(**kw) == -1 and lib.l3ac_last_error(), kw
    assert rng(stride=t - 1) == -1 and b"stride" in lib.l3ac_last_error()
    # 16385 short-term blocks: refused on the lengths alone, whatever the scratch
    long_t = (16385 + 29) * 800
    assert rng(t=long_t, stride=long_t, lens=None, fs=8000, batch=1) == -1 and b"16385 short-term blocks" in lib.l3ac_last_error()
    assert rng(t=long_t, stride=long_t, lens=(_capi.C.c_int32 * 2)(800, long_t), fs=8000) == -1 and b"short-term blocks" in lib.l3ac_last_error()

    tp_need = lib.l3ac_true_peak_scratch_bytes(2, t, fs)
    assert tp_need > 0 and lib.l3ac_true_peak_scratch_bytes(2, 40 * t, fs) > tp_need
    for kw in ((0, t, fs), (65536, t, fs), (2, 0, fs), (2, 1 << 31, fs), (2, t, 7999), (2, t, 192001)):
        assert lib.l3ac_true_peak_scratch_bytes(*kw) < 0 and lib.l3ac_last_error(), kw
    assert lib.l3ac_true_peak_scratch_bytes(2, t, 11025) > 0  # the oversampler needs no whole step: any rate in range

    def peak(audio=fake, stride=t, batch=2, t=t, lens=ok, fs=fs, stats=fake, scratch=fake, nbytes=tp_need):
        return lib.l3ac_true_peak(audio, stride, batch, t, lens, fs, stats, scratch, nbytes, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=bad_lens[0]), dict(lens=bad_lens[1]), dict(stride=t - 1), dict(audio=None),
               dict(stats=None), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=tp_need - 1), dict(fs=7999), dict(fs=192001)):
        assert peak(**kw) == -1 and lib.l3ac_last_error(), kw
    assert peak(nbytes=tp_need - 1) == -1 and b"l3ac_true_peak_scratch_bytes" in lib.l3ac_last_error()
    assert peak(fs=7999) == -1 and b"sample_rate" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 48000)
    for rate in BAD_RATES + (0, -16000):  # parameters first, on CPU tensors
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.short_term_loudness(x, sample_rate=rate)
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.loudness_range(x, sample_rate=rate)
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.normalize_loudness(x, sample_rate=rate, peak="true")
    for rate in (7999, 192001, 0):
        with pytest.raises(ValueError, match="sample_rate"):
            l3ac_amd.true_peak(x, sample_rate=rate)
    for window in (0.0, 0.05, 0.45, 60.1, -3.0, float("nan"), float("inf"), "long", None):
        with pytest.raises(ValueError, match="window"):
            l3ac_amd.short_term_loudness(x, window=window)
    for mode in ("peak", "True", None, 1):
        with pytest.raises(ValueError, match="peak must be"):
            l3ac_amd.normalize_loudness(x, peak=mode)
    for call in (lambda: l3ac_amd.true_peak(x), lambda: l3ac_amd.true_peak(x.numpy(), 48000), lambda: l3ac_amd.true_peak(x, lengths=[0, 1]),
                 lambda: l3ac_amd.short_term_loudness(x), lambda: l3ac_amd.short_term_loudness(x, window=0.4, return_parts=True),
                 lambda: l3ac_amd.short_term_loudness(x, lengths=[1, 48001]), lambda: l3ac_amd.loudness_range(x),
                 lambda: l3ac_amd.loudness_range(x.numpy()), lambda: l3ac_amd.loudness_range(x, lengths=[1, 48001]),
                 lambda: l3ac_amd.normalize_loudness(x, peak="true"), lambda: l3ac_amd.normalize_loudness(x, peak="sample")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_evaluate_checks_before_any_device_work():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):  # the network is not on a GPU
        codec.evaluate(torch.zeros(1, 8000), r128=True)
    codec.config.sample_rate = 11025  # a rate the meter is not defined for: refused first
    try:
        with pytest.raises(ValueError, match="sample_rate"):
            codec.evaluate(torch.zeros(1, 8000), r128=True)
    finally:
        codec.config.sample_rate = 16000


def test_exports_and_abi():
    for name in ("true_peak", "true_peak_factor", "short_term_loudness", "loudness_range"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name)), name
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    lib = _capi.load_library()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        proto = re.search(rf"\b{name}\s*\(([^()]*)\)\s*;", code)
        params = [] if proto and proto.group(1).strip() == "void" else proto.group(1).split(",")
        assert len(params) == len(_capi.SIGNATURES[name][1]), name
    assert "DESIGN.md section 3.25" in header
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    assert "kernels/true_peak.hip" in build.SOURCES
    design = (REPO / "DESIGN.md").read_text()
    assert "3.25" in design and "true peak is out of scope" not in design
