"""Sample-rate conversion, host side (no GPU): the library's filter design and rate reduction against the fp64 restatement
(tests/resample_ref.py) and against scipy.signal.resample_poly, and argument checks that happen before any device work."""
import ctypes
import math

import numpy as np
import pytest

from l3ac_amd import _capi
from tests import resample_ref as R

STANDARD = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]
PAIRS = [(r, 16000) for r in STANDARD] + [(16000, r) for r in STANDARD] + [(44100, 48000), (48000, 44100)]


def lib_bank(a, b):
    """The library's bank as [up][4][KE] fp32, and its K."""
    lib = _capi.load_library()
    n = lib.l3ac_resample_bank(a, b, None, 0)
    assert n > 0, lib.l3ac_last_error()
    bank = np.zeros(n, np.float32)
    assert lib.l3ac_resample_bank(a, b, bank.ctypes.data_as(ctypes.c_void_p), n) == n
    up, _ = R.factors(a, b)
    ke = n // (4 * up)
    assert ke * 4 * up == n and ke % 4 == 0
    return bank.reshape(up, 4, ke)


def deinterleave(bank, a, b):
    """h[j] back out of variant 0 of the bank: phase j mod up, tap K - 1 - j div up."""
    up, _ = R.factors(a, b)
    h_len = 2 * 10 * max(R.factors(a, b)) + 1
    K = -(-h_len // up)
    j = np.arange(h_len)
    return bank[j % up, 0, K - 1 - j // up]


def ulp_distance(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 31) - ia, ia)  # sign-magnitude -> monotone integer line
    ib = np.where(ib < 0, np.int64(-2 ** 31) - ib, ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("a,b", PAIRS)
def test_bank_layout_and_design(a, b):
    """Every phase is stored four times, shifted by 0 .. 3 zeros, zero-padded; the taps are the fp64 design rounded once
    (within 1 ulp of the restatement: sin / i0 / the sum's order differ in the last fp64 bits)."""
    bank = lib_bank(a, b)
    up, down = R.factors(a, b)
    h, K, _ = R.polyphase_taps(a, b)
    ke = bank.shape[2]
    assert ke >= K + 3
    for v in range(4):
        assert np.array_equal(bank[:, v, v:v + K], bank[:, 0, :K])
        assert not bank[:, v, :v].any() and not bank[:, v, v + K:].any()
    got = deinterleave(bank, a, b)
    assert got.size == h.size
    assert ulp_distance(got, h.astype(np.float32)).max() <= 1
    # taps past the end of h (phases whose last tap does not exist) are zero
    idx = np.arange(up)[:, None] + (K - 1 - np.arange(K))[None, :] * up
    assert not bank[:, 0, :K][idx >= h.size].any()


@pytest.mark.parametrize("a,b", PAIRS)
def test_bank_matches_scipy_firwin(a, b):
    signal = pytest.importorskip("scipy.signal")
    up, down = R.factors(a, b)
    M = max(up, down)
    want = (signal.firwin(2 * 10 * M + 1, 1.0 / M, window=("kaiser", 5.0)) * up).astype(np.float32)
    got = deinterleave(lib_bank(a, b), a, b)
    d = ulp_distance(got, want)
    assert d.max() <= 1, (a, b, int(d.max()), int((d > 0).sum()))


@pytest.mark.parametrize("a,b", [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000), (11025, 16000),
                                 (22050, 16000), (44100, 48000)])
def test_reference_matches_scipy_resample_poly(a, b):
    signal = pytest.importorskip("scipy.signal")
    up, down = R.factors(a, b)
    half_len = 10 * max(up, down)
    rng = np.random.default_rng(a + 7 * b)
    for n in sorted({1, 2, 3, 7, 50, half_len // up // 2 + 1, half_len - 1, 1000, 16000}):
        x = rng.standard_normal((2, n))
        want = signal.resample_poly(x, up, down, axis=-1)
        got, _ = R.resample_ref(x, a, b)
        assert got.shape == want.shape, (n, got.shape, want.shape)
        assert np.abs(got - want).max() <= 1e-12, (a, b, n, np.abs(got - want).max())


def test_length_matches_scipy():
    signal = pytest.importorskip("scipy.signal")
    lib = _capi.load_library()
    for a, b in PAIRS + [(16000, 16000)]:
        up, down = R.factors(a, b)
        for n in (1, 2, 3, 159, 160, 441, 16000, 44100, 48000):
            want = signal.resample_poly(np.zeros(n), up, down).size
            assert lib.l3ac_resample_length(a, b, n) == want == R.out_length(a, b, n), (a, b, n)


def test_length_is_int64():
    """Ten minutes at 192 kHz -> 44.1 kHz: n_in * up passes 2^31."""
    lib = _capi.load_library()
    n = 192000 * 600
    up, down = R.factors(192000, 44100)
    assert n * up > 2 ** 31
    assert lib.l3ac_resample_length(192000, 44100, n) == -(-n * up // down)


def test_equal_rates_need_no_bank():
    lib = _capi.load_library()
    assert lib.l3ac_resample_bank(16000, 16000, None, 0) == 0
    assert lib.l3ac_resample_length(48000, 48000, 12345) == 12345


@pytest.mark.parametrize("a,b", [(0, 16000), (16000, 0), (-44100, 16000), (16000, -48000), (16000, 16001), (44100, 16001)])
def test_bad_rates_raise_before_device_work(a, b):
    import l3ac_amd

    lib = _capi.load_library()
    assert lib.l3ac_resample_length(a, b, 100) < 0
    assert lib.l3ac_resample_bank(a, b, None, 0) < 0
    # null buffers and no stream: the rate check comes first, nothing reaches the device
    assert lib.l3ac_resample(None, 1, 100, 100, a, b, None, None, 100, None) == -1
    assert b"resample" in lib.l3ac_last_error()
    with pytest.raises(ValueError):
        l3ac_amd.resample_length(a, b, 100)
    with pytest.raises(ValueError):
        R.factors(a, b)


@pytest.mark.parametrize("rate", [0, -48000, 16001, 15999])
def test_codec_keyword_rejects_bad_rates(rate):
    """encode_audio / decode_audio(sample_rate=...) check the rate before anything else touches the device."""
    import l3ac_amd

    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    with pytest.raises(ValueError):
        codec._rate(rate)
    assert codec._rate(None) is None and codec._rate(16000) is None and codec._rate(48000) == 48000


def test_largest_supported_factor():
    lib = _capi.load_library()
    assert math.gcd(1024, 1023) == 1
    assert lib.l3ac_resample_length(1023, 1024, 1023) == 1024  # max(up, down) = 1024: supported
    assert lib.l3ac_resample_length(1025, 1024, 1025) < 0      # 1025: not


def test_resample_has_no_cpu_path():
    import l3ac_amd
    import torch

    with pytest.raises(RuntimeError, match="no CPU path"):
        l3ac_amd.resample(torch.zeros(1, 100), 48000, 16000)
