"""Quality metrics without a GPU: the library's two fp32 tables against their fp64 designs, the frame count, the fp64 restatement
(tests/metrics_ref.py) against torch.stft, and that every unsupported parameter is refused — through the ABI and through Python — before
any device work."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import metrics_ref as M


def ulp32(v):
    """The spacing of fp32 at |v| (at least that of the smallest normal)."""
    return np.spacing(np.maximum(np.abs(v), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("n_fft", [16, 32, 64, 256, 1024, 2048])
def test_basis_is_the_fp64_design_rounded_once(n_fft):
    got = l3ac_amd.stft_basis(n_fft).double().numpy()
    want = M.basis_design(n_fft)
    assert got.shape == (n_fft + 2, n_fft)
    # one rounding to fp32 of a design whose own fp64 error (cos / sin / the products: a few 2^-53, absolute, entries <= 1) can move the
    # rounding by one step: within 1 fp32 ulp of the value, plus that absolute floor for the entries that are zeros of the cosine
    assert (np.abs(got - want) <= ulp32(want) + 1e-15).all()
    assert np.abs(got[[1, n_fft + 1]]).max() < 1e-15  # the sine rows of DC and Nyquist: sin(0), sin(pi) as fp64 gives it
    assert not got[:, 0].any()  # the periodic Hann starts at 0


@pytest.mark.parametrize("sr,n_fft,n_mels", [(16000, 16, 4), (16000, 32, 24), (16000, 64, 8), (16000, 256, 20), (16000, 512, 40), (16000, 1024, 80),
                                              (16000, 2048, 80), (44100, 1024, 128)])
def test_mel_weights_are_the_fp64_design_rounded_once(sr, n_fft, n_mels):
    got = l3ac_amd.mel_weights(sr, n_fft, n_mels).double().numpy()
    want = M.mel_design(sr, n_fft, n_mels)
    assert got.shape == (n_mels, n_fft // 2 + 1)
    # 1 fp32 ulp of the value; the triangle's difference f_k - p_m cancels, so the design itself carries an absolute error of about
    # 2^-52 * (sr / 2) / (filter width >= 1 Hz here) <= 2e-12, which decides entries at a triangle's foot
    assert (np.abs(got - want) <= ulp32(want) + 2e-12).all()
    assert (got >= 0).all() and got.max() <= 1.0
    empty = [m for m in range(n_mels) if not got[m].any()]
    if sr == 16000:  # the shapes of the GPU tests: (32, 8, 24) is the one with empty filters (narrower than a bin)
        assert len(empty) == (6 if (n_fft, n_mels) == (32, 24) else 0), empty
    for m in range(n_mels):  # each filter is one contiguous run of bins
        nz = np.flatnonzero(got[m])
        assert nz.size == 0 or nz[-1] - nz[0] + 1 == nz.size


def test_default_scales_have_no_empty_filter():
    for n_fft, hop, n_mels in l3ac_amd.DEFAULT_SCALES:
        assert l3ac_amd.mel_weights(16000, n_fft, n_mels).abs().sum(dim=1).min() > 0


def test_stft_frames():
    lib = _capi.load_library()
    for n, hop in [(1, 4), (3, 4), (4, 4), (5, 4), (31, 16), (32, 16), (33, 16), (8000, 512), (1 << 40, 4)]:
        assert lib.l3ac_stft_frames(n, hop) == 1 + n // hop == l3ac_amd.stft_frames(n, hop) == M.frames(n, hop)
    for n, hop in [(0, 4), (-1, 4), (5, 0), (5, -4)]:
        assert lib.l3ac_stft_frames(n, hop) < 0
        with pytest.raises(ValueError):
            l3ac_amd.stft_frames(n, hop)


@pytest.mark.parametrize("n_fft,hop,n", [(16, 4, 9), (64, 16, 33), (64, 64, 200), (256, 64, 1000), (2048, 512, 8000)])
def test_restatement_matches_torch_stft(n_fft, hop, n):
    g = torch.Generator().manual_seed(n)
    x = (0.1 * torch.randn(n, generator=g) + 0.3 * torch.sin(0.05 * torch.arange(n))).double()
    want = torch.stft(x, n_fft, hop, n_fft, torch.hann_window(n_fft, dtype=torch.float64), center=True, pad_mode="constant", onesided=True,
                      return_complex=True).t().numpy()
    got = M.stft_explicit(x.numpy(), n_fft, hop)
    assert got.shape == want.shape == (1 + n // hop, n_fft // 2 + 1)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # and the table form (the oracle of the GPU tests) on the fp64 design is the same thing
    table, _ = M.stft_ref(x.numpy(), n_fft, hop, M.basis_design(n_fft))
    assert np.abs(table - want).max() <= 1e-9 * np.abs(want).max()


BAD = [  # (sample_rate, n_fft, hop, n_mels)
    (16000, 8, 4, 4), (16000, 24, 4, 4), (16000, 2064, 512, 80), (16000, 4096, 512, 80), (16000, 0, 4, 4), (16000, -64, 16, 8),
    (16000, 64, 0, 8), (16000, 64, 2, 8), (16000, 64, 6, 8), (16000, 64, 68, 8), (16000, 64, 128, 8), (16000, 64, -16, 8),
    (16000, 64, 16, 0), (16000, 64, 16, 257), (16000, 64, 16, -1), (0, 64, 16, 8), (-16000, 64, 16, 8),
]


@pytest.mark.parametrize("sr,n_fft,hop,n_mels", BAD)
def test_unsupported_parameters_are_refused_by_the_abi(sr, n_fft, hop, n_mels):
    lib = _capi.load_library()
    bad_fft = not (16 <= n_fft <= 2048 and n_fft % 16 == 0)
    assert (lib.l3ac_stft_basis(n_fft, None, 0) < 0) == bad_fft
    assert (lib.l3ac_mel_weights(sr, n_fft, n_mels, None, 0) < 0) == (bad_fft or sr <= 0 or not 1 <= n_mels <= 256)
    assert lib.l3ac_mel_weights(sr, n_fft, n_mels, None, 0) < 0 or lib.l3ac_mel_scratch_bytes(2, 100, n_fft, hop, n_mels) < 0
    # the device entries: refused on their parameters alone (EINVAL = -1), whatever the pointers — nothing is launched or dereferenced
    fake = 4096
    lens = (_capi.C.c_int32 * 2)(50, 100)
    if sr > 0:
        assert lib.l3ac_log_mel(fake, 2, 100, 100, lens, n_fft, hop, fake, fake, n_mels, fake, fake, 1 << 30, None) == -1
        assert lib.l3ac_mel_distance(fake, 100, fake, 100, 2, 100, lens, n_fft, hop, n_mels, fake, fake, fake, fake, 1 << 30, None) == -1
        assert lib.l3ac_last_error()
        if 1 <= n_mels <= 256:
            assert lib.l3ac_stft(fake, 2, 100, 100, lens, n_fft, hop, fake, fake, fake, 1 << 30, None) == -1


def test_other_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake = 4096
    need = lib.l3ac_mel_scratch_bytes(2, 100, 64, 16, 8)
    assert need > 0
    ok_lens = (_capi.C.c_int32 * 2)(50, 100)
    for lens in ((_capi.C.c_int32 * 2)(0, 100), (_capi.C.c_int32 * 2)(50, 101)):
        assert lib.l3ac_stft(fake, 2, 100, 100, lens, 64, 16, fake, fake, fake, need, None) == -1
        assert lib.l3ac_signal_metrics(fake, 100, fake, 100, 2, 100, lens, fake, fake, 8, None) == -1
    assert lib.l3ac_stft(fake, 2, 100, 100, ok_lens, 64, 16, fake, fake, fake, need - 1, None) == -1 and b"scratch" in lib.l3ac_last_error()
    assert lib.l3ac_stft(fake, 2, 100, 99, ok_lens, 64, 16, fake, fake, fake, need, None) == -1  # row stride below the samples
    assert lib.l3ac_stft(None, 2, 100, 100, ok_lens, 64, 16, fake, fake, fake, need, None) == -1
    assert lib.l3ac_stft(fake, 0, 100, 100, None, 64, 16, fake, fake, fake, need, None) == -1
    assert lib.l3ac_signal_metrics(fake, 100, fake, 100, 2, 100, ok_lens, fake, None, 0, None) == -1  # lengths need their scratch
    assert lib.l3ac_signal_metrics(fake, 100, fake, 100, 2, 0, None, fake, None, 0, None) == -1
    assert lib.l3ac_mel_scratch_bytes(0, 100, 64, 16, 8) < 0 and lib.l3ac_mel_scratch_bytes(2, 0, 64, 16, 8) < 0


@pytest.mark.parametrize("sr,n_fft,hop,n_mels", BAD)
def test_unsupported_parameters_raise_in_python_before_any_device_work(sr, n_fft, hop, n_mels):
    """ValueError on CPU tensors, on a machine without a GPU: the parameters are checked before the tensors are looked at."""
    x = torch.zeros(2, 100)
    if sr > 0 and 1 <= n_mels <= 256:
        with pytest.raises(ValueError):
            l3ac_amd.stft(x, n_fft, hop)
    with pytest.raises(ValueError):
        l3ac_amd.log_mel(x, sr, n_fft, hop, n_mels)
    with pytest.raises(ValueError):
        l3ac_amd.mel_distance(x, x, sr, scales=[(64, 16, 8), (n_fft, hop, n_mels)])


def test_bad_scales_raise():
    x = torch.zeros(2, 100)
    for scales in ([], [(64, 16)], 5, [("a", 1, 2)]):
        with pytest.raises(ValueError):
            l3ac_amd.mel_distance(x, x, scales=scales)


def test_evaluate_refuses_scales_and_cpu_tensors_before_any_device_work():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.eval()
    x = torch.zeros(1, 8000)
    with pytest.raises(ValueError, match="n_fft"):
        codec.evaluate(x, scales=[(8, 4, 4)])
    with pytest.raises(RuntimeError, match="no CPU path"):  # the network is not on a GPU
        codec.evaluate(x)


def test_cpu_tensors_raise():
    x = torch.zeros(2, 100)
    for call in (lambda: l3ac_amd.stft(x, 64), lambda: l3ac_amd.log_mel(x, 16000, 64, 16, 8), lambda: l3ac_amd.mel_distance(x, x),
                 lambda: l3ac_amd.signal_metrics(x, x), lambda: l3ac_amd.stft(x.numpy(), 64)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_header_and_binding_agree_on_the_metrics_entries():
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    assert _capi.load_library().l3ac_abi_version() == 5


def test_table_sizes_follow_the_protocol():
    """A null or short buffer returns the length and writes nothing."""
    lib = _capi.load_library()
    assert lib.l3ac_stft_basis(64, None, 0) == 66 * 64 and lib.l3ac_mel_weights(16000, 64, 8, None, 0) == 8 * 33
    buf = torch.full((66 * 64,), 7.0)
    assert lib.l3ac_stft_basis(64, buf.data_ptr(), 66 * 64 - 1) == 66 * 64 and (buf == 7.0).all()
    assert lib.l3ac_stft_basis(64, buf.data_ptr(), 66 * 64) == 66 * 64 and torch.equal(buf.view(66, 64), l3ac_amd.stft_basis(64))
    # the scratch minimum does not depend on n_mels and grows with the batch
    assert lib.l3ac_mel_scratch_bytes(3, 1000, 256, 64, 20) == lib.l3ac_mel_scratch_bytes(3, 1000, 256, 64, 80)
    assert lib.l3ac_mel_scratch_bytes(4, 1000, 256, 64, 20) > lib.l3ac_mel_scratch_bytes(3, 1000, 256, 64, 20)
