"""The coherence measures without a GPU: the SII band table, the exports and the ABI, every parameter refusal before
any device work, and the fp64 oracle of tests/coherence_ref.py against a plain numpy.fft restatement of CSII and on inputs whose answer is
known."""
import ctypes as C
import functools
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import coherence_ref as R
from tests.lpc_ref import add_noise, resonator

REPO = Path(__file__).resolve().parents[1]
EINVAL = -1
FS = 16000
VALUES = ("csii", "csii_high", "csii_mid", "csii_low")


@functools.lru_cache(maxsize=None)
def twiddles(n_fft):
    out = np.zeros(n_fft, dtype=np.float64)
    assert _capi.load_library().l3ac_bands_twiddles(n_fft, out.ctypes.data, n_fft) == n_fft
    return out.reshape(n_fft // 2, 2)


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------
def test_sii_bands_is_the_standards_table():
    centre, width, imp = l3ac_amd.sii_bands()
    assert all(v.dtype == torch.float64 and v.shape == (21,) and not v.is_cuda for v in (centre, width, imp))
    assert tuple(centre.tolist()) == R.CENTRES and tuple(imp.tolist()) == R.IMPORTANCE
    assert tuple(width.tolist()) == tuple(u - l for u, l in zip(R.UPPER, R.LOWER))
    assert R.CENTRES[0] == 150.0 and R.CENTRES[-1] == 8500.0 and R.LOWER[0] == 100.0 and R.UPPER[-1] == 9500.0 and R.UPPER[:-1] == R.LOWER[1:]
    assert R.IMPORTANCE[:3] == (0.0103, 0.0261, 0.0419) and R.IMPORTANCE[3:17] == (0.0577,) * 14 and R.IMPORTANCE[17:] == (0.0460, 0.0343, 0.0226, 0.0110)
    assert abs(float(imp.sum()) - 1.0) <= 1e-12
    for fs, keep in ((16000, 20), (8000, 16), (48000, 21), (19000, 21), (18999, 20)):
        got = l3ac_amd.sii_bands(fs)
        assert all(len(v) == keep for v in got) and tuple(got[0].tolist()) == R.CENTRES[:keep] == R.sii_table(fs)[0], fs
    w = l3ac_amd.band_weights(FS, 1024, l3ac_amd.sii_bands(FS)[:2])  # every default band has weights at the default transform
    assert w.shape == (20, 512) and (w.sum(dim=1) > 0).all()
    assert l3ac_amd.band_weights(8000, 512, l3ac_amd.sii_bands(8000)[:2]).shape == (16, 256)


def test_exports_header_and_abi_version():
    for name in ("coherence", "csii", "sii_bands"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in ("l3ac_sii_bands", "l3ac_coherence_scratch_bytes", "l3ac_coherence", "l3ac_csii"):
        proto = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", code)
        assert proto and len(proto.group(1).split(",")) == len(_capi.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert "DESIGN.md section 3.23" in header
    p = inspect.signature(l3ac_amd.L3AC.evaluate).parameters
    assert "coherence" in p and p["coherence"].default is False
    source = (REPO / "l3ac_amd" / "csrc" / "kernels" / "coherence.hip").read_text()
    assert "#pragma clang fp contract(off)" in source and not re.search(r"\batomic[A-Z]\w*\s*\(|__hip_atomic|__atomic_", source)  # no atomics
    shared = (REPO / "l3ac_amd" / "csrc" / "kernels" / "fft_f64.hpp").read_text()
    assert "#pragma clang fp contract(off)" in shared
    for user in ("bands.hip", "coherence.hip"):
        assert '#include "fft_f64.hpp"' in (REPO / "l3ac_amd" / "csrc" / "kernels" / user).read_text()
    assert "kernels/coherence.hip" in (REPO / "l3ac_amd" / "build.py").read_text()


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------
def test_scratch_sizes():
    lib = _capi.load_library()
    up = lambda v: 256 * -(-v // 256)
    for b, t, n, hop, n_fft in ((1, 1, 5, 1, 16), (3, 4000, 480, 120, 1024), (65, 500, 33, 1, 64), (2, 16384 * 2 + 98, 100, 2, 256),
                                (2, 9000, 2048, 512, 4096), (256, 16000, 480, 120, 1024)):
        f, h = R.n_frames(t, n, hop), n_fft // 2
        chunks = -(-f // R.chunk_frames(n_fft))
        want = up(4 * b) + up(8 * b * f) + up(4 * b * f) + up(20 * b) + up(128 * b * h) + up(128 * b * chunks * h)
        assert lib.l3ac_coherence_scratch_bytes(b, t, n, hop, n_fft) == want, (b, t, n, hop, n_fft)
    assert lib.l3ac_coherence_scratch_bytes(256, 16000, 480, 120, 1024) < 128 << 20  # 256 pairs of 1 s: below 128 MiB
    assert lib.l3ac_coherence_scratch_bytes(2, 16384 * 2 + 100, 100, 2, 256) < 0 and b"16385 frames" in lib.l3ac_last_error()
    for bad, word in (((0, 100, 64, 16, 128), b"batch"), ((65536, 100, 64, 16, 128), b"batch"), ((1, 0, 64, 16, 128), b"max_samples"),
                      ((1, 100, 1, 16, 128), b"frame"), ((1, 100, 2049, 16, 4096), b"frame"), ((1, 100, 64, 0, 128), b"hop"),
                      ((1, 100, 64, -2, 128), b"hop"), ((1, 100, 64, 16, 8), b"n_fft"), ((1, 100, 64, 16, 8192), b"n_fft"),
                      ((1, 100, 64, 16, 100), b"n_fft"), ((1, 100, 65, 16, 64), b"n_fft")):
        assert lib.l3ac_coherence_scratch_bytes(*bad) < 0 and word in lib.l3ac_last_error(), bad


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, n, hop, n_fft, nb = 4096, 3000, 240, 60, 512, 20
    need = lib.l3ac_coherence_scratch_bytes(2, t, n, hop, n_fft)
    ok = (C.c_int32 * 2)(3000, 100)
    geometry = (dict(n=1), dict(n=2049, n_fft=4096), dict(n=513), dict(hop=0), dict(hop=-1), dict(n_fft=8), dict(n_fft=8192), dict(n_fft=768),
                dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=(C.c_int32 * 2)(0, 5)), dict(lens=(C.c_int32 * 2)(3000, 3001)),
                dict(lens=(C.c_int32 * 2)(-7, 5)), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=0), dict(nbytes=need - 1),
                dict(rs=t - 1), dict(es=t - 1), dict(ref=None), dict(est=None), dict(tw=None), dict(ref=fake + 2), dict(tw=fake + 4), dict(sums=fake + 4),
                dict(counts=fake + 2), dict(t=16384 * 2 + 100, n=100, hop=2, rs=40000, es=40000, nbytes=1 << 40))

    def coherence(ref=fake, rs=t, est=fake, es=t, batch=2, t=t, lens=ok, n=n, hop=hop, n_fft=n_fft, window=fake, tw=fake, msc=fake, sums=None,
                  counts=fake, scratch=fake, nbytes=need):
        return lib.l3ac_coherence(ref, rs, est, es, batch, t, lens, n, hop, n_fft, window, tw, msc, None, sums, counts, None, None, scratch, nbytes, None)

    def csii(ref=fake, rs=t, est=fake, es=t, batch=2, t=t, lens=ok, n=n, hop=hop, n_fft=n_fft, window=fake, tw=fake, wt=fake, imp=fake, nb=nb, out=fake,
             sums=None, counts=fake, scratch=fake, nbytes=need):
        return lib.l3ac_csii(ref, rs, est, es, batch, t, lens, n, hop, n_fft, window, tw, wt, imp, nb, out, counts, None, None, None, sums, scratch,
                             nbytes, None)

    # refused on the arguments alone, whatever the pointers: nothing is launched or dereferenced
    for kw in geometry:
        assert coherence(**kw) == EINVAL and lib.l3ac_last_error(), kw
        assert csii(**kw) == EINVAL and lib.l3ac_last_error(), kw
    for kw in (dict(wt=None), dict(imp=None), dict(out=None), dict(nb=0), dict(nb=1), dict(nb=65), dict(wt=fake + 4), dict(out=fake + 4)):
        assert csii(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert coherence(n=513) == EINVAL and b"coherence: n_fft 512 is below the frame 513" in lib.l3ac_last_error()
    assert csii(n_fft=768) == EINVAL and b"csii: n_fft 768 is not a power of two" in lib.l3ac_last_error()
    assert csii(nb=65) == EINVAL and b"bands" in lib.l3ac_last_error()
    assert coherence(nbytes=need - 1) == EINVAL and b"l3ac_coherence_scratch_bytes" in lib.l3ac_last_error()
    assert coherence(lens=(C.c_int32 * 2)(3000, 0)) == EINVAL and b"samples[1]" in lib.l3ac_last_error()
    assert coherence(tw=fake + 4) == EINVAL and b"aligned" in lib.l3ac_last_error()
    assert csii(t=16384 * 2 + 100, n=100, hop=2, rs=40000, es=40000, nbytes=1 << 40) == EINVAL and b"frames" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 3000)
    calls = (lambda **kw: l3ac_amd.coherence(x, x, **kw), lambda **kw: l3ac_amd.csii(x, x, **kw))
    for kw in (dict(frame=1), dict(frame=2049), dict(frame=513, n_fft=512), dict(hop=0), dict(n_fft=8), dict(n_fft=8192), dict(n_fft=1000),
               dict(sample_rate=7999), dict(sample_rate=192001), dict(window="hamming"), dict(window=None), dict(frame="long"),
               dict(lengths=[0, 5]), dict(lengths=[3001, 5]), dict(lengths=[5]), dict(lengths=[2.5, 5])):
        for call in calls:
            with pytest.raises(ValueError):  # the parameter first, on CPU tensors
                call(**kw)
    with pytest.raises(ValueError, match="n_fft 1000 is not a power of two"):
        l3ac_amd.coherence(x, x, n_fft=1000)
    with pytest.raises(ValueError, match="window"):
        l3ac_amd.csii(x, x, window="hamming")
    two = ([1000.0, 2000.0], [200.0, 300.0])
    for bands in (two, two + ([0.5],), two + ([0.5, 0.0],), two + ([0.5, -1.0],), two + ([0.5, float("nan")],), two + ([0.5, float("inf")],), 7,
                  ([1000.0], [200.0], [1.0]), ([100.0, 9000.0], [70.0, 70.0], [0.5, 0.5]), ([100.0, 200.0], [70.0, 0.0], [0.5, 0.5]),
                  ([100.0] * 65, [70.0] * 65, [0.5] * 65)):
        with pytest.raises(ValueError):
            l3ac_amd.csii(x, x, bands=bands)
    with pytest.raises(ValueError, match="importance"):
        l3ac_amd.csii(x, x, bands=two + ([0.5, 0.0],))
    with pytest.raises(ValueError, match="centre_hz"):  # all 21 bands do not fit below 4 kHz
        l3ac_amd.csii(x, x, sample_rate=8000, bands=l3ac_amd.sii_bands())
    with pytest.raises(ValueError, match="differ in shape"):
        l3ac_amd.coherence(x, torch.zeros(2, 3001))
    with pytest.raises(ValueError, match="differ in shape"):
        l3ac_amd.csii(x, torch.zeros(2, 3001))
    with pytest.raises(ValueError, match="batch, samples"):
        l3ac_amd.coherence(torch.zeros(3000), torch.zeros(3000))
    long = torch.zeros(1, 16384 * 2 + 100)
    for call in (l3ac_amd.coherence, l3ac_amd.csii):
        with pytest.raises(ValueError, match="16385 frames"):
            call(long, long, frame=100, hop=2)
    for call in (lambda: l3ac_amd.coherence(x, x), lambda: l3ac_amd.csii(x, x), lambda: l3ac_amd.coherence(x.numpy(), x.numpy()),
                 lambda: l3ac_amd.csii(x, x, lengths=[3000, 100], return_bands=True, window="rect"),
                 lambda: l3ac_amd.csii(x, x, sample_rate=8000), lambda: l3ac_amd.coherence(x, x, n_fft=4096, return_sums=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_evaluate_checks_before_any_device_work():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):  # the network is not on a GPU
        codec.evaluate(torch.zeros(1, 8000), coherence=True)
    with pytest.raises(ValueError, match=r"evaluate\(coherence=True\).*16384 frames"):  # a recording too long for a pair: refused first
        codec.evaluate(torch.zeros(1, 480 + 16384 * 120), coherence=True)
    codec.config.sample_rate = 96000  # the default frame of 30 ms does not fit this rate: refused first
    try:
        with pytest.raises(ValueError, match="frame 2880 outside"):
            codec.evaluate(torch.zeros(1, 8000), coherence=True)
    finally:
        codec.config.sample_rate = 16000


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def swept_clip():
    """1 s at 16 kHz of the resonator under the envelope that sweeps 34 dB."""
    return (resonator(FS, FS, seed=7).astype(np.float64) * R.envelope(FS)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def swept_pair(snr_db):
    ref = swept_clip()
    est = add_noise(ref, snr_db, seed=int(snr_db) + 1)
    n, hop, n_fft = 480, 120, 1024
    centre, width, imp = R.sii_table(FS)
    w = l3ac_amd.band_weights(FS, n_fft, (centre, width)).numpy()
    return R.pair(ref, est, n, hop, n_fft, twiddles(n_fft), w, imp), R.plain_csii(ref, est, n, hop, n_fft, w, imp)


def test_oracle_is_plain_numpy_csii_on_swept_speech_like_clips():
    """The stated orders against numpy.fft and numpy.sum, and the inputs' sanity: every class occurs, every value lies strictly inside (0, 1),
    and csii rises with the SNR."""
    previous = 0.0
    for snr_db in (0.0, 5.0, 15.0, 30.0):
        got, plain = swept_pair(snr_db)
        assert got["frames"] == 130 and int(got["level_frames"].sum()) == 130
        assert (got["level_frames"][:3] >= 2).all(), got["level_frames"]
        assert got["level_frames"].tolist() == plain["level_frames"].tolist()
        for key in VALUES + ("i3", "intelligibility"):
            assert abs(got[key] - plain[key]) <= 1e-9, (key, snr_db, got[key], plain[key])
        for key in VALUES:
            assert 0.0 < got[key] < 1.0, (key, snr_db, got[key])
        assert got["csii"] > previous, (snr_db, got["csii"], previous)
        previous = got["csii"]
        assert (got["msc"] >= 0).all() and (got["msc"] <= 1).all() and got["msc_levels"].shape == (4, 512)
        print(f"snr {snr_db:4.1f} dB: frames {got['level_frames'].tolist()}, csii {got['csii']:.4f}, high {got['csii_high']:.4f}, mid "
              f"{got['csii_mid']:.4f}, low {got['csii_low']:.4f}, i3 {got['i3']:.4f}")


def test_oracle_exact_cases():
    ref = swept_clip()[:6000]
    n, hop, n_fft = 480, 120, 1024
    centre, width, imp = R.sii_table(FS)
    w = l3ac_amd.band_weights(FS, n_fft, (centre, width)).numpy()
    tw = twiddles(n_fft)
    for est in (ref, -2.0 * ref, 0.25 * ref):  # a power-of-two multiple of either sign: g == 1 exactly wherever Sxx > 0
        got = R.pair(ref, est.astype(np.float32), n, hop, n_fft, tw, w, imp)
        assert (got["level_frames"][:3] >= 2).all()
        assert (got["msc"][got["sums"][:, 0].sum(axis=0) > 0] == 1.0).all()
        assert all(got[key] == 1.0 for key in VALUES) and (got["band_distortion"] == 0.0).all()
        assert got["i3"] == (-3.47 + 1.84) + 9.99
    zero = R.pair(ref, np.zeros_like(ref), n, hop, n_fft, tw, w, imp)
    assert all(zero[key] == 0.0 for key in VALUES) and (zero["msc"] == 0.0).all() and zero["i3"] == -3.47
    silent = R.pair(np.zeros_like(ref), ref, n, hop, n_fft, tw, w, imp)  # an all-zero reference: every frame below
    assert silent["level_frames"].tolist() == [0, 0, 0, silent["frames"]] and (silent["frame_class"] == 3).all()
    assert all(np.isnan(silent[key]) for key in ("csii_high", "csii_mid", "csii_low", "i3", "intelligibility")) and silent["csii"] == 0.0
    one = R.pair(ref[:n + hop - 1], ref[:n + hop - 1], n, hop, n_fft, tw, w, imp)  # one frame: coherent with anything, so no value
    assert one["frames"] == 1 and all(np.isnan(one[key]) for key in VALUES) and np.isnan(one["msc"]).all()
    none = R.pair(ref[:n - 1], ref[:n - 1], n, hop, n_fft, tw, w, imp)
    assert none["frames"] == 0 and np.isnan(none["csii"]) and none["level_frames"].tolist() == [0, 0, 0, 0]


def test_oracle_sum_order_is_chunks_of_four_groups():
    assert [R.chunk_frames(v) for v in (16, 256, 512, 1024, 2048, 4096)] == [64, 64, 32, 32, 16, 8]
    rng = np.random.default_rng(3)
    prod = rng.standard_normal((70, 4, 8))
    cls = rng.integers(0, 4, 70).astype(np.int32)
    got = R.class_sums(prod, cls, 16)
    for c in range(4):
        first, second = np.zeros((4, 8)), np.zeros((4, 8))
        for t in range(64):
            first = first + np.where(cls[t] == c, prod[t], 0.0)  # adding +0 for the other classes' frames changes no bit
        for t in range(64, 70):
            second = second + np.where(cls[t] == c, prod[t], 0.0)
        assert np.array_equal((np.zeros((4, 8)) + first) + second, got[c])
