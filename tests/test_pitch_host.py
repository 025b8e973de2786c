"""Pitch without a GPU: the frame geometry against the oracle (tests/pitch_ref.py) at its edges, every bad argument refused — through the
ABI with pointers that are never dereferenced and through Python on CPU tensors — before any device work, the exports and the header, and
the oracle itself on signals whose period is known."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import pitch_ref as R

C = _capi.C
DEFAULTS = (60.0, 500.0, -1, -1)  # fmin, fmax, window, hop as the ABI takes them


def abi_lags(fs, fmin=60.0, fmax=500.0, window=-1, hop=-1):
    out = (C.c_int32 * 5)()
    rc = _capi.load_library().l3ac_pitch_lags(fs, fmin, fmax, window, hop, out)
    return rc, tuple(out)


@pytest.mark.parametrize("kw", [dict(fs=16000), dict(fs=8000), dict(fs=48000), dict(fs=44100, fmin=55.0, fmax=880.0), dict(fs=16000, fmin=64.0, fmax=400.0),
                                dict(fs=16000, window=100, hop=77), dict(fs=22050, fmin=70.0, fmax=5512.5), dict(fs=8000, fmin=3.9, fmax=2000.0, window=1)])
def test_lags_follow_the_specification(kw):
    g = R.lags(kw["fs"], kw.get("fmin", 60.0), kw.get("fmax", 500.0), kw.get("hop"), kw.get("window"))
    rc, out = abi_lags(kw["fs"], kw.get("fmin", 60.0), kw.get("fmax", 500.0), kw.get("window", -1), kw.get("hop", -1))
    assert rc == 0 and out == (g["tau_min"], g["tau_max"], g["W"], g["hop"], g["span"]), (out, g)
    py = l3ac_amd.pitch_lags(kw["fs"], kw.get("fmin", 60.0), kw.get("fmax", 500.0), hop=kw.get("hop"), window=kw.get("window"))
    assert tuple(py[k] for k in ("tau_min", "tau_max", "window", "hop", "span")) == out and all(type(v) is int for v in py.values())


def test_default_geometry():
    assert l3ac_amd.pitch_lags() == dict(tau_min=32, tau_max=267, window=267, hop=160, span=535)
    assert l3ac_amd.pitch_lags(8000) == dict(tau_min=16, tau_max=134, window=134, hop=80, span=269)
    assert abs(R.beta(R.lags(8000)) - 1.6e-5) < 1e-6 and abs(R.beta(R.lags(16000)) - 3.2e-5) < 1e-6  # the figures of DESIGN.md 3.15


def test_frame_count_at_its_edges():
    lib = _capi.load_library()
    for fs, window, hop in ((16000, None, None), (8000, None, None), (16000, 100, 77), (8000, 50, 1000)):
        g = R.lags(fs, window=window, hop=hop)
        span, h = g["span"], g["hop"]
        for n, f in ((0, 0), (1, 0), (span - 1, 0), (span, 1), (span + h - 1, 1), (span + h, 2), (span + 9 * h - 1, 9), (span + 9 * h, 10)):
            got = lib.l3ac_pitch_frames(n, fs, 60.0, 500.0, -1 if window is None else window, -1 if hop is None else hop)
            assert got == f == R.frames(n, g) == l3ac_amd.pitch_frames(n, fs, hop=hop, window=window), (fs, window, hop, n)
    assert lib.l3ac_pitch_frames(1 << 40, 16000, *DEFAULTS) == 1 + ((1 << 40) - 535) // 160
    assert lib.l3ac_pitch_frames(-1, 16000, *DEFAULTS) < 0 and b"samples" in lib.l3ac_last_error()
    with pytest.raises(ValueError, match="samples"):
        l3ac_amd.pitch_frames(-1)


# what the specification does not support -> a word of the message.  (fmin < fmax gives tau_max > tau_min in exact arithmetic; the two
# quotients can only round together for neighbouring doubles: 8000 / nextafter(8000 / 33, 0) rounds to 33.)
BAD_PARAMS = [(dict(fs=7999), "sample_rate"), (dict(fs=192001), "sample_rate"), (dict(fs=0), "sample_rate"), (dict(fmin=500.0, fmax=500.0), "fmin"),
              (dict(fmin=600.0, fmax=500.0), "fmin"), (dict(fmin=0.0), "fmin"), (dict(fmin=-60.0), "fmin"), (dict(fmin=math.nan), "fmin"),
              (dict(fmax=math.nan), "fmin"), (dict(fmax=math.inf), "fmin"), (dict(fmax=4000.5), "fmax"), (dict(fs=8000, fmax=2001.0), "fmax"),
              (dict(fs=8000, fmin=math.nextafter(8000 / 33, 0.0), fmax=8000 / 33), "lag range"), (dict(hop=0), "hop"), (dict(hop=-2), "hop"), (dict(window=0), "window"),
              (dict(window=-7), "window"), (dict(fs=192000), "span"), (dict(window=4000 - 268 + 1), "span"), (dict(fmin=1e-9), "span"),
              (dict(fs=48000, fmin=12.0), "span")]


@pytest.mark.parametrize("kw,word", BAD_PARAMS)
def test_unsupported_parameters_are_refused_by_the_abi(kw, word):
    lib = _capi.load_library()
    args = (kw.get("fs", 16000), kw.get("fmin", 60.0), kw.get("fmax", 500.0), kw.get("window", -1), kw.get("hop", -1))
    rc, _ = abi_lags(*args)
    assert rc == -1 and word.encode() in lib.l3ac_last_error(), lib.l3ac_last_error()
    assert lib.l3ac_pitch_frames(16000, *args) < 0 and lib.l3ac_pitch_scratch_bytes(2, 16000, *args) < 0
    fake = 4096
    assert lib.l3ac_pitch(fake, 16000, 2, 16000, None, *args, 0.1, fake, fake, fake, None, None, fake, 1 << 20, None) == -1
    assert word.encode() in lib.l3ac_last_error()


def test_the_cap_on_span_is_exact():
    assert abi_lags(16000, window=4000 - 268)[0] == 0 and abi_lags(16000, window=4000 - 268)[1][4] == 4000
    assert abi_lags(16000, window=4000 - 268 + 1)[0] == -1
    assert abi_lags(48000, fmin=60.0, fmax=500.0)[1] == (96, 800, 800, 480, 1601)  # the defaults fit at 48 kHz


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, fs = 4096, 16000, 16000
    need = lib.l3ac_pitch_scratch_bytes(2, t, fs, *DEFAULTS)
    assert need > 0 and lib.l3ac_pitch_scratch_bytes(100, t, fs, *DEFAULTS) > need
    for kw in ((0, t), (65536, t), (2, 0), (2, 1 << 31)):
        assert lib.l3ac_pitch_scratch_bytes(*kw, fs, *DEFAULTS) < 0 and lib.l3ac_last_error(), kw
    ok = (C.c_int32 * 2)(300, t)

    def call(audio=fake, stride=t, batch=2, t=t, lens=ok, thr=0.1, f0=fake, voiced=fake, aper=fake, cmnd=None, frames=None, scratch=fake, nbytes=need):
        return lib.l3ac_pitch(audio, stride, batch, t, lens, fs, *DEFAULTS, thr, f0, voiced, aper, cmnd, frames, scratch, nbytes, None)

    # refused on the arguments alone (EINVAL = -1), whatever the pointers: nothing is launched or dereferenced
    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(lens=(C.c_int32 * 2)(0, t)), dict(lens=(C.c_int32 * 2)(-5, t)),
               dict(lens=(C.c_int32 * 2)(300, t + 1)), dict(stride=t - 1), dict(audio=None), dict(f0=None), dict(voiced=None), dict(aper=None),
               dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=need - 1), dict(thr=0.0), dict(thr=1.0), dict(thr=-0.1), dict(thr=1.5),
               dict(thr=math.nan)):
        assert call(**kw) == -1 and lib.l3ac_last_error(), kw
    assert call(nbytes=need - 1) == -1 and b"scratch" in lib.l3ac_last_error()
    assert call(stride=t - 1) == -1 and b"stride" in lib.l3ac_last_error()
    assert call(thr=1.0) == -1 and b"threshold" in lib.l3ac_last_error()
    assert call(lens=(C.c_int32 * 2)(300, -1)) == -1 and b"samples[1]" in lib.l3ac_last_error()

    def compare(f0r=fake, vr=fake, f0e=fake, ve=fake, batch=2, frames_max=50, frames=(C.c_int32 * 2)(0, 50), out=fake, counts=fake):
        return lib.l3ac_pitch_metrics(f0r, vr, f0e, ve, batch, frames_max, frames, out, counts, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(frames_max=-1), dict(frames_max=1 << 31), dict(frames=(C.c_int32 * 2)(-1, 50)),
               dict(frames=(C.c_int32 * 2)(0, 51)), dict(f0r=None), dict(vr=None), dict(f0e=None), dict(ve=None), dict(out=None), dict(counts=None)):
        assert compare(**kw) == -1 and lib.l3ac_last_error(), kw
    assert compare(frames=(C.c_int32 * 2)(0, 51)) == -1 and b"frames[1]" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 16000)
    for kw, word in BAD_PARAMS:
        kw = {("sample_rate" if k == "fs" else k): v for k, v in kw.items()}
        for call in (lambda: l3ac_amd.pitch(x, **kw), lambda: l3ac_amd.pitch_metrics(x, x, **kw),
                     lambda: l3ac_amd.pitch_lags(**kw), lambda: l3ac_amd.pitch_frames(16000, **kw)):
            with pytest.raises(ValueError, match=word):  # parameters first, on CPU tensors
                call()
    for thr in (0.0, 1.0, -0.1, 1.5, math.nan, "low"):
        with pytest.raises(ValueError, match="threshold"):
            l3ac_amd.pitch(x, threshold=thr)
        with pytest.raises(ValueError, match="threshold"):
            l3ac_amd.pitch_metrics(x, x, threshold=thr)
    with pytest.raises(ValueError):
        l3ac_amd.pitch(x, sample_rate="fast")
    for call in (lambda: l3ac_amd.pitch(x), lambda: l3ac_amd.pitch(x.numpy()), lambda: l3ac_amd.pitch(x, lengths=[-1, 5]),
                 lambda: l3ac_amd.pitch_metrics(x, x), lambda: l3ac_amd.pitch_metrics(x, x, lengths=[1, 16001])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_evaluate_checks_before_any_device_work():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):  # the network is not on a GPU
        codec.evaluate(torch.zeros(1, 8000), pitch=True)
    codec.config.sample_rate = 192000  # the default parameters do not fit this rate: refused first
    try:
        with pytest.raises(ValueError, match="span"):
            codec.evaluate(torch.zeros(1, 8000), pitch=True)
    finally:
        codec.config.sample_rate = 16000


def test_exports_and_abi_version():
    for name in ("pitch", "pitch_metrics", "pitch_frames", "pitch_lags"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5


# ---- the oracle on known periods --------------------------------------------------------------------------------------------------------------
def test_oracle_reads_a_sine():
    """200 Hz at 16 kHz: a period of exactly 80 samples."""
    x = (0.5 * np.sin(2 * np.pi * 200.0 * np.arange(4000) / 16000.0)).astype(np.float32)
    o = R.oracle(x, 16000)
    assert len(o["f0"]) == R.frames(4000, o["g"]) == 22 and o["robust"].all()
    assert (o["tau"] == 80).all() and (o["voiced"] == 1).all() and np.abs(o["f0"] / 200.0 - 1).max() <= 1e-3
    assert (o["aperiodicity"] < 1e-6).all() and (o["cmnd"][:, 0] == 1.0).all()


def test_oracle_on_silence_noise_and_an_impulse_train():
    g = R.lags(8000)
    o = R.oracle(np.zeros(1000, dtype=np.float32), 8000)
    assert (o["tau"] == g["tau_min"]).all() and (o["voiced"] == 0).all() and (o["aperiodicity"] == 1.0).all() and (o["cmnd"] == 1.0).all()
    assert (o["f0"] == 8000 / g["tau_min"]).all()
    noise = R.oracle((0.1 * np.random.default_rng(5).standard_normal(2000)).astype(np.float32), 8000)
    assert (noise["voiced"] == 0).all() and (noise["aperiodicity"] > 0.3).all()
    x = np.zeros(2000, dtype=np.float32)
    x[::50] = 1.0  # 160 Hz
    train = R.oracle(x, 8000)
    assert (train["tau"] == 50).all() and (train["voiced"] == 1).all() and (np.abs(train["f0"] / 160.0 - 1) < 1e-3).all() and (train["aperiodicity"] == 0.0).all()
    assert R.oracle(np.zeros(g["span"] - 1, dtype=np.float32), 8000)["f0"].shape == (0,)


def test_pick_from_cmnd_restates_the_pick():
    g = R.lags(16000)
    c = np.full(g["T"] + 1, 0.9)
    c[100:104] = (0.5, 0.09, 0.05, 0.07)  # the first lag below the threshold is 101; the descent stops at 102
    c[200] = 0.01  # a deeper minimum later is not looked at
    star, voiced, f0, ap = R.pick_from_cmnd(c, g)
    shift = 0.5 * (0.09 - 0.07) / (0.09 - 2 * 0.05 + 0.07)
    assert (star, voiced, ap) == (102, 1, 0.05) and f0 == 16000 / (102 + shift)
    c[:] = 0.9
    c[50], c[150] = 0.3, 0.3  # unvoiced: the first of two equal minima
    assert R.pick_from_cmnd(c, g)[:2] == (50, 0)
    c[:] = 0.9
    c[g["tau_max"]] = 0.01  # the last lag: the parabola reads lag T
    assert R.pick_from_cmnd(c, g)[:2] == (g["tau_max"], 1)
    assert R.robust(c, np.ones_like(c), 1e-5, g) and not R.robust(np.where(c == 0.01, 0.1 - 1e-7, c), np.ones_like(c), 1e-5, g)


def test_oracle_metrics():
    f_ref = np.array([100.0, 100.0, 100.0, 100.0, 100.0, 100.0])
    f_est = np.array([100.0, 200.0, 121.0, 119.0, 100.0, 100.0])
    v_ref, v_est = np.array([1, 1, 1, 1, 0, 1]), np.array([1, 1, 1, 1, 1, 0])
    m = R.metrics(f_ref, v_ref, f_est, v_est, 6)
    assert (m["frames"], m["voiced_reference"], m["voiced_estimate"], m["voiced_both"]) == (6, 5, 5, 4)
    assert m["vde"] == 2 / 6 and m["gpe"] == 2 / 4 and m["ffe"] == 4 / 6
    want = math.sqrt((1200.0 ** 2 + (1200 * math.log2(1.21)) ** 2 + (1200 * math.log2(1.19)) ** 2) / 4)
    assert abs(m["f0_rmse_cents"] / want - 1) < 1e-14
    empty = R.metrics(f_ref, v_ref, f_est, v_est, 0)
    assert all(math.isnan(empty[k]) for k in ("vde", "gpe", "ffe", "f0_rmse_cents")) and empty["frames"] == 0
    none = R.metrics(f_ref, v_ref, f_est, np.zeros(6, dtype=int), 6)
    assert math.isnan(none["gpe"]) and math.isnan(none["f0_rmse_cents"]) and none["vde"] == 5 / 6 == none["ffe"]
