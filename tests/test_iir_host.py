"""IIR filtering without a GPU: the Butterworth designs against their closed forms and against scipy's response, the K-weighting cascade
against loudness' own coefficients, the numpy restatement of the parallel recursion (tests/iir_ref.py) against a long-double filter,
the bookkeeping of the streaming session, and that every bad argument is refused — through the ABI and through Python — before any
device work, on CPU tensors as well."""
import ctypes
import math

import numpy as np
import pytest
import torch
from scipy import signal

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.streaming import FILTER_SEGMENT, FilterPush, FilterState, filter_advance
from tests import iir_ref as R

RATES = (8000, 16000, 44100, 48000, 192000)
ORDERS = (1, 2, 3, 4, 5, 8, 12, 16)
KINDS = ("highpass", "lowpass")
IDENTITY = [[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def library_sos(name):
    order, fc, fs, kind = R.FILTERS[name]
    return l3ac_amd.butter_sos(order, fc, fs, kind).numpy()


# ---- 1. butter_sos against its formula ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fs", RATES)
def test_butter_sos_follows_its_closed_forms(fs, kind):
    """Within 4 ulp of the numpy restatement, the low cutoffs the scipy comparison leaves out included (20 Hz at 192 kHz)."""
    for order in range(1, 17):
        for fc in (20.0, 50.0, fs / 100, fs / 20, 0.2 * fs, 0.45 * fs):
            got = l3ac_amd.butter_sos(order, fc, fs, kind)
            want = R.butter_formula(order, fc, fs, kind)
            assert got.shape == ((order + 1) // 2, 6) and got.dtype == torch.float64 and not got.is_cuda
            got = got.numpy()
            assert (got[:, 3] == 1.0).all()
            zero = want == 0.0
            assert (got[zero] == 0.0).all(), (order, fc)
            assert ulps(got[~zero], want[~zero]).max() <= 4, (order, fc, ulps(got[~zero], want[~zero]).max())
            if order % 2:
                assert got[0, 2] == 0.0 and got[0, 5] == 0.0  # the first-order section comes first
    lib = _capi.load_library()
    assert lib.l3ac_butter_sos(4, 50.0, 16000.0, 1, None, 0) == 12
    buf = torch.full((12,), 7.0, dtype=torch.float64)
    assert lib.l3ac_butter_sos(4, 50.0, 16000.0, 1, buf.data_ptr(), 11) == 12 and (buf == 7.0).all()  # a short buffer: nothing written


# ---- 2. butter_sos against scipy's design, by frequency response ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fs", RATES)
def test_butter_sos_has_scipys_response(fs, kind):
    """|H - H_scipy| / |H_scipy| <= 1e-10 at 400 log-spaced points from fc / 8 to 0.999 fs / 2, wherever |H_scipy| > 1e-6."""
    worst = 0.0
    for order in ORDERS:
        for fc in (fs / 100, fs / 20, 0.2 * fs, 0.45 * fs):
            w = np.geomspace(fc / 8, 0.999 * fs / 2, 400)
            _, h = signal.sosfreqz(l3ac_amd.butter_sos(order, fc, fs, kind).numpy(), worN=w, fs=fs)
            _, h_ref = signal.sosfreqz(signal.butter(order, fc, kind, fs=fs, output="sos"), worN=w, fs=fs)
            keep = np.abs(h_ref) > 1e-6
            assert keep.any(), (order, fc)
            rel = np.max(np.abs(h[keep] - h_ref[keep]) / np.abs(h_ref[keep]))
            worst = max(worst, rel)
            assert rel <= 1e-10, (order, fc, rel)
    print(f"butter_sos vs scipy at {fs} Hz, {kind}: worst relative difference {worst:.3g}")


# ---- 3. the K-weighting cascade --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [8000, 16000, 48000])
def test_k_weighting_sos_is_loudness_own_cascade(fs):
    got = l3ac_amd.k_weighting_sos(fs)
    want, _ = l3ac_amd.loudness_coeffs(fs)
    assert got.shape == (2, 6) and got.dtype == torch.float64 and not got.is_cuda
    assert np.array_equal(got.numpy().view(np.int64), want.numpy().view(np.int64))
    with pytest.raises(ValueError):
        l3ac_amd.k_weighting_sos(11025)


# ---- 4. the restatement against long double ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.FILTERS))
def test_restatement_is_within_four_times_what_fp64_costs(name):
    """restate(...) with the restated M against the long-double loop, relative to its peak, within 4 E of every length, E = scipy's
    fp64 filter against the same loop.  Measured here: E from 4.6e-17 (one sample) to 6.3e-13 (F2), the restatement between 0.53 E and
    1.88 E."""
    sos = library_sos(name)
    m_hi, m_lo = R.design_matrix(sos)
    assert m_hi.shape == m_lo.shape == (2 * len(sos), 2 * len(sos))
    assert np.all(np.abs(m_lo) <= np.spacing(np.abs(m_hi))), "M is not a normalised pair"
    for x, (ref, long, e) in zip(R.case_signals(name), R.case_references(name, sos.tobytes())):
        assert e <= 1e-11, (name, len(x), e)
        got = R.restate(sos, x, m_hi, m_lo)
        err = R.error(got, long)
        print(f"{name} n = {len(x)}: E = {e:.3g}, restatement {err:.3g} = {err / e:.2f} E")
        assert err <= 4 * e, (name, len(x), err, e)
        if len(x) <= R.SEG:  # one segment from rest is the sequential filter itself
            assert np.array_equal(got, ref)


def test_rounding_m_to_fp64_is_what_the_pairs_avoid():
    """The reason M is carried as pairs, on the near-double pole of F2: the same restatement with M rounded to fp64 is several times
    further from the long-double filter than with the pair (measured here: see the printed figures)."""
    sos = library_sos("F2")
    m_hi, m_lo = R.design_matrix(sos)
    x = R.case_signals("F2")[-1]
    _, long, e = R.case_references("F2", sos.tobytes())[-1]
    with_pairs = R.error(R.restate(sos, x, m_hi, m_lo), long)
    rounded = R.error(R.restate(sos, x, m_hi, np.zeros_like(m_lo)), long)
    print(f"F2, n = {len(x)}: E = {e:.3g}, pairs {with_pairs:.3g}, M rounded to fp64 {rounded:.3g}")
    assert with_pairs <= 4 * e and rounded > with_pairs


# ---- 5. the session's bookkeeping ---------------------------------------------------------------------------------------------------------------
def test_filter_advance_bookkeeping():
    seg = FILTER_SEGMENT
    assert seg == R.SEG == _capi.load_library().l3ac_sosfilt_segment() == l3ac_amd.sosfilt_segment()
    assert l3ac_amd.filter_advance is filter_advance
    fresh = FilterState()
    assert fresh == (0, 0)
    push, st = filter_advance(fresh, 5, False)
    assert push == FilterPush(0, 5, 5, False, True) and st == FilterState(5, 5)
    push, st = filter_advance(st, 0, False)  # a push that brings nothing
    assert push == FilterPush(5, 0, 0, False, False) and st == FilterState(5, 5)
    push, st = filter_advance(st, seg - 6, False)  # up to k = SEG - 1
    assert push == FilterPush(5, seg - 6, seg - 6, False, False) and st == FilterState(seg - 1, seg - 1)
    push, st = filter_advance(st, 1, False)  # exactly onto the boundary
    assert push == FilterPush(seg - 1, 1, 1, False, False) and st == FilterState(0, seg)
    push, st = filter_advance(st, 3 * seg + 7, False)  # across boundaries
    assert push == FilterPush(0, 3 * seg + 7, 3 * seg + 7, False, False) and st == FilterState(7, 4 * seg + 7)  # (k = 0, yet not fresh)
    push, st = filter_advance(st, seg - 7, False)
    assert st == FilterState(0, 5 * seg)
    push, st = filter_advance(FilterState(seg - 1, seg - 1), 2, False)
    assert push.k == seg - 1 and st == FilterState(1, seg + 1)
    push, st = filter_advance(FilterState(9, 9), 4, True)  # end: the push is as any other, the slot is at rest afterwards
    assert push == FilterPush(9, 4, 4, True, False) and st == fresh
    push, st = filter_advance(FilterState(9, 9), 0, True)
    assert push == FilterPush(9, 0, 0, True, False) and st == fresh
    push, st = filter_advance(fresh, 0, False)  # a stream that has received nothing is still fresh at its next push
    assert push == FilterPush(0, 0, 0, False, True) and st == fresh and filter_advance(st, 3, True)[0] == FilterPush(0, 3, 3, True, True)
    with pytest.raises(ValueError):
        filter_advance(fresh, -1, False)
    lib = _capi.load_library()
    for n in range(1, 9):
        assert lib.l3ac_sosfilt_stream_state(n) == 8 * n
    assert lib.l3ac_sosfilt_stream_state(0) < 0 and lib.l3ac_sosfilt_stream_state(9) < 0 and b"sections" in lib.l3ac_last_error()


# ---- 6. every bad argument, before any device work ----------------------------------------------------------------------------------------------
def c_rows(rows):
    flat = [float(v) for row in rows for v in row]
    return (ctypes.c_double * len(flat))(*flat)


BAD_SOS5 = {  # b0 b1 b2 a1 a2
    "a2 = 1": ([[1.0, 0.0, 0.0, 0.0, 1.0]], b"not stable"),
    "|a1| = 1 + a2": ([[1.0, 0.0, 0.0, 1.5, 0.5]], b"not stable"),
    "a pole outside": ([[1.0, 0.0, 0.0, -2.5, 1.2]], b"not stable"),
    "nan": ([[1.0, math.nan, 0.0, 0.0, 0.0]], b"non-finite"),
    "inf": ([[1.0, 0.0, 0.0, math.inf, 0.0]], b"non-finite"),
    "the second section": ([[1.0, 0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0, -1.0]], b"section 1"),
}


def test_abi_refuses_bad_arguments_before_any_device_work():
    lib = _capi.load_library()
    good = c_rows([[1.0, 0.0, 0.0, 0.0, 0.0]])
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below fails its checks first
    for sections in (0, 9, -1):
        assert lib.l3ac_sosfilt_scratch_bytes(1, 16, sections) < 0 and b"sections" in lib.l3ac_last_error()
        assert lib.l3ac_sosfilt(fake, 16, 1, 16, None, good, sections, fake, 16, 0, fake, 1 << 20, None) == -1 and b"sections" in lib.l3ac_last_error()
        assert lib.l3ac_sosfilt_matrix(good, sections, fake, fake, None) == -1
    for what, (rows, message) in BAD_SOS5.items():
        sos = c_rows(rows)
        assert lib.l3ac_sosfilt(fake, 16, 1, 16, None, sos, len(rows), fake, 16, 0, fake, 1 << 20, None) == -1, what
        assert message in lib.l3ac_last_error(), (what, lib.l3ac_last_error())
        assert lib.l3ac_sosfilt_matrix(sos, len(rows), fake, fake, None) == -1, what
        desc = (_capi.SosStreamDesc * 1)(_capi.SosStreamDesc(0, 0, 4, 0))
        assert lib.l3ac_sosfilt_stream(fake, fake, 1, 8 * len(rows), fake, 4, 4, sos, len(rows), desc, 1, fake, 4, 0, fake, 1 << 20, None) == -1, what
    assert lib.l3ac_sosfilt(fake, 16, 1, 16, None, None, 1, fake, 16, 0, fake, 1 << 20, None) == -1 and b"null sos" in lib.l3ac_last_error()
    # shapes, lengths, strides, buffers, scratch
    need = lib.l3ac_sosfilt_scratch_bytes(2, 16, 1)
    assert need > 0 and lib.l3ac_sosfilt_scratch_bytes(0, 16, 1) < 0 and lib.l3ac_sosfilt_scratch_bytes(65536, 16, 1) < 0
    assert lib.l3ac_sosfilt_scratch_bytes(1, 0, 1) < 0 and lib.l3ac_sosfilt_scratch_bytes(1, 1 << 31, 1) < 0
    lens = (ctypes.c_int32 * 2)
    calls = {
        "batch": lambda: lib.l3ac_sosfilt(fake, 16, 0, 16, None, good, 1, fake, 16, 0, fake, need, None),
        "max_samples": lambda: lib.l3ac_sosfilt(fake, 16, 2, 0, None, good, 1, fake, 16, 0, fake, need, None),
        "null buffer": lambda: lib.l3ac_sosfilt(None, 16, 2, 16, None, good, 1, fake, 16, 0, fake, need, None),
        "row stride": lambda: lib.l3ac_sosfilt(fake, 15, 2, 16, None, good, 1, fake, 16, 0, fake, need, None),
        "samples[1] = 17": lambda: lib.l3ac_sosfilt(fake, 16, 2, 16, lens(16, 17), good, 1, fake, 16, 0, fake, need, None),
        "samples[0] = 0": lambda: lib.l3ac_sosfilt(fake, 16, 2, 16, lens(0, 16), good, 1, fake, 16, 0, fake, need, None),
        "scratch of": lambda: lib.l3ac_sosfilt(fake, 16, 2, 16, None, good, 1, fake, 16, 0, fake, need - 1, None),
        "256-byte aligned": lambda: lib.l3ac_sosfilt(fake, 16, 2, 16, None, good, 1, fake, 16, 0, ctypes.c_void_p(264), need, None),
    }
    for message, call in calls.items():
        assert call() == -1 and message.encode() in lib.l3ac_last_error(), (message, lib.l3ac_last_error())
    # the streaming entry's descriptors
    D = _capi.SosStreamDesc
    seg = lib.l3ac_sosfilt_segment()

    def stream(descs, streams=2, state_stride=8, frames=4, state_out=ctypes.c_void_p(4096)):
        arr = (D * len(descs))(*descs)
        return lib.l3ac_sosfilt_stream(fake, state_out, streams, state_stride, fake, frames, frames, good, 1, arr, len(descs), fake, frames, 0, fake,
                                       1 << 20, None)

    for message, call in {
        "stream 2 of 2": lambda: stream([D(2, 0, 4, 0)]),
        "position": lambda: stream([D(0, seg, 4, 0)]),
        "takes 5": lambda: stream([D(0, 0, 5, 0)]),
        "unknown bit": lambda: stream([D(0, 0, 4, 4)]),
        "a fresh stream at position 5": lambda: stream([D(0, 5, 4, D.FRESH)]),
        "two descriptors": lambda: stream([D(1, 0, 4, 0), D(1, 0, 4, 0)]),
        "descriptors for": lambda: stream([D(0, 0, 4, 0), D(1, 0, 4, 0), D(0, 0, 4, 0)]),
        "state rows": lambda: stream([D(0, 0, 4, 0)], state_stride=7),
        "overlap": lambda: stream([D(0, 0, 4, 0)], state_out=fake),
        "new frames": lambda: stream([D(0, 0, 0, 0)], frames=-1),
    }.items():
        assert call() == -1 and message.encode() in lib.l3ac_last_error(), (message, lib.l3ac_last_error())
    for args in ((0, 50.0, 16000.0), (17, 50.0, 16000.0), (4, 8000.0, 16000.0), (4, 9000.0, 16000.0), (4, 0.0, 16000.0), (4, math.nan, 16000.0),
                 (4, 50.0, 0.0)):
        assert lib.l3ac_butter_sos(*args, 1, None, 0) < 0 and b"butter_sos" in lib.l3ac_last_error(), args


BAD_SOS6 = {
    "a2 = 1": [[1.0, 0.0, 0.0, 1.0, 0.0, 1.0]],
    "unstable after the division by a0": [[1.0, 0.0, 0.0, 0.5, 0.2, 0.6]],
    "nan": [[1.0, 0.0, math.nan, 1.0, 0.0, 0.0]],
    "a0 = 0": [[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]],
    "no section": torch.zeros(0, 6),
    "nine sections": IDENTITY * 9,
    "five columns": [[1.0, 0.0, 0.0, 0.0, 0.0]],
    "one row, flat": [1.0, 0.0, 0.0, 1.0, 0.0, 0.0],
    "not numbers": "butter",
}


def test_python_refuses_bad_arguments_on_cpu_tensors():
    x = torch.zeros(2, 16)
    for what, sos in BAD_SOS6.items():
        with pytest.raises(ValueError):
            l3ac_amd.sosfilt(x, sos)
        with pytest.raises(ValueError):
            l3ac_amd.stream_filter(2, sos)
        with pytest.raises(ValueError):
            l3ac_amd.sosfilt_matrix(sos, "cuda:0")
    for lengths in ([0, 16], [16, 17], [16], [1.5, 2]):
        with pytest.raises(ValueError):
            l3ac_amd.sosfilt(x, IDENTITY, lengths=lengths)
    with pytest.raises(ValueError):
        l3ac_amd.sosfilt(torch.zeros(16), IDENTITY)
    with pytest.raises(ValueError):
        l3ac_amd.sosfilt(x, IDENTITY, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):  # a good call on a CPU tensor: the device is the last thing checked
        l3ac_amd.sosfilt(x, IDENTITY, lengths=[16, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        l3ac_amd.highpass(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        l3ac_amd.sosfilt(x, np.array(IDENTITY * 8))  # eight sections, a first-order section and the identity are legal
    l3ac_amd.stream_filter(1, [[1.0, -1.0, 0.0, 1.0, -0.5, 0.0]])
    for args in ((0, 50, 16000), (17, 50, 16000), (4, 8000, 16000), (4, 8001, 16000), (4, 0, 16000), (4, -5, 16000), (2.5, 50, 16000),
                 (4, math.nan, 16000), (4, 50, 0), (True, 50, 16000), ("4", 50, 16000)):
        with pytest.raises(ValueError):
            l3ac_amd.butter_sos(*args)
        if args[0] == 4:
            with pytest.raises(ValueError):  # highpass: the design's errors come before the device's
                l3ac_amd.highpass(x, cutoff_hz=args[1], sample_rate=args[2])
    assert torch.equal(l3ac_amd.butter_sos(np.int64(4), np.float32(50), np.int32(16000)), l3ac_amd.butter_sos(4, 50.0, 16000.0))
    with pytest.raises(ValueError):
        l3ac_amd.butter_sos(4, 50, 16000, "bandpass")
    with pytest.raises(ValueError):
        l3ac_amd.highpass(x, order=0)
    for streams in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            l3ac_amd.stream_filter(streams, IDENTITY)
    flt = l3ac_amd.stream_filter(2, IDENTITY)
    for bad in (torch.zeros(3, 4), torch.zeros(8), None):
        with pytest.raises(ValueError):
            flt.push(bad)
    with pytest.raises(ValueError):
        flt.push(x, lengths=[17, 0])
    with pytest.raises(ValueError):
        flt.push(x, end=[True])
    with pytest.raises(RuntimeError, match="no CPU path"):
        flt.push(x)
    assert flt.states == [FilterState(), FilterState()]


# ---- 7. the public names ------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_exported():
    for name in ("sosfilt", "sosfilt_segment", "sosfilt_matrix", "butter_sos", "k_weighting_sos", "highpass", "stream_filter", "StreamFilter",
                 "filter_advance"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name)), name
