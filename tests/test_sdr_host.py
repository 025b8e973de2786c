"""BSS Eval SDR without a GPU: the oracle (tests/sdr_ref.py) against the definition — the least-squares projection on the delayed references
by numpy.linalg.lstsq — and against independent mathematics (the Toeplitz solve, the closed form of one tap, the identities that hold
exactly), the measure's reason to exist, every bad argument refused — through the ABI with pointers that are never dereferenced and through
Python on CPU tensors — before any device work, the scratch formulas, and the exports against the header."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import sdr_ref as R

C = _capi.C
EINVAL = -1
REPO = Path(__file__).resolve().parents[1]


# ---- the oracle against the definition ------------------------------------------------------------------------------------------------------------
def projection(s, est, taps):
    """The definition: the estimate (zero past n) projected on the `taps` delayed copies of the reference -> (sdr_db, filter, cond of the
    Gram matrix)."""
    s64, e64 = s.astype(np.float64), est.astype(np.float64)
    n = len(s64)
    delayed = np.zeros((n + taps - 1, taps))
    for k in range(taps):
        delayed[k:k + n, k] = s64
    target = np.concatenate([e64, np.zeros(taps - 1)])
    c, *_ = np.linalg.lstsq(delayed, target, rcond=None)
    y = delayed @ c
    return 10.0 * np.log10(np.sum(y * y) / np.sum((target - y) ** 2)), c, np.linalg.cond(delayed.T @ delayed)


@pytest.mark.parametrize("n,taps,kind", [(1000, 1, "white"), (1000, 64, "white"), (300, 512, "white"), (65, 65, "white"), (4000, 128, "resonator")])
def test_oracle_is_the_least_squares_projection_on_the_delayed_references(n, taps, kind):
    s = R.white(n, seed=n + taps) if kind == "white" else R.resonator(n, seed=n + taps)
    est = R.distorted(s, seed=n + taps + 1)
    want_db, want_c, cond = projection(s, est, taps)
    assert cond < 1e5, cond  # a condition of the case, not a measurement: the bounds below cover lstsq's own cond * U error
    got = R.sdr(s, est, taps)
    assert got["valid"] == 1
    print(f"n {n} L {taps} {kind}: cond {cond:.3g}, sdr {got['sdr_db']:.6f} dB, |d sdr| {abs(got['sdr_db'] - want_db):.3g}, "
          f"|d filter| {np.abs(got['filter'] - want_c).max():.3g}")
    assert abs(got["sdr_db"] - want_db) <= 1e-9
    assert np.abs(got["filter"] - want_c).max() <= 1e-10


@pytest.mark.parametrize("n,taps,kind", [(500, 2, "white"), (200, 65, "white"), (2000, 100, "resonator"), (700, 300, "white")])
def test_oracle_solve_is_numpy_solve_on_the_toeplitz_matrix(n, taps, kind):
    s = R.white(n, seed=taps) if kind == "white" else R.resonator(n, seed=taps)
    r, b = R.correlate(s, s, taps), R.correlate(s, R.distorted(s, seed=taps + 1), taps)
    sol = R.toeplitz_solve(r, b)
    assert sol["valid"] == 1 and 0.0 < sol["error"] <= r[0]
    gram = r[np.abs(np.arange(taps)[:, None] - np.arange(taps)[None, :])]
    want = np.linalg.solve(gram, b)
    cond = np.linalg.cond(gram)
    assert np.abs(sol["x"] - want).max() <= 1e-13 * cond * max(1.0, np.abs(want).max())
    direct = np.array([s[:n - k].astype(np.float64) @ s[k:].astype(np.float64) if k < n else 0.0 for k in range(taps)])
    assert np.abs(r - direct).max() <= 1e-13 * r[0]  # the stated order against BLAS's


def test_oracle_marks_an_indefinite_system_and_a_silent_reference_invalid():
    bad = R.toeplitz_solve(np.array([1.0, 2.0, 0.0, 0.0]), np.ones(4))  # k_1 = -2: E_1 = 1 - 4 < 0
    assert bad["valid"] == 0 and np.isnan(bad["x"]).all() and np.isnan(bad["error"])
    silent = R.sdr(np.zeros(100, dtype=np.float32), R.white(100, 1), 8)
    assert silent["valid"] == 0 and np.isnan(silent["sdr_db"]) and np.isnan(silent["filter"]).all() and (silent["autocorr"] == 0.0).all()
    mute = R.sdr(R.white(100, 1), np.zeros(100, dtype=np.float32), 8)  # valid, no target and no error: 0 / 0
    assert mute["valid"] == 1 and mute["target_energy"] == 0.0 and mute["error_energy"] == 0.0 and np.isnan(mute["sdr_db"])


def test_one_tap_is_the_closed_form_projection():
    s = R.white(1000, seed=3) + np.float32(0.25)  # not zero-mean: the projection takes no mean away
    est = R.distorted(s, seed=4)
    got = R.sdr(s, est, 1)
    s64, e64 = s.astype(np.float64), est.astype(np.float64)
    c = (s64 @ e64) / (s64 @ s64)
    assert abs(got["filter"][0] - c) <= 1e-13 * abs(c)
    want = 10.0 * np.log10(np.sum((c * s64) ** 2) / np.sum((e64 - c * s64) ** 2))
    assert abs(got["sdr_db"] - want) <= 1e-10 and got["prediction_error"] == got["autocorr"][0]


@pytest.mark.parametrize("n,taps", [(1000, 64), (300, 512), (1, 3)])
def test_a_clip_against_itself_and_its_double_is_plus_infinity_exactly(n, taps):
    s = R.resonator(n, seed=n) if n > 1 else np.array([0.75], dtype=np.float32)
    for scale in (1.0, 2.0):
        got = R.sdr(s, (np.float32(scale) * s).astype(np.float32), taps)
        delta = np.zeros(taps)
        delta[0] = scale
        assert got["valid"] == 1 and got["sdr_db"] == np.inf and got["error_energy"] == 0.0 and got["target_energy"] > 0.0
        assert np.array_equal(got["filter"], delta) and not np.signbit(got["filter"]).any()  # lambda is exactly 0 at every step


def test_a_filtered_estimate_scores_far_above_its_plain_snr():
    """The reason for the measure: 0.5 s[t - 17] - 0.2 s[t - 3] plus noise 30 dB down is noise to a sample-by-sample comparison."""
    for seed, s in enumerate((R.white(4000, seed=11), R.resonator(4000, seed=12))):
        est = R.distorted(s, seed=20 + seed)
        got = R.sdr(s, est, 512)
        plain = R.snr_db(s, est)
        print(f"snr_db {plain:.2f}, BSS SDR {got['sdr_db']:.2f}")
        assert got["valid"] == 1 and got["sdr_db"] > plain + 10.0 and plain < 3.0 and got["sdr_db"] > 12.0
        assert abs(got["filter"][17] - 0.5) < 0.05 and abs(got["filter"][3] + 0.2) < 0.05  # the filter IS the linear response


def test_loading_scales_lag_zero_alone():
    s = R.resonator(500, seed=5)
    est = R.distorted(s, seed=6)
    plain, loaded = R.sdr(s, est, 32), R.sdr(s, est, 32, load=1e-3)
    assert loaded["autocorr"][0] == plain["autocorr"][0] * (1.0 + 1e-3) and np.array_equal(loaded["autocorr"][1:], plain["autocorr"][1:])
    assert np.array_equal(loaded["crosscorr"], plain["crosscorr"]) and loaded["sdr_db"] < plain["sdr_db"]  # a loaded filter is not the best fit


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------------
def up(v):
    return 256 * -(-v // 256)


def test_scratch_sizes():
    lib = _capi.load_library()
    for b, t, taps in ((1, 1, 1), (3, 9000, 512), (65, 500, 1024), (2, 4096 - 64 + 1, 64), (2, 4096 - 64 + 2, 64), (7, 160000, 512)):
        segs = -(-(t + taps - 1) // 4096)
        assert lib.l3ac_correlate_scratch_bytes(b, t, taps) == up(4 * b)
        assert lib.l3ac_toeplitz_solve_scratch_bytes(b, taps) == up(4 * b)
        assert lib.l3ac_sdr_scratch_bytes(b, t, taps) == up(4 * b) + up(16 * b * taps) + up(8 * b * taps) + up(16 * b * segs), (b, t, taps)
    assert lib.l3ac_sdr_scratch_bytes(1, 4096 - 64 + 1, 64) == 256 + 1024 + 512 + 256  # exactly one segment ...
    assert lib.l3ac_sdr_scratch_bytes(16, 4096 - 64 + 1, 64) + 256 == lib.l3ac_sdr_scratch_bytes(16, 4096 - 64 + 2, 64)  # ... and just over
    edge = (1 << 31) - 512
    assert lib.l3ac_sdr_scratch_bytes(1, edge, 512) > 0 and lib.l3ac_correlate_scratch_bytes(1, edge, 512) > 0  # max_samples + L - 1 = 2^31 - 1
    for fn in (lib.l3ac_sdr_scratch_bytes, lib.l3ac_correlate_scratch_bytes):
        assert fn(1, edge + 1, 512) < 0 and b"2^31" in lib.l3ac_last_error()
        assert fn(1, (1 << 31) - 1, 2) < 0 and b"2^31" in lib.l3ac_last_error()
        for bad, word in (((0, 100, 8), b"batch"), ((65536, 100, 8), b"batch"), ((1, 0, 8), b"max_samples"), ((1, 1 << 31, 1), b"max_samples"),
                          ((1, 100, 0), b"outside 1..1024"), ((1, 100, 1025), b"outside 1..1024"), ((1, 100, -5), b"outside 1..1024")):
            assert fn(*bad) < 0 and word in lib.l3ac_last_error(), bad
    assert lib.l3ac_sdr_scratch_bytes(1, 100, 1025) < 0 and b"filter_length" in lib.l3ac_last_error()
    assert lib.l3ac_correlate_scratch_bytes(1, 100, 1025) < 0 and b"lags" in lib.l3ac_last_error()
    for bad, word in (((0, 8), b"batch"), ((65536, 8), b"batch"), ((1, 0), b"length"), ((1, 1025), b"length")):
        assert lib.l3ac_toeplitz_solve_scratch_bytes(*bad) < 0 and word in lib.l3ac_last_error(), bad


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, taps = 4096, 3000, 64
    ok = (C.c_int32 * 2)(3000, 100)
    nan, inf = float("nan"), float("inf")
    lens_cases = (dict(lens=(C.c_int32 * 2)(0, 5)), dict(lens=(C.c_int32 * 2)(3000, 3001)), dict(lens=(C.c_int32 * 2)(-7, 5)))
    far = (1 << 31) - 512

    need = lib.l3ac_sdr_scratch_bytes(2, t, taps)

    def sdr(ref=fake, rs=t, est=fake, es=t, batch=2, t=t, lens=ok, taps=taps, load=0.0, out=fake, valid=fake, filt=None, corr=None, scratch=fake,
            nbytes=need):
        return lib.l3ac_sdr(ref, rs, est, es, batch, t, lens, taps, load, out, valid, filt, corr, scratch, nbytes, None)

    # refused on the arguments alone, whatever the pointers: nothing is launched or dereferenced
    for kw in (dict(taps=0), dict(taps=1025), dict(taps=-1), dict(load=-1e-9), dict(load=nan), dict(load=inf), dict(batch=0), dict(batch=65536), dict(t=0),
               dict(rs=t - 1), dict(es=t - 1), *lens_cases, dict(ref=None), dict(est=None), dict(out=None), dict(valid=None), dict(scratch=None),
               dict(scratch=fake + 128), dict(nbytes=need - 1), dict(nbytes=0), dict(t=far, taps=513, rs=far, es=far, lens=None, nbytes=1 << 40)):
        assert sdr(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert sdr(taps=1025) == EINVAL and b"filter_length" in lib.l3ac_last_error()
    assert sdr(load=nan) == EINVAL and b"load" in lib.l3ac_last_error()
    assert sdr(load=-1.0) == EINVAL and b"load" in lib.l3ac_last_error()
    assert sdr(nbytes=need - 1) == EINVAL and b"l3ac_sdr_scratch_bytes" in lib.l3ac_last_error()
    assert sdr(scratch=fake + 128) == EINVAL and b"aligned" in lib.l3ac_last_error()
    assert sdr(lens=(C.c_int32 * 2)(3000, 0)) == EINVAL and b"samples[1]" in lib.l3ac_last_error()
    assert sdr(t=far, taps=513, rs=far, es=far, lens=None, nbytes=1 << 40) == EINVAL and b"2^31" in lib.l3ac_last_error()

    need = lib.l3ac_correlate_scratch_bytes(2, t, taps)

    def correlate(u=fake, us=t, v=fake, vs=t, batch=2, t=t, lens=ok, lags=taps, out=fake, scratch=fake, nbytes=need):
        return lib.l3ac_correlate(u, us, v, vs, batch, t, lens, lags, out, scratch, nbytes, None)

    for kw in (dict(lags=0), dict(lags=1025), dict(batch=0), dict(batch=65536), dict(t=0), dict(us=t - 1), dict(vs=t - 1), *lens_cases, dict(u=None),
               dict(v=None), dict(out=None), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=need - 1), dict(nbytes=0),
               dict(t=far, lags=513, us=far, vs=far, lens=None)):
        assert correlate(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert correlate(lags=0) == EINVAL and b"lags" in lib.l3ac_last_error()
    assert correlate(nbytes=need - 1) == EINVAL and b"l3ac_correlate_scratch_bytes" in lib.l3ac_last_error()
    assert correlate(t=far, lags=513, us=far, vs=far, lens=None) == EINVAL and b"2^31" in lib.l3ac_last_error()

    need = lib.l3ac_toeplitz_solve_scratch_bytes(2, taps)

    def solve(r=fake, b=fake, batch=2, length=taps, x=fake, error=fake, valid=fake, scratch=fake, nbytes=need):
        return lib.l3ac_toeplitz_solve(r, b, batch, length, x, error, valid, scratch, nbytes, None)

    for kw in (dict(length=0), dict(length=1025), dict(batch=0), dict(batch=65536), dict(r=None), dict(b=None), dict(x=None), dict(error=None),
               dict(valid=None), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=need - 1), dict(nbytes=0)):
        assert solve(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert solve(length=1025) == EINVAL and b"length" in lib.l3ac_last_error()
    assert solve(nbytes=need - 1) == EINVAL and b"l3ac_toeplitz_solve_scratch_bytes" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 3000)
    for kw in (dict(filter_length=0), dict(filter_length=1025), dict(filter_length=-3), dict(filter_length="long"), dict(filter_length=None)):
        with pytest.raises(ValueError, match="filter_length"):  # the parameter first, on CPU tensors
            l3ac_amd.sdr(x, x, **kw)
    for bad in (-1e-9, -1.0, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError, match="load"):
            l3ac_amd.sdr(x, x, load=bad)
    for bad in (0, 1025, -1, "many"):
        with pytest.raises(ValueError, match="lags"):
            l3ac_amd.correlate(x, x, bad)
    for kw in (dict(lengths=[0, 5]), dict(lengths=[3001, 5]), dict(lengths=[5]), dict(lengths=[1, 2, 3]), dict(lengths=[2.5, 5])):
        with pytest.raises(ValueError, match="lengths"):
            l3ac_amd.sdr(x, x, **kw)
        with pytest.raises(ValueError, match="lengths"):
            l3ac_amd.correlate(x, x, 8, **kw)
    for other in (torch.zeros(2, 3001), torch.zeros(3, 3000)):
        with pytest.raises(ValueError, match="differ in shape"):
            l3ac_amd.sdr(x, other)
        with pytest.raises(ValueError, match="differ in shape"):
            l3ac_amd.correlate(other, x, 8)
    with pytest.raises(ValueError, match="batch, samples"):
        l3ac_amd.sdr(torch.zeros(3000), torch.zeros(3000))
    with pytest.raises(ValueError, match="empty"):
        l3ac_amd.sdr(torch.zeros(0, 10), torch.zeros(0, 10))
    elsewhere = torch.zeros(2, 3000, device="meta")
    with pytest.raises(RuntimeError, match="is on cpu but estimate is on meta"):
        l3ac_amd.sdr(x, elsewhere)
    with pytest.raises(RuntimeError, match="is on cpu but v is on meta"):
        l3ac_amd.correlate(x, elsewhere, 8)
    far = torch.zeros(1, (1 << 31) - 512, device="meta")  # (no storage behind it)
    with pytest.raises(ValueError, match="2\\^31"):
        l3ac_amd.sdr(far, far, filter_length=513)
    with pytest.raises(ValueError, match="2\\^31"):
        l3ac_amd.correlate(far, far, 513)
    r = torch.zeros(2, 64, dtype=torch.float64)
    for a, b, word in ((r, torch.zeros(2, 65, dtype=torch.float64), "differ in shape"), (r, torch.zeros(3, 64, dtype=torch.float64), "differ in shape"),
                       (torch.zeros(64), torch.zeros(64), "batch, length"), (torch.zeros(2, 1025), torch.zeros(2, 1025), "length 1025"),
                       (torch.zeros(2, 0), torch.zeros(2, 0), "length 0"), (torch.zeros(0, 4), torch.zeros(0, 4), "empty")):
        with pytest.raises(ValueError, match=word):
            l3ac_amd.toeplitz_solve(a, b)
    with pytest.raises(RuntimeError, match="is on cpu but b is on meta"):
        l3ac_amd.toeplitz_solve(r, torch.zeros(2, 64, device="meta"))
    for call in (lambda: l3ac_amd.sdr(x, x), lambda: l3ac_amd.sdr(x.numpy(), x.numpy()), lambda: l3ac_amd.sdr(x, x, lengths=[1, 3000], return_filter=True),
                 lambda: l3ac_amd.sdr(x, x, filter_length=1, load=0.5), lambda: l3ac_amd.correlate(x, x, 1024), lambda: l3ac_amd.correlate(x, x, 1, lengths=[5, 6]),
                 lambda: l3ac_amd.toeplitz_solve(r, r), lambda: l3ac_amd.toeplitz_solve(r.numpy(), r.numpy())):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_exports_header_and_abi_version():
    for name in ("sdr", "correlate", "toeplitz_solve"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5
    assert "DESIGN.md section 3.21" in header
    for formula in ("256 ceil(16 batch L / 256)", "256 ceil(8", "256 ceil(16 batch S / 256)", "S = ceil((max_samples + L - 1) / 4096)"):
        assert formula in header, formula  # the closed form of the scratch is stated
    params = inspect.signature(l3ac_amd.sdr).parameters
    assert list(params)[:6] == ["reference", "estimate", "filter_length", "load", "lengths", "return_filter"]
    assert params["filter_length"].default == 512 and params["load"].default == 0.0 and params["return_filter"].default is False
    assert "sdr" in inspect.signature(l3ac_amd.L3AC.evaluate).parameters
    text = (REPO / "INTEGRATION.md").read_text()
    for name in ("l3ac_correlate", "l3ac_toeplitz_solve", "l3ac_sdr_scratch_bytes"):
        assert name in text
    design = (REPO / "DESIGN.md").read_text()
    assert "### 3.21" in design and "eight families" in design
