"""Time alignment without a GPU: every bad argument refused — through the ABI with pointers that are never dereferenced and through
Python on CPU tensors — before any device work, the exports and the header, the scratch size at its edges, and the oracle
(tests/align_ref.py) on pairs whose delay is known."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import align_ref as R

C = _capi.C
EINVAL = -1


def scratch_bytes(batch, t, max_lag):
    return _capi.load_library().l3ac_xcorr_scratch_bytes(batch, t, max_lag)


def test_scratch_size_at_its_edges():
    lens = lambda b: 256 * -(-4 * b // 256)
    for b, t, lag in ((1, 1, 0), (1, 4096, 0), (1, 4097, 0), (3, 4096, 1), (64, 1, 5), (65, 8193, 40), (2, 48000, 1600), (1, (1 << 31) - 1, 16384),
                      (65535, 1, 16384)):
        assert scratch_bytes(b, t, lag) == lens(b) + 8 * b * -(-t // 4096) * (2 * lag + 1), (b, t, lag)
    assert scratch_bytes(1, 1, 0) == 256 + 8 and scratch_bytes(64, 1, 0) == 256 + 512 and scratch_bytes(65, 1, 0) == 512 + 520
    lib = _capi.load_library()
    for bad, word in (((0, 100, 4), b"batch"), ((65536, 100, 4), b"batch"), ((-1, 100, 4), b"batch"), ((2, 0, 4), b"max_samples"),
                      ((2, -3, 4), b"max_samples"), ((2, 1 << 31, 4), b"max_samples"), ((2, 100, -1), b"max_lag"), ((2, 100, 16385), b"max_lag")):
        assert scratch_bytes(*bad) < 0 and word in lib.l3ac_last_error(), bad


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, t, lag = 4096, 9000, 40
    need = scratch_bytes(2, t, lag)
    ok = (C.c_int32 * 2)(300, t)

    def xcorr(ref=fake, rs=t, est=fake, es=t, batch=2, t=t, lens=ok, max_lag=lag, out_lag=fake, pol=fake, delay=fake, corr=fake, row=None,
              scratch=fake, nbytes=need):
        return lib.l3ac_xcorr(ref, rs, est, es, batch, t, lens, max_lag, out_lag, pol, delay, corr, row, scratch, nbytes, None)

    # refused on the arguments alone, whatever the pointers: nothing is launched or dereferenced
    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(t=1 << 31), dict(max_lag=-1), dict(max_lag=16385), dict(lens=(C.c_int32 * 2)(0, t)),
               dict(lens=(C.c_int32 * 2)(-5, t)), dict(lens=(C.c_int32 * 2)(300, t + 1)), dict(rs=t - 1), dict(es=t - 1), dict(ref=None),
               dict(est=None), dict(out_lag=None), dict(pol=None), dict(delay=None), dict(corr=None), dict(scratch=None), dict(scratch=fake + 128),
               dict(nbytes=need - 1), dict(nbytes=0)):
        assert xcorr(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert xcorr(max_lag=16385) == EINVAL and b"max_lag" in lib.l3ac_last_error()
    assert xcorr(nbytes=need - 1) == EINVAL and b"scratch" in lib.l3ac_last_error()
    assert xcorr(es=t - 1) == EINVAL and b"stride" in lib.l3ac_last_error()
    assert xcorr(lens=(C.c_int32 * 2)(300, -1)) == EINVAL and b"samples[1]" in lib.l3ac_last_error()
    assert xcorr(row=fake, nbytes=scratch_bytes(2, t, 0)) == EINVAL  # the scratch of another max_lag

    need = scratch_bytes(2, t, 0)

    def apply(ref=fake, rs=t, est=fake, es=t, batch=2, t=t, lens=ok, lag_dev=fake, out_ref=fake, ors=t, out_est=fake, oes=t, m=fake, scratch=fake,
              nbytes=need):
        return lib.l3ac_align_apply(ref, rs, est, es, batch, t, lens, lag_dev, out_ref, ors, out_est, oes, m, scratch, nbytes, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(t=1 << 31), dict(lens=(C.c_int32 * 2)(0, t)), dict(lens=(C.c_int32 * 2)(300, t + 1)),
               dict(rs=t - 1), dict(es=t - 1), dict(ors=t - 1), dict(oes=t - 1), dict(ref=None), dict(est=None), dict(lag_dev=None),
               dict(out_ref=None), dict(out_est=None), dict(m=None), dict(scratch=None), dict(scratch=fake + 128), dict(nbytes=255), dict(nbytes=0)):
        assert apply(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert apply(oes=t - 1) == EINVAL and b"stride" in lib.l3ac_last_error()
    assert apply(lag_dev=None) == EINVAL and b"lag" in lib.l3ac_last_error()
    assert apply(lens=(C.c_int32 * 2)(300, 0)) == EINVAL and b"samples[1]" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x = torch.zeros(2, 5000)
    lag = torch.zeros(2, dtype=torch.int32)
    for bad in (-1, 16385, 1 << 40, 2.5, "wide", None):
        with pytest.raises(ValueError, match="max_lag"):  # the parameter first, on CPU tensors
            l3ac_amd.delay(x, x, bad)
        with pytest.raises(ValueError, match="max_lag"):
            l3ac_amd.align(x, x, bad)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros((2, 1), dtype=torch.int32), [0, 0], None):
        with pytest.raises(ValueError, match="lag"):
            l3ac_amd.apply_delay(x, x, bad)
    for call in (lambda: l3ac_amd.delay(x, x, 16), lambda: l3ac_amd.delay(x.numpy(), x, 16), lambda: l3ac_amd.delay(x, x, 16, lengths=[0, 5]),
                 lambda: l3ac_amd.delay(x, x, 0, return_xcorr=True), lambda: l3ac_amd.apply_delay(x, x, lag),
                 lambda: l3ac_amd.apply_delay(x, x, lag, lengths=[1, 5001]), lambda: l3ac_amd.align(x, x, 16384)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_exports_and_abi_version():
    for name in ("delay", "apply_delay", "align"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5
    assert "DESIGN.md section 3.16" in header


# ---- the oracle on known answers ----------------------------------------------------------------------------------------------------------------
def test_beta_is_the_figure_of_the_design():
    assert abs(R.gamma_r() - 7.63e-6) < 1e-8
    for n in (1, 4097, 48000):
        assert 7.62e-6 < R.beta(n) < 7.7e-6 and R.beta(n) - R.gamma_r() < 1e-13  # the fp64 part is nothing beside the fp32 chains


@pytest.mark.parametrize("name", list(R.known_cases()))
def test_oracle_reads_known_delays(name):
    ref, est, max_lag, lag, polarity = R.known_cases()[name]
    o = R.oracle(ref, est, max_lag)
    assert o["robust"] and (o["lag"], o["polarity"]) == (lag, polarity), (o["lag"], o["polarity"], o["margin"])
    assert 0.99 < abs(o["correlation"]) <= 1.0 + 1e-12 and math.copysign(1, o["correlation"]) == polarity
    if abs(lag) == max_lag:
        assert o["delay"] == lag  # no refinement at the ends of the range
    elif not name.startswith("sines"):
        assert abs(o["delay"] - lag) < 1e-3  # an exact copy: the parabola's vertex is at the peak up to the shrinking overlap


@pytest.mark.parametrize("delay", R.SINES_DELAYS)
def test_oracle_reads_fractional_delays_of_the_sine_mixture(delay):
    """12 tones at 100-800 Hz, 16 kHz, 1.5 s: the parabola reads the delay within 0.005 samples (observed: 0.0011, 0.0002, 0.0010)."""
    ref, est = R.sines(R.SINES_N, delay)
    o = R.oracle(ref, est, 32)
    print(f"\n[align] sines late by {delay}: delay {o['delay']:.5f}, margin {o['margin']:.2e}")
    assert o["robust"] and o["lag"] == round(delay) and abs(o["delay"] - delay) <= 0.005


def test_every_gpu_case_is_robust_on_the_oracle_alone():
    """The GPU suite asserts this again before each comparison; here it is seen without a GPU.  The smallest margin over the runner-up is
    that of the sine mixture at -7.49, 3.9e-4 of sqrt(E_ref E_est), against 2 beta = 1.5e-5."""
    margins = {}
    for name, (n, max_lag, shift) in R.EDGES.items():
        o = R.oracle(*R.noisy_copy(n, shift), max_lag)
        assert o["robust"] and o["lag"] == shift and o["polarity"] == 1, (name, o["lag"], o["margin"])
        margins[name] = o["margin"]
    o = R.oracle(*R.tone_noise(12000, 13), 100)
    assert o["robust"] and o["lag"] == 13, o["margin"]
    margins["tone + noise"] = o["margin"]
    o = R.oracle(*R.integers(4096 + 33), 40)
    assert o["robust"], o["margin"]
    margins["integers"] = o["margin"]
    print("\n[align] margins over the runner-up / sqrt(E_ref E_est):", {k: f"{v:.2e}" for k, v in margins.items()})


def test_the_matrix_form_is_the_direct_form():
    """The identity the kernel rests on, in fp64: the segments' diagonal sums are the cross-correlation, at clip and lag edges."""
    for n, max_lag, shift in ((6000, 64, 37), (70, 100, 3), (4096, 0, 0), (4097, 17, -17), (33, 33, 5), (8193, 16, 2)):
        ref = R.white(n, n)
        est = R.delayed(R.white(n, n + 1) + ref, shift)
        r, a = R.xcorr(ref, est, max_lag)
        assert np.abs(R.gemm_form(ref, est, max_lag) - r).max() <= 64 * R.U64 * a.max(), (n, max_lag)


def test_the_fp32_chain_stays_far_inside_the_bound():
    """`chain_form` is the specification's arithmetic: fp32 fmaf chains of 128 terms, fp64 diagonal and segment sums.  Against the direct
    fp64 form it meets the bound beta A(d) (observed: 0.5 % of it; the roundings of a chain average out where the bound adds them up)."""
    one, up = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    tie = np.array([one]), np.array([one])  # the product is 1 + 2^-11 + 2^-24: half way between two fp32; the addend decides
    assert R.fma32(*tie, np.array([np.float32(2.0 ** -80)]))[0] == up and R.fma32(*tie, np.array([np.float32(-2.0 ** -80)]))[0] == np.float32(1.0 + 2.0 ** -11)
    assert R.fma32(*tie, np.array([np.float32(0.0)]))[0] == np.float32(1.0 + 2.0 ** -11)  # the tie itself: to even
    worst = 0.0
    for ref, est, max_lag in ((*R.noisy_copy(4097, 9), 17), (*R.noisy_copy(70, 3), 100), (*R.tone_noise(12000, 13), 100), (*R.integers(4096 + 33), 40)):
        r, a = R.xcorr(ref, est, max_lag)
        c = R.chain_form(ref, est, max_lag)
        ok = a > 0
        assert (c[~ok] == 0.0).all() and (np.abs(c - r) <= R.beta(len(ref)) * a).all()
        worst = max(worst, float((np.abs(c - r)[ok] / (R.beta(len(ref)) * a[ok])).max()))
    assert np.array_equal(c, r)  # (the last pair: integer data is exact)
    print(f"\n[align] fp32 chain against the direct fp64 form: worst {worst:.4f} beta A")


def test_pick_and_refine_on_given_rows():
    assert R.pick(np.array([1.0, -3.0, 2.0, 3.0, 0.0])) == 1  # equal |r| at d = -1 and d = +1: the smaller d
    assert R.pick(np.array([5.0, 0.0, 1.0, 0.0, -5.0])) == 0  # equal at -2 and +2
    assert R.pick(np.array([2.0, 0.0, 0.0, 2.0, 0.0])) == 3  # the smaller |d| first
    assert R.pick(np.zeros(7)) == 3 and R.pick(np.array([math.nan, math.nan, math.nan])) == 1  # all equal, nothing comparable: lag 0
    lag, pol, delay, corr = R.refine(np.array([0.0, -1.0, -4.0, -3.0, 0.0]), 4.0, 4.0)
    assert (lag, pol, corr) == (0, -1, -1.0) and delay == (0.5 * (1.0 - 3.0)) / ((1.0 - 8.0) + 3.0)  # the vertex leans to the larger neighbour
    assert delay == 0.25
    assert R.refine(np.array([4.0, 1.0, 0.0]), 1.0, 16.0)[:3] == (-1, 1, -1.0)  # at -L: no refinement
    assert R.refine(np.array([1.0, 4.0, 7.0]), 1.0, 49.0) == (1, 1, 1.0, 1.0)
    assert R.refine(np.array([2.0, 2.0, 2.0]), 1.0, 4.0)[2] == 0.0  # den = 0: no shift
    out = R.refine(np.array([1.0, 2.0, 3.0]), 0.0, 5.0)
    assert out[:3] == (0, 0, 0.0) and math.isnan(out[3])
    r, a = np.array([0.0, 1.0, 0.5]), np.ones(3)
    assert R.robust(r, a, (1.0, 1.0), 0.2) and not R.robust(r, a, (1.0, 1.0), 0.25) and R.robust(r, a, (0.0, 1.0), 10.0)


def test_shift_pair_and_delayed():
    x = np.arange(1, 8, dtype=np.float32)
    assert R.delayed(x, 2).tolist() == [0, 0, 1, 2, 3, 4, 5] and R.delayed(x, -3).tolist() == [4, 5, 6, 7, 0, 0, 0] and not R.delayed(x, 7).any()
    r, e, m = R.shift_pair(x, R.delayed(x, 2), 2)
    assert m == 5 and r.tolist() == e.tolist() == [1, 2, 3, 4, 5, 0, 0]
    r, e, m = R.shift_pair(x, R.delayed(x, -3), -3)
    assert m == 4 and r.tolist() == e.tolist() == [4, 5, 6, 7, 0, 0, 0]
    assert R.shift_pair(x, x, 7)[2] == 0 and R.shift_pair(x, x, -9)[2] == 0 and not R.shift_pair(x, x, 9)[0].any()
