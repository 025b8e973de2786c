"""Time alignment on the MI355X (kernels/align.hip) against the fp64 oracle (tests/align_ref.py): the
cross-correlation row exact on integer data and within the derived bound beta A(d) of the oracle's elsewhere, the energies and the
correlation within their bounds, lag / polarity / delay bit for bit the pick of the library's OWN row, lag and polarity those of the
oracle, the shapes at which the kernels take another path, bit invariance over batch / row / stride / scratch size / what lies after a
clip's length, the shift against NumPy slicing, `align` against the composed calls, and graph capture as the first alignment call of
the process.

Every numeric case first asserts on the ORACLE alone (`conditions`) that its pick is robust: the peak leads the runner-up by more than
2 beta max A, so the pick is the same in any arithmetic that meets the bound.  A case that misses it fails, it is never skipped.  The
figures measured on an MI355X are in the docstrings of the tests that print them."""
import functools
import sys

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import align_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("lag", "polarity", "delay", "correlation", "xcorr")


def bits(t):
    """A device tensor as integers: NaN entries compare like any other."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def dev(*arrays):
    return torch.from_numpy(np.stack(arrays)).to(DEV)


def run(ref, est, max_lag, **kw):
    """The library on one pair alone -> numpy scalars and the (2 L + 1,) row."""
    out = l3ac_amd.delay(dev(ref), dev(est), max_lag, return_xcorr=True, **kw)
    assert set(out) == set(KEYS) and all(v.is_cuda for v in out.values())
    assert out["lag"].dtype == out["polarity"].dtype == torch.int32 and out["delay"].dtype == out["correlation"].dtype == out["xcorr"].dtype == torch.float64
    assert out["xcorr"].shape == (1, 2 * max_lag + 1) and all(out[k].shape == (1,) for k in KEYS[:4])
    return {k: v[0].cpu().numpy() for k, v in out.items()}


# ---- 6. graph capture: FIRST in this file, no other file of the suite calls delay / apply_delay ---------------------------------------------------
def test_graph_capture_replays_the_eager_bits_as_the_first_alignment_call():
    """There is no table to upload and no kernel to configure: the very first call may be the captured one."""
    a, b = R.noisy_copy(9000, 17, seed=1), R.noisy_copy(9000, -30, seed=2)
    ref, est = dev(a[0], b[0]), dev(a[1], b[1])
    other = dev(b[1], a[1])
    lens = [9000, 5001]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d = l3ac_amd.delay(ref, est, 40, lengths=lens, return_xcorr=True)
        shifted = l3ac_amd.apply_delay(ref, est, d["lag"], lengths=lens)
    graph.replay()
    torch.cuda.synchronize()
    e_d = l3ac_amd.delay(ref, est, 40, lengths=lens, return_xcorr=True)
    e_shifted = l3ac_amd.apply_delay(ref, est, e_d["lag"], lengths=lens)
    assert e_d["lag"].tolist() == [17, -30] and e_shifted[2].tolist() == [9000 - 17, 5001 - 30]
    for k in e_d:
        assert same(d[k], e_d[k]), k
    for got, want in zip(shifted, e_shifted):
        assert same(got, want)
    est.copy_(other)  # the replay reads the tensors' current contents
    graph.replay()
    torch.cuda.synchronize()
    again = l3ac_amd.delay(ref, other, 40, lengths=lens, return_xcorr=True)
    for k in again:
        assert same(d[k], again[k]), k
    for got, want in zip(shifted, l3ac_amd.apply_delay(ref, other, again["lag"], lengths=lens)):
        assert same(got, want)
    assert not same(again["xcorr"], e_d["xcorr"])


# ---- the numeric cases ---------------------------------------------------------------------------------------------------------------------------
def conditions(o, name):
    """The pick robust, on the oracle alone; a case that misses it fails (it is never skipped)."""
    assert o["robust"], f"{name}: the oracle's peak leads by {o['margin']:.3e} sqrt(E_ref E_est) only: not above 2 beta max A"
    return o


def check_against_oracle(o, g, n, name):
    """Checks 2 of one pair -> the worst |r_library - r_oracle| / (beta A)."""
    bt, fp64 = o["beta"], (2 * n + 8) * R.U64
    # the row: exact zeros where no product is non-zero, within beta A(d) elsewhere
    err = np.abs(g["xcorr"] - o["r"])
    assert (err <= bt * o["A"]).all(), f"{name}: |r - r_oracle| is {(err[o['A'] > 0] / (bt * o['A'][o['A'] > 0])).max():.3f} beta A"
    worst = float((err[o["A"] > 0] / (bt * o["A"][o["A"] > 0])).max()) if (o["A"] > 0).any() else 0.0
    # lag, polarity and delay are the pick of the library's own row, bit for bit
    lag, polarity, delay, _ = R.refine(g["xcorr"], o["e_ref"], o["e_est"])
    assert (int(g["lag"]), int(g["polarity"])) == (lag, polarity), name
    assert np.float64(delay).view(np.int64) == g["delay"].view(np.int64), (name, delay, float(g["delay"]))
    # ... and lag and polarity the oracle's
    assert (lag, polarity) == (o["lag"], o["polarity"]), name
    if polarity == 0:
        assert np.isnan(g["correlation"]) and float(g["delay"]) == 0.0, name
        return worst
    # the energies, through sqrt(E_ref E_est) = r(d*) / correlation (a product, a root and two quotients on top of the two sums), and
    # the correlation
    at = lag + (len(o["r"]) - 1) // 2
    root = np.sqrt(o["e_ref"] * o["e_est"])
    assert abs(float(g["xcorr"][at] / g["correlation"]) - root) <= fp64 * root, name
    assert abs(float(g["correlation"]) - o["correlation"]) <= bt * o["A"][at] / root + fp64, name
    assert abs(float(g["correlation"])) <= 1.0 + bt + fp64, name
    return worst


def case(ref, est, max_lag, name, **kw):
    o = conditions(R.oracle(ref, est, max_lag), name)
    return o, check_against_oracle(o, run(ref, est, max_lag, **kw), len(ref), name)


def test_exact_data():
    """Integer samples in [-8, 8], the two sides drawn apart, n = 4096 + 33, L = 40: every product and every partial sum is exact in
    fp32, so every r(d) equals the oracle's exactly; a wrong lane map or a wrong diagonal cannot."""
    ref, est = R.integers(4096 + 33)
    o = conditions(R.oracle(ref, est, 40), "integers")
    g = run(ref, est, 40)
    assert np.array_equal(g["xcorr"], o["r"]), np.flatnonzero(g["xcorr"] != o["r"]).tolist()
    assert (int(g["lag"]), int(g["polarity"])) == (o["lag"], o["polarity"]) and np.abs(o["r"]).max() > 500
    assert not np.array_equal(o["r"], o["r"][::-1])  # (asymmetric: a row mirrored in d would show)


def test_the_row_is_the_specified_arithmetic_bit_for_bit():
    """The specification fixes the bits of r: fp32 fmaf chains over k in the order of k, fp64 sums in the order of a, then of g
    (`align_ref.chain_form`, with a correctly rounded fmaf).  Two segments, a clip shorter than the lag range, two blocks of lags."""
    for ref, est, max_lag in ((*R.noisy_copy(4097, 9), 17), (*R.noisy_copy(70, 3), 100), (*R.tone_noise(6000, 13), 120)):
        g = run(ref, est, max_lag)
        want = R.chain_form(ref, est, max_lag)
        assert np.array_equal(g["xcorr"].view(np.int64), want.view(np.int64)), (len(ref), max_lag, np.flatnonzero(g["xcorr"] != want).tolist()[:8])


@pytest.mark.parametrize("name", list(R.known_cases()) + ["tone + noise"])
def test_bound_against_the_oracle(name):
    """Checks 2 on the inputs with known answers.  Measured on an MI355X, worst |r - r_oracle| / (beta A): 0.0061 white + 37, 0.0026
    coloured - 48, 0.0014 inverted, 0.0069 / 0.0057 / 0.0037 the sine mixture at 12.3 / -7.49 / 0.25, 0.0046 tone + noise."""
    if name == "tone + noise":
        (ref, est), max_lag, lag, polarity = R.tone_noise(12000, 13), 100, 13, 1
    else:
        ref, est, max_lag, lag, polarity = R.known_cases()[name]
    o, worst = case(ref, est, max_lag, name)
    assert (o["lag"], o["polarity"]) == (lag, polarity)
    print(f"\n[align] {name}: worst |r - r_oracle| = {worst:.4f} beta A (beta = {o['beta']:.3e}), margin {o['margin']:.2e}")


def test_fractional_delays_of_the_sine_mixture():
    for delay in R.SINES_DELAYS:
        ref, est = R.sines(R.SINES_N, delay)
        g = run(ref, est, 32)
        assert abs(float(g["delay"]) - delay) <= 0.005, (delay, float(g["delay"]))


def test_each_energy_alone():
    """delay(x, x, 0): correlation = r(0) / sqrt(E E), so E = r(0) / correlation up to three fp64 roundings."""
    for x in (R.white(5000, 9), R.coloured(4097, 10), R.integers(333)[0]):
        g = run(x, x, 0)
        want = R.energies(x, x)[0]
        assert int(g["lag"]) == 0 and int(g["polarity"]) == 1
        assert abs(float(g["xcorr"][0] / g["correlation"]) - want) <= (2 * len(x) + 8) * R.U64 * want


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.EDGES))
def test_edges(name):
    """Checks 2 at each shape.  Measured on an MI355X, worst |r - r_oracle| / (beta A): 0.0003 (L = 1) to 0.0055 (n = L = 33)."""
    n, max_lag, shift = R.EDGES[name]
    ref, est = R.noisy_copy(n, shift)
    o, worst = case(ref, est, max_lag, name)
    assert o["lag"] == shift and o["polarity"] == 1
    if abs(shift) == max_lag:
        g = run(ref, est, max_lag)
        assert float(g["delay"]) == float(shift)  # no refinement at the ends of the range
    print(f"\n[align] {name}: worst |r - r_oracle| = {worst:.4f} beta A")


def test_edge_shapes_are_what_they_say():
    seg, block = 4096, 224  # samples of a segment, lags of a block (kernels/align.hip)
    assert [-(-R.EDGES[f"n = {n}"][0] // seg) for n in (4095, 4096, 4097, 8193)] == [1, 1, 2, 3]
    blocks = lambda name: -(-(2 * R.EDGES[name][1] + 1) // block)
    assert blocks("223 lags: one block, all of it") == 1 and blocks("225 lags: a second block of one lag") == 2 and blocks("601 lags: three blocks") == 3
    assert blocks("n = 48000, L = 1600") == 15 and R.EDGES["L above n: n = 70, L = 100"][1] > R.EDGES["L above n: n = 70, L = 100"][0]


def test_a_silent_estimate_and_an_inverted_one():
    ref = R.white(5000, 5)
    zero = run(ref, np.zeros_like(ref), 30)
    assert (int(zero["lag"]), int(zero["polarity"]), float(zero["delay"])) == (0, 0, 0.0) and np.isnan(zero["correlation"])
    assert not zero["xcorr"].any()
    assert np.isnan(run(np.zeros_like(ref), ref, 30)["correlation"])
    o, _ = case(ref, -R.delayed(ref, -7), 30, "inverted")
    assert (o["lag"], o["polarity"]) == (-7, -1)


def test_unaligned_and_strided_rows_give_the_same_bits():
    (a, x), (b, y) = R.noisy_copy(6001, 11, seed=3), R.noisy_copy(6001, -4, seed=4)
    plain = l3ac_amd.delay(dev(a, b), dev(x, y), 20, return_xcorr=True)
    views = []
    for rows in (dev(a, b), dev(x, y)):
        wide = torch.full((2, 6011), 7.0, device=DEV)
        wide[:, 1:6002] = rows
        views.append(wide[:, 1:6002])
        assert views[-1].data_ptr() % 16 != 0 and views[-1].stride(0) % 4 != 0 and not views[-1].is_contiguous()
    shifted = l3ac_amd.delay(*views, 20, return_xcorr=True)
    for k in KEYS:
        assert same(plain[k], shifted[k]), k
    assert plain["lag"].tolist() == [11, -4]
    for got, want in zip(l3ac_amd.apply_delay(*views, plain["lag"]), l3ac_amd.apply_delay(dev(a, b), dev(x, y), plain["lag"])):
        assert same(got, want)


# ---- 4. invariance -------------------------------------------------------------------------------------------------------------------------------
def test_a_clip_does_not_depend_on_its_batch_row_scratch_or_what_follows_it():
    lens, shifts, max_lag = [9000, 4096, 333], [25, -50, 3], 50
    pairs = [R.noisy_copy(n, s, seed=10 + i) for i, (n, s) in enumerate(zip(lens, shifts))]
    rows = np.empty((2, 3, 9000), dtype=np.float32)
    for i, (pair, n) in enumerate(zip(pairs, lens)):
        for side in range(2):
            rows[side, i, :n] = pair[side]
            rows[side, i, n::2] = 1e30  # what lies after a clip's length is not read
            rows[side, i, n + 1::2] = np.nan
    ref, est = torch.from_numpy(rows[0]).to(DEV), torch.from_numpy(rows[1]).to(DEV)
    alone = [l3ac_amd.delay(dev(p[0]), dev(p[1]), max_lag, return_xcorr=True) for p in pairs]
    assert [int(a["lag"][0]) for a in alone] == shifts
    need = _capi.load_library().l3ac_xcorr_scratch_bytes(3, 9000, max_lag)
    for order in ([0, 1, 2], [2, 1, 0]):
        for extra in (None, 0, need):  # the minimum scratch (twice: the default is the minimum) and twice the minimum
            out = l3ac_amd.delay(ref[order], est[order], max_lag, lengths=[lens[i] for i in order], return_xcorr=True, extra_scratch=extra)
            for row, i in enumerate(order):
                for k in KEYS:
                    assert same(out[k][row], alone[i][k][0]), (order, extra, i, k)
    # NaN inside one clip leaves the others bit for bit, and its own lag inside the range
    est[1, 100] = np.nan
    out = l3ac_amd.delay(ref, est, max_lag, lengths=lens, return_xcorr=True)
    for i in (0, 2):
        for k in KEYS:
            assert same(out[k][i], alone[i][k][0]), (i, k)
    assert -max_lag <= int(out["lag"][1]) <= max_lag


# ---- 5. apply_delay and align ----------------------------------------------------------------------------------------------------------------------
def test_apply_delay_equals_numpy_slicing():
    t = 5000
    lens = [5000, 4097, 33, 1, 700, 700, 5000, 64]
    lags = [7, -13, 0, 0, 700, -705, -(1 << 31), 63]  # positive, negative, zero, and |d| at and above n
    rng = np.random.default_rng(21)
    ref, est = rng.standard_normal((2, len(lens), t)).astype(np.float32)
    for i, n in enumerate(lens):
        ref[i, n:], est[i, n:] = np.nan, 1e30
    lag = torch.tensor(lags, dtype=torch.int32, device=DEV)
    out_r, out_e, m = l3ac_amd.apply_delay(torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV), lag, lengths=lens)
    assert out_r.shape == out_e.shape == (len(lens), t) and out_r.dtype == out_e.dtype == torch.float32 and m.dtype == torch.int32 and m.is_cuda
    for i, (n, d) in enumerate(zip(lens, lags)):
        want_r, want_e, want_m = R.shift_pair(ref[i, :n], est[i, :n], d)
        assert int(m[i]) == want_m == max(0, n - abs(d)), i
        for got, want in ((out_r[i], want_r), (out_e[i], want_e)):
            got = got.cpu().numpy()
            assert np.array_equal(got[:n].view(np.int32), want.view(np.int32)), i
            assert not got[want_m:].view(np.int32).any(), i  # exact zeros after m, to the end of the row
    whole = l3ac_amd.apply_delay(torch.from_numpy(ref[:1]).to(DEV), torch.from_numpy(est[:1]).to(DEV), lag[:1])  # no lengths: n = T
    assert int(whole[2][0]) == t - 7 and np.array_equal(whole[1][0, :t - 7].cpu().numpy(), est[0, 7:])


def test_align_puts_shifted_copies_on_common_samples():
    x, y = R.white(8000, 31), R.coloured(8000, 32)
    ref, est = dev(x, y, x), dev(R.delayed(x, 23), R.delayed(y, -40), -R.delayed(x, 5))
    lens = [8000, 6000, 7000]
    before = l3ac_amd.signal_metrics(ref, est, lengths=lens)
    assert (before["mse"] > 0).all()
    ref_a, est_a, new_lens, info = l3ac_amd.align(ref, est, 64, lengths=lens)
    assert new_lens == [8000 - 23, 6000 - 40, 7000 - 5] and all(type(v) is int for v in new_lens) and info["empty"] == []
    assert info["lag"].tolist() == [23, -40, 5] and info["polarity"].tolist() == [1, 1, -1] and info["lengths"].tolist() == new_lens
    after = l3ac_amd.signal_metrics(ref_a, est_a, lengths=new_lens)
    assert after["mse"][:2].tolist() == [0.0, 0.0] and float(after["mse"][2]) > 0  # the polarity is not applied
    est_a[2] = -est_a[2]
    assert float(l3ac_amd.signal_metrics(ref_a, est_a, lengths=new_lens)["mse"][2]) == 0.0
    # the composed calls, bit for bit
    d = l3ac_amd.delay(ref, est, 64, lengths=lens)
    composed = l3ac_amd.apply_delay(ref, est, d["lag"], lengths=lens)
    ref_a, est_a, _, _ = l3ac_amd.align(ref, est, 64, lengths=lens)
    assert same(ref_a, composed[0]) and same(est_a, composed[1]) and same(info["lengths"], composed[2])
    for k in d:
        assert same(info[k], d[k]), k


def test_align_reports_clips_with_no_common_sample(monkeypatch):
    """Only a lag that reaches the clip's length leaves nothing; `delay` never picks one on finite data (r is exactly 0 there), so the
    lags are handed in."""
    x = R.white(100, 41)
    ref, est = dev(x, x), dev(x, x)
    module = sys.modules["l3ac_amd.align"]
    real = module.delay
    monkeypatch.setattr(module, "delay", lambda *a, **kw: dict(real(*a, **kw), lag=torch.tensor([60, 3], dtype=torch.int32, device=DEV)))
    ref_a, est_a, new_lens, info = l3ac_amd.align(ref, est, 80, lengths=[60, 100])
    assert new_lens == [1, 97] and info["empty"] == [0] and info["lengths"].tolist() == [0, 97]
    assert not ref_a[0].any() and not est_a[0].any()
    m = l3ac_amd.signal_metrics(ref_a, est_a, lengths=new_lens)  # the metric functions take the list as it is
    assert float(m["mse"][1]) > 0
