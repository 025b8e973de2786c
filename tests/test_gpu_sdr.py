"""BSS Eval SDR on the GPU (csrc/kernels/sdr.hip) against the fp64 oracle of tests/sdr_ref.py: the correlations, the
filter, the prediction error, the validity and the two energies bit for bit; integer data exactly, without the oracle's order; the identities
that hold bit for bit; the value behind the log within the bound section 3.21 derives (1 ulp for the device's log10, as HIP's documentation
states and nobody has measured on gfx950, plus the product); invalid pairs; a pair's bits independent of its batch, strides, scratch and what
follows its length; composition; stream capture as the first call; and isolation from a corrupt neighbour."""
import functools

import numpy as np
import pytest
import torch

import l3ac_amd
from tests import poison
from tests import sdr_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALARS = (("target_energy", "target_energy"), ("error_energy", "error_energy"), ("prediction_error", "prediction_error"))
VECTORS = ("autocorr", "crosscorr", "filter")


def bits(t):
    """A tensor or array as integers: NaN entries compare like any other."""
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def dev(*arrays):
    return torch.from_numpy(np.stack(arrays)).to(DEV)


def cpu(t):
    return t.detach().cpu().numpy()


# ---- 8. capture: first in the file, so that nothing of this family has run before it -----------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits_as_the_first_call_of_the_family():
    """There is no table to upload and no kernel to configure: the very first call may be the captured one."""
    s = dev(R.resonator(1200, seed=80), R.white(1200, seed=81))
    est = dev(R.distorted(cpu(s[0]), seed=82), R.distorted(cpu(s[1]), seed=83))
    other = dev(R.distorted(cpu(s[0]), seed=84, noise_db=10.0), R.distorted(cpu(s[1]), seed=85, noise_db=10.0))
    kw = dict(filter_length=37, lengths=[1200, 640], return_filter=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = l3ac_amd.sdr(s, est, **kw)
        out_corr = l3ac_amd.correlate(s, est, 37, lengths=[1200, 640])
        out_solve = l3ac_amd.toeplitz_solve(out["autocorr"], out["crosscorr"])
    graph.replay()
    torch.cuda.synchronize()
    eager = l3ac_amd.sdr(s, est, **kw)
    for key in eager:
        assert same(out[key], eager[key]), key
    assert same(out_corr, eager["crosscorr"]) and same(out_solve["x"], eager["filter"]) and same(out_solve["error"], eager["prediction_error"])
    assert cpu(out_solve["valid"]).tolist() == cpu(eager["valid"]).tolist() == [1, 1]
    est.copy_(other)  # the replay reads the tensors' current contents
    graph.replay()
    torch.cuda.synchronize()
    again = l3ac_amd.sdr(s, other, **kw)
    for key in again:
        assert same(out[key], again[key]), key
    assert same(out_corr, again["crosscorr"]) and same(out_solve["x"], again["filter"])
    assert not same(again["sdr_db"], eager["sdr_db"]) and (again["sdr_db"] < eager["sdr_db"]).all()


# ---- 1. the bit-exact stage ---------------------------------------------------------------------------------------------------------------------
# every L of {1, 2, 63, 64, 65, 512, 1024} with n = 4096 - L + 1 and 4096 - L + 2 (exactly one residual segment, and just over one), and every
# n of {1, 63, 64, 65, 200, 300 (n < L), 9000 (three segments, five correlation tiles)} at least once
CASES = [(1, 1), (1, 4096), (1, 4097), (2, 63), (2, 4095), (2, 4096), (63, 64), (63, 4034), (63, 4035), (64, 65), (64, 4033), (64, 4034), (64, 9000),
         (65, 200), (65, 4032), (65, 4033), (512, 1), (512, 300), (512, 3585), (512, 3586), (512, 9000), (1024, 63), (1024, 300), (1024, 3073),
         (1024, 3074), (1024, 9000)]
assert {c[0] for c in CASES} == {1, 2, 63, 64, 65, 512, 1024} and {1, 63, 64, 65, 200, 300, 9000} <= {c[1] for c in CASES}
assert all((taps, 4096 - taps + 1) in CASES and (taps, 4096 - taps + 2) in CASES for taps in (1, 2, 63, 64, 65, 512, 1024))


@functools.lru_cache(maxsize=None)
def case_inputs(taps, n):
    """Two pairs: white noise and the resonator, each against the filtered-plus-noise estimate."""
    s = np.stack([R.white(n, seed=1000 * taps + n), R.resonator(n, seed=2000 * taps + n)])
    est = np.stack([R.distorted(s[0], seed=3000 * taps + n), R.distorted(s[1], seed=4000 * taps + n)])
    return s, est


@functools.lru_cache(maxsize=None)
def case_oracle(taps, n):
    s, est = case_inputs(taps, n)
    return [R.sdr(s[i], est[i], taps) for i in range(2)]


@functools.lru_cache(maxsize=None)
def case_device(taps, n):
    s, est = case_inputs(taps, n)
    got = l3ac_amd.sdr(torch.from_numpy(s).to(DEV), torch.from_numpy(est).to(DEV), filter_length=taps, return_filter=True)
    assert all(v.is_cuda for v in got.values())
    return {k: cpu(v) for k, v in got.items()}


@pytest.mark.parametrize("taps,n", CASES)
def test_correlations_filter_validity_and_energies_are_the_oracles_bits(taps, n):
    want, got = case_oracle(taps, n), case_device(taps, n)
    assert set(got) == {"sdr_db", "target_energy", "error_energy", "prediction_error", "valid", "filter", "autocorr", "crosscorr"}
    assert got["filter"].shape == got["autocorr"].shape == got["crosscorr"].shape == (2, taps) and got["sdr_db"].shape == (2,)
    assert got["sdr_db"].dtype == got["filter"].dtype == np.float64 and got["valid"].dtype == np.int32
    for i in range(2):
        assert want[i]["valid"] == 1, (taps, n, i)  # the oracle shows the case valid
        assert int(got["valid"][i]) == 1
        for key in VECTORS:
            assert same(got[key][i], want[i][key]), (key, i)
        for key, name in SCALARS:
            assert same(got[key][i:i + 1], np.array([want[i][name]])), (key, i, float(got[key][i]), want[i][name])


# ---- 2. exact without the oracle's order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lags", [(1, 4), (200, 64), (100, 256), (2500, 300), (4100, 1024)])
def test_integer_samples_give_the_integer_sums_exactly(n, lags):
    rng = np.random.default_rng(n)
    u = rng.integers(-8, 9, (2, n)).astype(np.float32)
    v = rng.integers(-8, 9, (2, n)).astype(np.float32)
    lens = [n, max(1, n - n // 3)]
    got = cpu(l3ac_amd.correlate(torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV), lags, lengths=lens))
    assert got.shape == (2, lags) and got.dtype == np.float64
    for i, m in enumerate(lens):
        a, b = u[i, :m].astype(np.int64), v[i, :m].astype(np.int64)
        want = np.array([(a[:m - k] * b[k:]).sum() if k < m else 0 for k in range(lags)])
        assert np.array_equal(got[i], want.astype(np.float64)), i
        assert same(got[i, m:], np.zeros(max(lags - m, 0)))  # lags at and after the length are +0


# ---- 3. identities that hold bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps,n", [(64, 1500), (512, 300), (1024, 5000)])
def test_a_clip_against_itself_and_against_its_double(taps, n):
    x = dev(R.resonator(n, seed=5), R.white(n, seed=6))
    for scale in (1.0, 2.0):
        got = l3ac_amd.sdr(x, scale * x, filter_length=taps, return_filter=True)
        delta = torch.zeros(2, taps, dtype=torch.float64)
        delta[:, 0] = scale
        assert same(got["sdr_db"], torch.full((2,), float("inf"), dtype=torch.float64)), scale
        assert same(got["error_energy"], torch.zeros(2, dtype=torch.float64)) and (got["target_energy"] > 0).all()
        assert same(got["filter"], delta), scale  # lambda is exactly 0 at every step: +0 everywhere else, not -0
        assert cpu(got["valid"]).tolist() == [1, 1]


# ---- 4. the log stage -----------------------------------------------------------------------------------------------------------------------------
def test_sdr_db_is_within_three_ulps_of_the_oracle():
    """T / D is a bit-exact quotient; 10 log10 of it: 2U for two logs each within 1 ulp of the truth, U for the product (section 3.21)."""
    worst = 0.0
    for taps, n in [(1, 4096), (2, 63), (63, 64), (64, 9000), (65, 200), (512, 300), (512, 3586), (1024, 3073)]:
        want, got = case_oracle(taps, n), case_device(taps, n)
        for i in range(2):
            err, bound = abs(float(got["sdr_db"][i]) - want[i]["sdr_db"]), 3.0 * R.U * abs(want[i]["sdr_db"])
            print(f"L {taps} n {n} pair {i}: sdr_db {want[i]['sdr_db']:.6f}, error {err:.3g}, bound {bound:.3g}")
            assert np.isfinite(want[i]["sdr_db"]) and bound > 0.0
            assert err <= bound, (taps, n, i, err, bound)
            worst = max(worst, err / bound)
    print(f"worst observed error over the derived bound: {worst:.3f}")


# ---- 5. invalid pairs, the loading ---------------------------------------------------------------------------------------------------------------
def test_an_indefinite_system_is_invalid_and_its_batch_neighbours_are_unchanged():
    taps = 96
    s0, s2 = R.resonator(800, seed=1), R.white(800, seed=2)
    r = np.stack([R.correlate(s0, s0, taps), np.zeros(taps), R.correlate(s2, s2, taps)])
    r[1, :2] = [1.0, 2.0]  # k_1 = -2: E_1 = 1 - 4 < 0
    b = np.stack([R.correlate(s0, R.distorted(s0, 3), taps), np.ones(taps), R.correlate(s2, R.distorted(s2, 4), taps)])
    got = l3ac_amd.toeplitz_solve(torch.from_numpy(r).to(DEV), torch.from_numpy(b).to(DEV))
    assert set(got) == {"x", "error", "valid"} and got["x"].shape == (3, taps) and got["valid"].dtype == torch.int32
    assert cpu(got["valid"]).tolist() == [1, 0, 1]
    assert np.isnan(cpu(got["x"][1])).all() and np.isnan(cpu(got["error"][1]))
    for i in (0, 2):
        alone = l3ac_amd.toeplitz_solve(torch.from_numpy(r[i:i + 1]).to(DEV), torch.from_numpy(b[i:i + 1]).to(DEV))
        want = R.toeplitz_solve(r[i], b[i])
        assert same(got["x"][i], alone["x"][0]) and same(got["error"][i:i + 1], alone["error"])
        assert same(got["x"][i], want["x"]) and same(got["error"][i:i + 1], np.array([want["error"]]))


def test_silent_reference_silent_estimate_and_the_loading():
    n, taps = 700, 48
    s = R.resonator(n, seed=9)
    est = R.distorted(s, seed=10)
    zero = np.zeros(n, dtype=np.float32)
    got = l3ac_amd.sdr(dev(zero, s, s), dev(est, zero, est), filter_length=taps, return_filter=True)
    assert cpu(got["valid"]).tolist() == [0, 1, 1]
    for key in ("sdr_db", "target_energy", "error_energy", "prediction_error", "filter"):  # a silent reference: invalid, NaN ...
        assert np.isnan(cpu(got[key][0])).all(), key
    assert same(got["autocorr"][0], np.zeros(taps)) and same(got["crosscorr"][0], np.zeros(taps))  # ... and its r and b are kept
    assert float(got["target_energy"][1]) == 0.0 and float(got["error_energy"][1]) == 0.0 and np.isnan(float(got["sdr_db"][1]))  # 0 / 0
    assert float(got["prediction_error"][1]) > 0.0 and not np.isnan(cpu(got["filter"][1])).any()
    plain = R.sdr(s, est, taps)
    assert abs(float(got["sdr_db"][2]) - plain["sdr_db"]) <= 3.0 * R.U * abs(plain["sdr_db"])
    loaded = l3ac_amd.sdr(dev(s), dev(est), filter_length=taps, load=1e-3, return_filter=True)
    want = R.sdr(s, est, taps, load=1e-3)
    assert want["valid"] == 1 and want["autocorr"][0] == plain["autocorr"][0] * (1.0 + 1e-3)
    for key in VECTORS:
        assert same(loaded[key][0], want[key]), key
    for key, name in SCALARS:
        assert same(loaded[key], np.array([want[name]])), key
    assert abs(float(loaded["sdr_db"][0]) - want["sdr_db"]) <= 3.0 * R.U * abs(want["sdr_db"]) and want["sdr_db"] < plain["sdr_db"]


# ---- 6. ragged batches and independence -------------------------------------------------------------------------------------------------------------
def test_a_pair_does_not_depend_on_its_batch_row_strides_scratch_or_what_follows_it():
    taps = 64
    lens = [1500, 733, 1, 64]
    t = max(lens)
    ref = np.stack([R.resonator(t, seed=30 + i) for i in range(4)])
    est = np.stack([R.distorted(ref[i], seed=50 + i) for i in range(4)])
    alone = [l3ac_amd.sdr(dev(ref[i, :m]), dev(est[i, :m]), filter_length=taps, return_filter=True) for i, m in enumerate(lens)]
    alone_corr = [l3ac_amd.correlate(dev(ref[i, :m]), dev(est[i, :m]), taps) for i, m in enumerate(lens)]
    junk_r, junk_e = ref.copy(), est.copy()
    for i, m in enumerate(lens):
        junk_r[i, m:] = np.nan
        junk_e[i, m:] = np.inf
    wide_r = torch.full((4, t + 37), float("nan"), device=DEV)
    wide_e = torch.full((4, t + 37), float("nan"), device=DEV)
    wide_r[:, 5:5 + t] = torch.from_numpy(junk_r).to(DEV)
    wide_e[:, 9:9 + t] = torch.from_numpy(junk_e).to(DEV)
    view_r, view_e = wide_r[:, 5:5 + t], wide_e[:, 9:9 + t]  # non-contiguous row views, NaN / inf after every length
    assert not view_r.is_contiguous()
    batch = l3ac_amd.sdr(view_r, view_e, filter_length=taps, lengths=lens, return_filter=True, extra_scratch=4096 + 256)
    batch_corr = l3ac_amd.correlate(view_r, view_e, taps, lengths=lens, extra_scratch=1 << 16)
    for i in range(4):
        for key in batch:
            assert same(batch[key][i:i + 1], alone[i][key]), (key, i)
        assert same(batch_corr[i:i + 1], alone_corr[i]) and same(batch_corr[i], batch["crosscorr"][i]), i
    assert cpu(batch["valid"]).tolist() == [1, 1, 1, 1] and torch.isfinite(batch["sdr_db"][[0, 1, 3]]).all()
    assert float(batch["sdr_db"][2]) == float("inf")  # one sample is always a multiple of one sample


# ---- 7. composition -------------------------------------------------------------------------------------------------------------------------------
def test_sdr_is_correlate_then_toeplitz_solve_then_the_oracles_residual():
    n, taps = 3000, 200
    s = np.stack([R.resonator(n, seed=70), R.white(n, seed=71)])
    est = np.stack([R.distorted(s[0], seed=72), R.distorted(s[1], seed=73)])
    ds, de = torch.from_numpy(s).to(DEV), torch.from_numpy(est).to(DEV)
    got = l3ac_amd.sdr(ds, de, filter_length=taps, return_filter=True)
    r, b = l3ac_amd.correlate(ds, ds, taps), l3ac_amd.correlate(ds, de, taps)
    assert same(got["autocorr"], r) and same(got["crosscorr"], b)
    sol = l3ac_amd.toeplitz_solve(r, b)
    assert same(got["filter"], sol["x"]) and same(got["prediction_error"], sol["error"]) and same(got["valid"], sol["valid"])
    for i in range(2):
        t_want, d_want, _, _ = R.residual(s[i], est[i], cpu(sol["x"][i]))  # on the device's own filter
        assert same(got["target_energy"][i:i + 1], np.array([t_want])) and same(got["error_energy"][i:i + 1], np.array([d_want])), i
        db = 10.0 * np.log10(t_want / d_want)
        assert abs(float(got["sdr_db"][i]) - db) <= 3.0 * R.U * abs(db)
    short = l3ac_amd.sdr(ds, de, filter_length=taps)
    assert set(short) == {"sdr_db", "target_energy", "error_energy", "prediction_error", "valid"}
    for key in short:
        assert same(short[key], got[key]), key


@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_with_sdr_equals_the_composed_calls(codec):
    lens = [16000, 14400]
    audio = torch.zeros(2, 16000)
    for i, m in enumerate(lens):
        audio[i, :m] = torch.from_numpy(R.resonator(m, seed=600 + i))
    audio = audio.to(DEV)
    kw = dict(process_window=5400, prefix_tokens=3)  # several chunks each
    result = codec.evaluate(audio, lengths=lens, sdr=True, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :16000]
    composed = l3ac_amd.sdr(audio, decoded, lengths=lens)
    assert same(result["sdr_db"], composed["sdr_db"]) and same(result["sdr_valid"], composed["valid"]) and result["sdr_db"].is_cuda
    assert cpu(result["sdr_valid"]).tolist() == [1, 1] and torch.isfinite(result["sdr_db"]).all()
    today = {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
    assert set(result) == today | {"sdr_db", "sdr_valid"}
    assert set(codec.evaluate(audio, lengths=lens, **kw)) == today


# ---- 9. isolation ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_a_corrupt_pair_stays_alone(pattern):
    n, taps = 1500, 64
    lens = [1500, 1100, 900]
    ref = np.stack([R.resonator(n, seed=90 + i) for i in range(3)])
    est = np.stack([R.distorted(ref[i], seed=95 + i) for i in range(3)])
    pairs = torch.from_numpy(np.stack([ref, est], axis=1)).to(DEV)  # (3, 2, n): a pair's two sides are rows of one clip
    run_sdr = lambda q: l3ac_amd.sdr(q[:, 0], q[:, 1], filter_length=taps, lengths=lens, return_filter=True)
    clean, bad = poison.twin_check(run_sdr, pairs, [1], pattern, what="sdr")
    assert cpu(clean["valid"]).tolist() == [1, 1, 1] and int(bad["valid"][0]) == 1 and int(bad["valid"][2]) == 1
    poison.twin_check(lambda q: l3ac_amd.correlate(q[:, 0], q[:, 1], taps, lengths=lens), pairs, [1], pattern, what="correlate")
    r, b = clean["autocorr"], clean["crosscorr"]
    systems = torch.stack([r, b], dim=1)
    poison.twin_check(lambda q: l3ac_amd.toeplitz_solve(q[:, 0], q[:, 1]), systems, [1], pattern, what="toeplitz_solve")
