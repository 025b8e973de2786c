"""EBU R128 on the MI355X (kernels/true_peak.hip, kernels/loudness.hip) against the library's own resample and
loudness, bit for bit, and against the fp64 oracle (tests/r128_ref.py): the true peak at every tile and halo edge, the block series of any
window, the loudness range with its gates and picks, invariance over batch / row / stride / scratch, isolation from non-finite neighbours,
graph capture (true_peak as a process' first call), normalize_loudness(peak="true") and codec.evaluate(r128=True) as compositions.

Every loudness range case first asserts on the ORACLE alone that no short-term block lies within 0.05 LU of either gate: the gate decisions
are then the same in any arithmetic that meets the energy bound, and order statistics are 1-Lipschitz in the values.

The figures measured on an MI355X are in the docstrings of the tests that print them."""
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import loudness_ref as L
from tests import poison
from tests import r128_ref as R
from tests.test_gpu_loudness import MARGIN, clip as loudness_clip, family, yardstick as loudness_yardstick
from tests.test_gpu_resample import EPS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
STEP = FS // 10
TILE = _capi.load_library().l3ac_true_peak_tile()
TAPS = 21


# ---- 1. true peak, bit for bit against the library's own resample -------------------------------------------------------------------------------
def peak_signals(n, seed):
    """(4, n) fp32: seeded noise; a unit impulse at sample 0, at the last sample of a tile (of the clip, where it is shorter) and at the
    clip's last sample."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(4, n)
    x[0] = 0.3 * torch.randn(n, generator=g)
    x[1, 0] = 1.0
    x[2, min(TILE, n) - 1] = -1.0
    x[3, n - 1] = 1.0
    if (n - 1) // TILE > 1:
        x[2, (n - 1) // TILE * TILE - 1] = 0.75  # and at the last sample of the clip's last whole tile
    return x


def composed_true_peak(row, fs):
    """max(amax |x|, amax |resample(x alone, fs, L fs)|) of one clip on the device, widened to fp64."""
    up = l3ac_amd.true_peak_factor(fs)
    y = l3ac_amd.resample(row[None], fs, up * fs)
    assert y.shape == (1, up * row.shape[0])
    return torch.maximum(row.abs().amax(), y.abs().amax()).double(), row.abs().amax().double()


@pytest.mark.parametrize("fs", [8000, 96000])
def test_true_peak_is_the_maximum_of_the_librarys_own_resample(fs):
    assert l3ac_amd.true_peak_factor(fs) == (4 if fs == 8000 else 2)
    for n in (1, 20, 21, 22, TILE - 1, TILE, TILE + 1, 3 * TILE + 7):
        x = peak_signals(n, seed=n + fs).to(DEV)
        got = l3ac_amd.true_peak(x, fs)
        assert all(got[k].dtype == torch.float64 and got[k].shape == (4,) and got[k].is_cuda for k in ("true_peak", "true_peak_db", "peak"))
        for i in range(4):
            want, peak = composed_true_peak(x[i], fs)
            assert torch.equal(got["true_peak"][i], want), (fs, n, i, float(got["true_peak"][i]), float(want))
            assert torch.equal(got["peak"][i], peak), (fs, n, i)
        assert torch.equal(got["true_peak_db"], 20.0 * torch.log10(got["true_peak"]))
        assert (got["true_peak"][1:] >= 1.0).all()  # an impulse: the centre tap of phase 0 is the sample itself, or nearly
    silent = l3ac_amd.true_peak(torch.zeros(2, 100, device=DEV), fs)
    assert not silent["true_peak"].any() and not silent["peak"].any() and (silent["true_peak_db"] == -np.inf).all()


# ---- 2. true peak against fp64 -----------------------------------------------------------------------------------------------------------------
def quarter_rate_sine(n=2000):
    """A sine at fs / 4, amplitude 0.5, sampled 45 degrees off its crests: every sample is 0.35355 in magnitude."""
    return (0.5 * np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4)).astype(np.float32)


@pytest.mark.parametrize("name", ["noise:8000", "noise:96000", "sine:16000"])
def test_true_peak_within_the_fp32_dot_bound_of_the_oracle(name):
    """|max_m |y_m| - max_m |ref_m|| <= max_m |y_m - ref_m| <= max_m (K + 2) 2^-24 sum |h x|, the bound of tests/test_gpu_resample.py; the sample
    peak is exact.  Measured on an MI355X: 7.2e-8, 8.0e-8 and 6.9e-8 against bounds of 1.7e-6, 1.9e-6 and 1.1e-6."""
    kind, _, fs = name.partition(":")
    fs = int(fs)
    x = quarter_rate_sine() if kind == "sine" else peak_signals(3 * TILE + 7, seed=fs)[0].numpy()
    o = R.true_peak(x, fs)
    got = l3ac_amd.true_peak(torch.from_numpy(x)[None].to(DEV), fs)
    bound = float(np.max((TAPS + 2) * EPS * o["absdot"]))
    err = abs(float(got["true_peak"][0]) - o["true_peak"])
    print(f"\n[r128] true peak {name}: oracle {o['true_peak']:.7f}, GPU |err| = {err:.3e}, bound {bound:.3e}")
    assert float(got["peak"][0]) == o["peak"] and bound > 0 and err <= bound
    if kind == "sine":  # the motivating case: the samples miss the crests by 3 dB
        assert abs(o["peak"] - 0.35355) < 1e-5 and abs(o["true_peak"] - 0.5067) < 1e-4
        assert float(got["true_peak"][0]) / float(got["peak"][0]) > 1.4


# ---- 3. the block series ----------------------------------------------------------------------------------------------------------------------------
SERIES_LENS = (30 * STEP - 1, 30 * STEP, 30 * STEP + 1, 31 * STEP)


@functools.lru_cache(maxsize=None)
def series_clips():
    """The short clips at the short-term block-count edges (K = 0, 1, 1, 2) and the 130-step clip of the loudness suite, at 8 kHz."""
    base = (0.5 * family(31 * STEP, FS, 41)).astype(np.float32)
    return [base[:n].copy() for n in SERIES_LENS] + [loudness_clip("long")[0]]


@functools.lru_cache(maxsize=None)
def series_batch():
    clips = series_clips()
    lens = [c.shape[0] for c in clips]
    rows = torch.full((len(clips), max(lens) + 5), 1e30)
    rows[:, 1::2] = float("nan")
    for i, c in enumerate(clips):
        rows[i, :lens[i]] = torch.from_numpy(c)
    return rows.to(DEV)[:, :max(lens)], lens


def test_momentary_series_is_the_meters_own():
    x, lens = series_batch()
    meter = l3ac_amd.loudness(x, FS, lengths=lens, return_momentary=True)
    got = l3ac_amd.short_term_loudness(x, FS, lengths=lens, window=0.4)
    assert set(got) == {"lufs", "blocks"} and got["lufs"].dtype == torch.float64 and got["blocks"].dtype == torch.int32
    assert torch.equal(got["lufs"], meter["momentary"]) and torch.equal(got["blocks"], meter["blocks"])
    assert torch.isfinite(got["lufs"][4]).all() and got["lufs"].shape == (5, 127)


@pytest.mark.parametrize("steps", [1, 4, 30])
def test_series_is_the_left_to_right_sum_of_the_step_energies(steps):
    x, lens = series_batch()
    got = l3ac_amd.short_term_loudness(x, FS, lengths=lens, window=steps / 10.0, return_parts=True)
    assert set(got) == {"lufs", "blocks", "mean_square", "energies"}
    k_max = 130 - steps + 1
    assert got["lufs"].shape == got["mean_square"].shape == (5, k_max) and got["energies"].shape == (5, 130)
    ms, en, lufs = (got[k].cpu().numpy() for k in ("mean_square", "energies", "lufs"))
    for i, n in enumerate(lens):
        s, k = n // STEP, R.block_count(n, FS, steps)
        assert int(got["blocks"][i]) == k
        assert np.array_equal(ms[i, :k], R.left_to_right(en[i, :s], steps, STEP)) and not ms[i, k:].any() and not en[i, s:].any(), (steps, i)
        assert (en[i, :s] > 0).all() and (lufs[i, k:] == -np.inf).all()
        assert np.abs(lufs[i, :k] - L.lkfs(ms[i, :k])).max(initial=0.0) <= 1e-9
    if steps == 30:
        assert [R.block_count(n, FS, 30) for n in lens] == [0, 1, 1, 2, 101]


@functools.lru_cache(maxsize=None)
def series_yardstick(i):
    return loudness_yardstick("long") if i == 4 else L.yardstick(series_clips()[i], FS)


def test_step_energies_within_four_times_what_fp64_costs():
    """The rule of tests/test_gpu_loudness.py on the energies themselves: relative to the fp64 oracle's, within 4 E of the clip.  Measured on
    an MI355X: E = 2.2e-15 and the GPU at 0.90 E on the short clips, E = 4.7e-15 and 1.02 E on the 130-step clip."""
    x, lens = series_batch()
    en = l3ac_amd.short_term_loudness(x, FS, lengths=lens, window=3.0, return_parts=True)["energies"].cpu().numpy()
    for i, c in enumerate(series_clips()):
        want = L.energies64(c, FS)
        e = series_yardstick(i)
        err = float(np.max(np.abs(en[i, :want.size] - want) / want))
        print(f"\n[r128] clip {i} ({want.size} steps): E = {e:.3e}, GPU worst relative energy error {err:.3e}, ratio {err / e:.3f}")
        assert e > 0 and err <= 4 * e


# ---- 4. loudness range --------------------------------------------------------------------------------------------------------------------------
RANGE_CASES = {"G1": ((-10.0, -22.0, -50.0, -95.0), 1), "G2": ((-95.0, -6.0, -45.0, -18.0), 1), "G3": ((-30.0, -55.0, -12.0, -100.0), 2)}
RANGE_COUNTS = {"G1": (161, 140, 100), "G2": (161, 140, 117), "G3": (161, 129, 122)}  # blocks, above the absolute gate, gated


@functools.lru_cache(maxsize=None)
def range_clip(name):
    """19 s of 0.5 family(22 s at 8 kHz, seed): sections of 5, 5, 5 and 4 s at the case's levels in dB."""
    levels, seed = RANGE_CASES[name]
    x = 0.5 * family(22 * FS, FS, seed)[:19 * FS]
    for (a, b), level in zip(((0, 5), (5, 10), (10, 15), (15, 19)), levels):
        x[a * FS:b * FS] *= 10.0 ** (level / 20.0)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def range_oracle(name):
    return R.loudness_range(range_clip(name), FS)


def restated_range(ms):
    """Tech 3342 in numpy fp64 on the library's own short-term mean squares -> (low, high, above_absolute, gated)."""
    l = L.lkfs(ms)
    absolute = l > L.ABS_GATE
    if not absolute.any():
        return -np.inf, -np.inf, 0, 0
    gamma = float(L.lkfs(np.sum(ms[absolute]) / absolute.sum())) - 20.0
    passing = absolute & (l > gamma)
    low, high = R.picks(ms[passing])
    return low, high, int(absolute.sum()), int(passing.sum())


def run_range(x, fs=FS):
    x = torch.from_numpy(x)[None].to(DEV)
    got = l3ac_amd.loudness_range(x, fs)
    assert all(got[k].dtype == torch.float64 for k in ("lra", "low_lufs", "high_lufs", "short_term_max", "momentary_max"))
    assert all(got[k].dtype == torch.int32 for k in ("blocks", "above_absolute", "gated")) and all(v.shape == (1,) and v.is_cuda for v in got.values())
    parts = l3ac_amd.short_term_loudness(x, fs, window=3.0, return_parts=True)
    return {k: v[0].cpu().numpy() for k, v in got.items()}, parts


@pytest.mark.parametrize("name", sorted(RANGE_CASES))
def test_loudness_range_of_the_level_steps(name):
    """Measured on an MI355X: 16.037206, 15.343664 and 19.753792 LU, the oracle's own fp64 values, and the picks the restated ones bit for
    bit; E = 7.2e-14, 1.4e-13 and 1.1e-14."""
    o = range_oracle(name)
    assert o["abs_margin"] >= MARGIN, f"{name}: a block lies {o['abs_margin']:.3f} LU from the absolute gate"
    assert o["rel_margin"] >= MARGIN, f"{name}: a block lies {o['rel_margin']:.3f} LU from the relative gate"
    assert (o["blocks"], o["above_absolute"], o["gated"]) == RANGE_COUNTS[name]
    got, parts = run_range(range_clip(name))
    assert (int(got["blocks"]), int(got["above_absolute"]), int(got["gated"])) == RANGE_COUNTS[name]
    ms = parts["mean_square"][0].cpu().numpy()
    low, high, above, gated = restated_range(ms)
    assert (above, gated) == RANGE_COUNTS[name][1:]
    e = L.yardstick(range_clip(name), FS)
    slack = 10.0 * np.log10((1 + 4 * e) / (1 - 4 * e)) + 2e-9
    print(f"\n[r128] {name}: oracle LRA {o['lra']:.6f} LU, GPU {float(got['lra']):.6f}, |err| = {abs(float(got['lra']) - o['lra']):.3e} (E = {e:.3e}, "
          f"allowed {slack:.3e}); picks off the restated ones by {abs(float(got['low_lufs']) - low):.1e}, {abs(float(got['high_lufs']) - high):.1e} dB")
    assert abs(float(got["low_lufs"]) - low) <= 1e-9 and abs(float(got["high_lufs"]) - high) <= 1e-9
    assert abs(float(got["lra"]) - (high - low)) <= 2e-9
    assert abs(float(got["lra"]) - o["lra"]) <= slack
    assert abs(float(got["short_term_max"]) - float(parts["lufs"].max())) == 0.0 and abs(float(got["short_term_max"]) - o["short_term_max"]) <= 1e-6
    mom = l3ac_amd.loudness(torch.from_numpy(range_clip(name))[None].to(DEV), FS, return_momentary=True)["momentary"]
    assert float(got["momentary_max"]) == float(mom.max()) and abs(float(got["momentary_max"]) - o["momentary_max"]) <= 1e-6


def test_loudness_range_without_a_gated_block():
    for x in (np.zeros(5 * FS, dtype=np.float32), range_clip("G1")[:30 * STEP - 1], np.full(4 * FS, 1e-6, dtype=np.float32)):
        got, _ = run_range(x)
        assert int(got["blocks"]) == R.block_count(x.shape[0], FS, 30) and int(got["gated"]) == 0 and int(got["above_absolute"]) == 0
        assert float(got["lra"]) == 0.0 and not np.signbit(got["lra"]) and float(got["low_lufs"]) == float(got["high_lufs"]) == -np.inf
    silent, _ = run_range(np.zeros(5 * FS, dtype=np.float32))
    assert float(silent["short_term_max"]) == float(silent["momentary_max"]) == -np.inf and int(silent["blocks"]) == 21
    short, _ = run_range(range_clip("G1")[:30 * STEP - 1])
    assert float(short["short_term_max"]) == -np.inf and np.isfinite(float(short["momentary_max"])) and int(short["blocks"]) == 0


def test_loudness_range_of_one_and_two_blocks():
    base = range_clip("G2")[5 * FS:]  # from the -6 dB section on
    for n, g in ((30 * STEP, 1), (31 * STEP - 1, 1), (31 * STEP, 2)):
        o = R.loudness_range(base[:n], FS)
        assert o["gated"] == g and min(o["abs_margin"], o["rel_margin"]) >= MARGIN
        got, parts = run_range(base[:n])
        ms = parts["mean_square"][0].cpu().numpy()
        assert int(got["blocks"]) == int(got["above_absolute"]) == int(got["gated"]) == g == ms.size
        assert abs(float(got["low_lufs"]) - L.lkfs(ms.min())) <= 1e-9 and abs(float(got["high_lufs"]) - L.lkfs(ms.max())) <= 1e-9
        assert float(got["lra"]) == float(got["high_lufs"]) - float(got["low_lufs"]) and (g == 2 or float(got["lra"]) == 0.0)
        assert abs(float(got["lra"]) - o["lra"]) <= 1e-9


def test_loudness_range_takes_16384_blocks_and_refuses_one_more():
    x = torch.zeros(1, (16385 + 29) * STEP, device=DEV)
    got = l3ac_amd.loudness_range(x[:, :(16384 + 29) * STEP], FS)
    assert int(got["blocks"]) == 16384 and int(got["gated"]) == 0 and float(got["lra"]) == 0.0 and float(got["short_term_max"]) == -np.inf
    assert int(l3ac_amd.loudness_range(x, FS, lengths=[(16384 + 29) * STEP + STEP - 1])["blocks"]) == 16384  # its own length decides
    with pytest.raises(_capi.L3acError, match="16385 short-term blocks are more than the 16384"):
        l3ac_amd.loudness_range(x, FS)


# ---- 5. invariance, bit for bit -----------------------------------------------------------------------------------------------------------------
RAGGED_LENS = [40 * STEP, 35 * STEP + 123, 30 * STEP + 1]


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """Three clips of 4, 3.5 and 3 s in rows of 4 s + 37 samples, 1e30 and NaN after every length."""
    width = RAGGED_LENS[0] + 37
    rows = torch.full((3, width), 1e30)
    rows[:, 1::2] = float("nan")
    clips = []
    for i, (name, n) in enumerate(zip(("G1", "G2", "G3"), RAGGED_LENS)):
        start = (3, 5, 9)[i] * FS  # stretches that cross a level step
        c = torch.from_numpy(range_clip(name)[start:start + n].copy())
        clips.append(c)
        rows[i, :n] = c
    return rows, clips


def everything(x, lengths=None):
    """The three entries' results as one flat dict of tensors whose axis 0 is the clip."""
    out = {f"tp.{k}": v for k, v in l3ac_amd.true_peak(x, FS, lengths=lengths).items()}
    out.update({f"st.{k}": v for k, v in l3ac_amd.short_term_loudness(x, FS, lengths=lengths, window=3.0, return_parts=True).items()})
    out.update({f"mo.{k}": v for k, v in l3ac_amd.short_term_loudness(x, FS, lengths=lengths, window=0.4).items()})
    out.update({f"lra.{k}": v for k, v in l3ac_amd.loudness_range(x, FS, lengths=lengths).items()})
    return out


def through_the_abi(x, lens, factor):
    """The same through the C entries, with `factor` times the minimum scratch."""
    lib = _capi.load_library()
    b, t = x.shape
    c_lens = (_capi.C.c_int32 * b)(*lens)
    stream = torch.cuda.current_stream().cuda_stream
    s_max = t // STEP
    out = {}
    need = lib.l3ac_true_peak_scratch_bytes(b, t, FS) * factor
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    stats = torch.empty((b, 2), dtype=torch.float64, device=DEV)
    _capi.check(lib.l3ac_true_peak(x.data_ptr(), x.stride(0), b, t, c_lens, FS, stats.data_ptr(), scratch.data_ptr(), need, stream))
    out["tp.true_peak"], out["tp.peak"] = stats[:, 0], stats[:, 1]
    need = lib.l3ac_r128_scratch_bytes(b, t, FS) * factor
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    for tag, w in (("st", 30), ("mo", 4)):
        k_max = s_max - w + 1
        lufs, ms = (torch.empty((b, k_max), dtype=torch.float64, device=DEV) for _ in range(2))
        en = torch.empty((b, s_max), dtype=torch.float64, device=DEV)
        blocks = torch.empty((b,), dtype=torch.int32, device=DEV)
        _capi.check(lib.l3ac_r128_series(x.data_ptr(), x.stride(0), b, t, c_lens, FS, w, lufs.data_ptr(), ms.data_ptr(), en.data_ptr(), blocks.data_ptr(),
                                         scratch.data_ptr(), need, stream))
        out[f"{tag}.lufs"], out[f"{tag}.blocks"] = lufs, blocks
        if tag == "st":
            out["st.mean_square"], out["st.energies"] = ms, en
    stats = torch.empty((b, 5), dtype=torch.float64, device=DEV)
    counts = torch.empty((b, 3), dtype=torch.int32, device=DEV)
    _capi.check(lib.l3ac_r128_range(x.data_ptr(), x.stride(0), b, t, c_lens, FS, stats.data_ptr(), counts.data_ptr(), scratch.data_ptr(), need, stream))
    for i, k in enumerate(("lra", "low_lufs", "high_lufs", "short_term_max", "momentary_max")):
        out[f"lra.{k}"] = stats[:, i]
    for i, k in enumerate(("blocks", "above_absolute", "gated")):
        out[f"lra.{k}"] = counts[:, i]
    return out


def test_bits_do_not_depend_on_batch_row_stride_or_scratch():
    rows, clips = ragged_batch()
    lens, t = RAGGED_LENS, RAGGED_LENS[0]
    alone = [everything(c[None].to(DEV)) for c in clips]
    for a in alone:
        assert int(a["lra.gated"]) >= 1 and torch.isfinite(a["lra.lra"]).all() and float(a["tp.true_peak"]) > 0
    assert [int(a["lra.blocks"]) for a in alone] == [11, 6, 1]
    wide = rows.to(DEV)
    strided = wide[:, :t]
    assert strided.stride(0) == t + 37
    results = {"strided": everything(strided, lens), "contiguous": everything(strided.contiguous(), lens), "wide": everything(wide, lens),
               "minimum scratch": through_the_abi(strided, lens, 1), "twice the minimum": through_the_abi(strided, lens, 2)}
    pad = {"st.lufs": -np.inf, "mo.lufs": -np.inf, "st.mean_square": 0.0, "st.energies": 0.0}
    for what, got in results.items():
        for key, value in got.items():
            for i in range(3):
                want = alone[i][key][0]
                if key in pad:
                    k = want.shape[0]
                    assert torch.equal(value[i, :k], want) and (value[i, k:] == pad[key]).all(), (what, key, i)
                else:
                    assert torch.equal(value[i], want), (what, key, i)
    flipped = everything(strided.flip(0), lens[::-1])
    for key, value in flipped.items():
        assert torch.equal(value, results["strided"][key].flip(0)), key


@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_non_finite_clips_leave_their_neighbours_alone(pattern):
    rows, _ = ragged_batch()
    batch = rows.to(DEV)[:, :RAGGED_LENS[0]].contiguous()

    def finite_part(x):
        out = everything(x, RAGGED_LENS)
        return {k: v for k, v in out.items() if k not in ("st.lufs", "mo.lufs")}  # (-inf after a clip's own blocks: compared below)

    poison.twin_check(finite_part, batch, [1], pattern, extent=RAGGED_LENS, what="r128")
    poison.twin_check(lambda x: {k: v for k, v in everything(x, RAGGED_LENS).items() if k in ("st.lufs", "mo.lufs")}, batch, [0, 2], pattern,
                      extent=RAGGED_LENS, finite=False, what="r128 series")


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------------------
def test_true_peak_is_capturable_as_the_first_call_of_a_process():
    """No table, no upload: a fresh process captures true_peak before anything else has run."""
    script = Path(__file__).resolve().parent / "capture_cold_true_peak.py"
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "captured as the first call; bits equal True true peak above the peak True replay follows the input True" in r.stdout, r.stdout[-2000:]


def test_loudness_range_graph_replays_the_eager_bits():
    rows, _ = ragged_batch()
    x = rows.to(DEV)[:, :RAGGED_LENS[0]]
    eager = l3ac_amd.loudness_range(x, FS, lengths=RAGGED_LENS)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = l3ac_amd.loudness_range(x, FS, lengths=RAGGED_LENS)
        series = l3ac_amd.short_term_loudness(x, FS, lengths=RAGGED_LENS)
    graph.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(got[k], v), k
    assert torch.equal(series["lufs"], l3ac_amd.short_term_loudness(x, FS, lengths=RAGGED_LENS)["lufs"])
    assert (eager["lra"] > 1.0).any() and (eager["gated"] >= 1).all()


# ---- 7. compositions ----------------------------------------------------------------------------------------------------------------------------
TARGET = 6.0  # LUFS: more than a full-scale signal reaches


def test_normalize_to_a_true_peak_limit_is_the_composition():
    """The target lies above what either limit allows, so the limit decides the gain in both modes.  Measured on an MI355X: the true peak
    after is -0.9999997 dBTP on both clips; limited on the sample peak the fs / 4 sine comes out about 3 dB above -1 dBTP."""
    fs = 16000
    sine = torch.from_numpy(quarter_rate_sine(fs))
    other = torch.from_numpy((0.3 * family(fs, fs, 90)).astype(np.float32))
    x = torch.stack([sine, other]).to(DEV)
    lens = [fs, fs - 1234]
    out, info = l3ac_amd.normalize_loudness(x, target_lufs=TARGET, sample_rate=fs, lengths=lens, peak="true")
    stats = l3ac_amd.loudness(x, fs, lengths=lens)
    tp = l3ac_amd.true_peak(x, fs, lengths=lens)
    gain = l3ac_amd.loudness_gain({"lufs": stats["lufs"], "peak": tp["true_peak"]}, target_lufs=TARGET, peak_limit_db=-1.0)
    assert set(info) == {"lufs", "peak", "true_peak", "gain_db", "gain"}
    assert torch.equal(out, l3ac_amd.apply_gain(x, gain["gain"], lengths=lens))
    assert torch.equal(info["lufs"], stats["lufs"]) and torch.equal(info["peak"], stats["peak"]) and torch.equal(info["true_peak"], tp["true_peak"])
    assert torch.equal(info["gain_db"], gain["gain_db"]) and torch.equal(info["gain"], gain["gain"])
    after = l3ac_amd.true_peak(out, fs, lengths=lens)["true_peak_db"]
    sample_out, sample_info = l3ac_amd.normalize_loudness(x, target_lufs=TARGET, sample_rate=fs, lengths=lens)
    sample_after = l3ac_amd.true_peak(sample_out, fs, lengths=lens)["true_peak_db"]
    print(f"\n[r128] normalised to -1 dBTP: true peak after {[f'{v:+.7f}' for v in after.tolist()]} dBTP; with the sample-peak limit "
          f"{[f'{v:+.4f}' for v in sample_after.tolist()]} dBTP")
    assert set(sample_info) == {"lufs", "peak", "gain_db", "gain"}
    explicit, _ = l3ac_amd.normalize_loudness(x, target_lufs=TARGET, sample_rate=fs, lengths=lens, peak="sample")
    assert torch.equal(explicit, sample_out)
    assert (info["gain_db"] < TARGET - stats["lufs"]).all()  # the limit acts on both clips
    assert (after <= -1.0 + 1e-6).all()
    assert (sample_after > -1.0).all()
    # the samples of the fs / 4 sine miss its crests by 20 log10(0.5009 / 0.35355) = 3.03 dB (3.13 dB at the clip's edges)
    assert float(sample_after[0]) > -1.0 + 3.0


@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_with_r128_equals_the_composed_calls(codec):
    fs = codec.config.sample_rate
    lens = [4 * fs, 4 * fs + 4000]  # 11 and 13 short-term blocks
    audio = torch.zeros(2, lens[1])
    for i, n in enumerate(lens):
        c = 0.3 * family(n, fs, 700 + i)
        c[:2 * fs] *= 0.2  # a level step of 14 dB: the blocks' levels span 10 log10((2 + 0.04) / (1 + 0.08)) = 2.8 dB
        audio[i, :n] = torch.from_numpy(c.astype(np.float32))
    audio = audio.to(DEV)
    kw = dict(process_window=2700, prefix_tokens=3)
    got = codec.evaluate(audio, lengths=lens, r128=True, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :lens[1]]
    ref, dec = (l3ac_amd.loudness_range(s, sample_rate=fs, lengths=lens)["lra"] for s in (audio, decoded))
    assert torch.equal(got["lra_reference"], ref) and (ref > 1.0).all()
    assert torch.equal(got["lra_decoded"], dec) and torch.equal(got["lra_shift"], dec - ref) and got["lra_shift"].dtype == torch.float64
    for key, side in (("true_peak_reference_db", audio), ("true_peak_decoded_db", decoded)):
        assert torch.equal(got[key], l3ac_amd.true_peak(side, sample_rate=fs, lengths=lens)["true_peak_db"]), key
    assert torch.isfinite(got["true_peak_reference_db"]).all() and got["true_peak_reference_db"].is_cuda
    today = {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
    assert set(got) == today | {"lra_reference", "lra_decoded", "lra_shift", "true_peak_reference_db", "true_peak_decoded_db"}
    assert set(codec.evaluate(audio, lengths=lens, **kw)) == today
