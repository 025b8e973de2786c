"""YIN pitch tracking and the F0 metrics on the MI355X (kernels/pitch.hip) against the fp64 oracle (tests/pitch_ref.py, DESIGN.md section
3.15): the normalised difference within the derived bound beta of the oracle's, the tracks bit for bit the pick of the library's OWN
normalised difference, the voicing decisions and the voiced lags those of the oracle, what the tracker reads on signals whose pitch is
known, the shapes at which the kernel takes another path, bit invariance over batch / row / stride / scratch size / what lies after a
clip's length, the pair metrics, graph capture as the first pitch call of the process, and codec.evaluate(pitch=True) against the
hand-composed calls.

Every numeric case first asserts on the ORACLE alone (`conditions`) that every frame is robust: each comparison the pick makes keeps its
outcome under a relative error of beta in the normalised difference, so the decisions are the same in any arithmetic that meets the bound.
For a frame the oracle calls unvoiced only the threshold comparisons count; which of its near-equal minima the library takes is pinned
against the library's own row.  The seeds below satisfy it; a case that misses it fails, it is never skipped.

The clips are 2 s at 8 and 16 kHz (197 frames each, 96 of them voiced) and shorter ones at the edges.  The figures measured on an MI355X
are in the docstrings of the tests that print them."""
import functools

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import pitch_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0
RATES = (8000, 16000)
GROUP = 8    # frames of a frame group at the default parameters, and groups a workgroup walks (kernels/pitch.hip): the shapes of `EDGES`
WALK = 4


def bits(t):
    """A device tensor as integers: NaN rows compare like any other."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def track(x, fs, **kw):
    """The library on one clip alone -> numpy: f0, voiced, aperiodicity, cmnd (rows per frame), frames."""
    out = l3ac_amd.pitch(torch.from_numpy(np.ascontiguousarray(x))[None].to(DEV), sample_rate=fs, return_cmnd=True, **kw)
    assert out["f0"].dtype == out["aperiodicity"].dtype == out["cmnd"].dtype == torch.float64
    assert out["voiced"].dtype == out["frames"].dtype == torch.int32 and all(v.is_cuda for v in out.values())
    n = int(out["frames"][0])
    assert out["f0"].shape == out["voiced"].shape == out["aperiodicity"].shape == (1, n) and out["cmnd"].shape[:2] == (1, n)
    return {k: v[0].cpu().numpy() for k, v in out.items() if k != "frames"} | {"frames": n}


# ---- 8. graph capture: FIRST in this file, no other file of the suite calls pitch ---------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits_as_the_first_pitch_call():
    """There is no table to upload and no kernel to configure: the very first call may be the captured one."""
    a, b = R.clip(16000, SEED)[:20000], R.clip(16000, SEED + 1)[:20000]
    x = torch.from_numpy(np.stack((a, a))).to(DEV)
    y = torch.from_numpy(np.stack((b, a))).to(DEV)
    lens = [20000, 9001]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr = l3ac_amd.pitch(x, lengths=lens, return_cmnd=True)
        pm = l3ac_amd.pitch_metrics(x, y, lengths=lens)
    graph.replay()
    torch.cuda.synchronize()
    e_tr = l3ac_amd.pitch(x, lengths=lens, return_cmnd=True)
    e_pm = l3ac_amd.pitch_metrics(x, y, lengths=lens)
    assert e_tr["frames"].tolist() == [R.frames(n, R.lags(16000)) for n in lens] and int(e_tr["voiced"].sum()) > 40
    for k in e_tr:
        assert same(tr[k], e_tr[k]), k
    for k in e_pm:
        assert same(pm[k], e_pm[k]), k
    assert float(e_pm["f0_rmse_cents"][1]) == 0.0 and float(e_pm["f0_rmse_cents"][0]) > 0.0
    x.copy_(y)  # the replay reads the tensors' current contents
    graph.replay()
    torch.cuda.synchronize()
    again = l3ac_amd.pitch(y, lengths=lens, return_cmnd=True)
    for k in again:
        assert same(tr[k], again[k]), k
    assert float(pm["f0_rmse_cents"][0]) == 0.0 and float(pm["vde"][0]) == 0.0


# ---- the numeric cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip(fs):
    return R.clip(fs, SEED)


@functools.lru_cache(maxsize=None)
def want(fs, threshold=0.1):
    return R.oracle(clip(fs), fs, threshold=threshold)


@functools.lru_cache(maxsize=None)
def got(fs, threshold=0.1):
    return track(clip(fs), fs, threshold=threshold)


def conditions(o, name):
    """Every frame robust, on the oracle alone; a case that misses it fails (it is never skipped)."""
    bad = np.flatnonzero(~o["robust"])
    assert bad.size == 0, f"{name}: frames {bad.tolist()} of the oracle have a comparison within beta of its edge: change the seed"
    return o


def check_against_oracle(o, g, name):
    """Checks 1 to 3 of one clip -> the worst |c_library - c_oracle| / (beta c)."""
    geo, bt = o["g"], R.beta(o["g"])
    n = len(o["f0"])
    assert g["frames"] == n and g["cmnd"].shape == (n, geo["T"] + 1), name
    if n == 0:
        return 0.0
    # 1. the normalised difference: exact ones where S = 0 on both sides, within beta c elsewhere
    exact = np.concatenate((np.ones((n, 1), dtype=bool), np.cumsum(o["d"][:, 1:], axis=1) == 0.0), axis=1)
    assert (g["cmnd"][exact] == 1.0).all() and (o["cmnd"][exact] == 1.0).all(), name
    err = np.abs(g["cmnd"] - o["cmnd"])
    worst = float((err[~exact] / (bt * o["cmnd"][~exact])).max()) if (~exact).any() else 0.0
    assert (err <= bt * o["cmnd"]).all(), f"{name}: |c - c_oracle| is {worst:.3f} beta c"
    # 2. the tracks are the pick of the library's own row, bit for bit
    picks = [R.pick_from_cmnd(row, geo, o["threshold"]) for row in g["cmnd"]]
    assert np.array_equal(np.array([p[2] for p in picks]).view(np.int64), g["f0"].view(np.int64)), name
    assert np.array_equal(np.array([p[1] for p in picks], dtype=np.int32), g["voiced"]), name
    assert np.array_equal(np.array([p[3] for p in picks]).view(np.int64), g["aperiodicity"].view(np.int64)), name
    # 3. the decisions are the oracle's: voiced on every frame, the lag on the voiced ones
    star = np.array([p[0] for p in picks])
    assert np.array_equal(g["voiced"], o["voiced"]), f"{name}: voiced differs at frames {np.flatnonzero(g['voiced'] != o['voiced']).tolist()}"
    v = o["voiced"] == 1
    assert np.array_equal(star[v], o["tau"][v]), name
    return worst


def case(x, fs, name, threshold=0.1, **kw):
    o = R.oracle(x, fs, threshold=threshold, **kw)
    o["threshold"] = threshold
    conditions(o, name)
    return o, check_against_oracle(o, track(x, fs, threshold=threshold, **kw), name)


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("threshold", (0.1, 0.15))
def test_tracks_against_the_oracle(fs, threshold):
    """Checks 1 to 3 on the 2 s clips.  Measured on an MI355X, worst |c - c_oracle| / (beta c): 0.0138 at 8 kHz, 0.0099 at 16 kHz, at both
    thresholds (the row does not depend on the threshold)."""
    o = dict(conditions(want(fs, threshold), f"{fs}"), threshold=threshold)
    assert len(o["f0"]) == 197 and int(o["voiced"].sum()) == 96
    worst = check_against_oracle(o, got(fs, threshold), f"{fs} Hz, threshold {threshold}")
    print(f"\n[pitch] {fs} Hz, threshold {threshold}: worst |c - c_oracle| = {worst:.4f} beta c (beta = {R.beta(o['g']):.3e})")


@pytest.mark.parametrize("fs", RATES)
def test_what_the_tracker_reads(fs):
    o, g = conditions(want(fs), f"{fs}"), got(fs)
    geo, x = o["g"], clip(fs)
    part = fs // 2
    start = np.arange(g["frames"]) * geo["hop"]
    end = start + geo["span"]
    glide, noise, silence, tones = end <= part, (start >= part) & (end <= 2 * part), (start >= 2 * part) & (end <= 3 * part), start >= 3 * part
    assert glide.sum() > 40 and noise.sum() > 40 and silence.sum() > 40 and tones.sum() > 40
    at = R.glide_f0(np.array([R.nominal_time(t, geo) for t in np.flatnonzero(glide)]))
    assert (g["voiced"][glide] == 1).all() and np.abs(g["f0"][glide] / at - 1).max() <= 0.02
    assert (g["voiced"][tones] == 1).all() and np.abs(g["f0"][tones] / 220.5 - 1).max() <= 0.005
    assert (g["voiced"][noise] == 0).all() and (g["voiced"][silence] == 0).all()
    # all-zero frames: tau_min and an aperiodicity of exactly 1
    assert (g["f0"][silence] == fs / geo["tau_min"]).all() and (g["aperiodicity"][silence] == 1.0).all() and (g["cmnd"][silence] == 1.0).all()
    # frames whose first W samples are zero and whose lags reach into the tones: unvoiced, exact ones as long as S = 0
    edge = [t for t in range(g["frames"]) if not x[start[t]:start[t] + geo["W"]].any() and x[start[t] + geo["W"]:end[t]].any()]
    assert edge, "no frame straddles the end of the silence"
    for t in edge:
        first = int(np.flatnonzero(o["d"][t, 1:])[0]) + 1  # the first lag that reaches a sample of the tones
        assert g["voiced"][t] == 0 and (g["cmnd"][t, :first] == 1.0).all() and g["cmnd"][t, first] == float(first)


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------------------------
def voiced_clip(n, fs, seed=SEED, scale=1.0, steady=False):
    """The glide from `scale` 110 Hz; `steady`: 220.5 Hz and its octave instead (a long window needs a pitch that stays)."""
    rng = np.random.default_rng(seed)
    if steady:
        t = np.arange(n) / fs
        return (0.25 * np.sin(2 * np.pi * 220.5 * t) + 0.125 * np.sin(2 * np.pi * 441.0 * t + 1.0) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    return R.glide(n, fs, rng, scale).astype(np.float32)


G8 = R.lags(8000)
EDGES = {
    "span - 1": (G8["span"] - 1, 8000, {}),
    "span": (G8["span"], 8000, {}),
    "span + hop - 1": (G8["span"] + G8["hop"] - 1, 8000, {}),
    "span + hop": (G8["span"] + G8["hop"], 8000, {}),
    "one sample": (1, 8000, {}),
    "a group and a frame": (G8["span"] + GROUP * G8["hop"], 8000, {}),
    "a workgroup's groups and a frame": (G8["span"] + GROUP * WALK * G8["hop"] + 3, 8000, {}),
    "T + 1 = 128": (1500, 8000, dict(fmin=8000 / 126, fmax=400.0)),
    "T + 1 = 65": (900, 8000, dict(fmin=8000 / 63, fmax=1000.0), dict(scale=2.0)),
    "hop odd": (1500, 8000, dict(hop=77)),
    "window 101": (1200, 8000, dict(window=101)),
    "window 102": (1200, 8000, dict(window=102)),
    "window 103": (1200, 8000, dict(window=103, hop=1)),
    "window 3": (400, 8000, dict(window=3, hop=31)),
    "hop above span": (2400, 8000, dict(window=50, hop=501)),
    "48 kHz: groups of two frames, a stage above the prefetch": (1601 + 6 * 480 + 7, 48000, {}),
    "48 kHz, fmin 30: one frame a group": (3201 + 2 * 480, 48000, dict(fmin=30.0)),
    "window 3000: a stage above the prefetch": (3268 + 9 * 160, 16000, dict(window=3000), dict(steady=True)),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(name):
    n, fs, kw = EDGES[name][:3]
    o, worst = case(voiced_clip(n, fs, **(EDGES[name][3] if len(EDGES[name]) > 3 else {})), fs, name, **kw)
    assert len(o["f0"]) == R.frames(n, o["g"]) == l3ac_amd.pitch_frames(n, fs, **kw)
    assert o["voiced"].all()
    print(f"\n[pitch] {name}: {len(o['f0'])} frames, {int(o['voiced'].sum())} voiced, worst |c - c_oracle| = {worst:.4f} beta c")


def test_edge_shapes_are_what_they_say():
    for name, frames in (("span - 1", 0), ("span", 1), ("span + hop - 1", 1), ("span + hop", 2), ("one sample", 0), ("a group and a frame", GROUP + 1),
                         ("a workgroup's groups and a frame", GROUP * WALK + 1)):
        n, fs, kw = EDGES[name][:3]
        assert R.frames(n, R.lags(fs, **kw)) == frames, name
    assert R.lags(8000, 8000 / 126, 400.0)["T"] + 1 == 128 and R.lags(8000, 8000 / 63, 1000.0)["T"] + 1 == 65
    assert (R.lags(8000)["T"] + 1) % 64 and (R.lags(16000)["T"] + 1) % 64  # the defaults: not multiples of 64


def test_no_frame_gives_empty_tracks_and_nan_rows():
    x = torch.from_numpy(voiced_clip(1000, 8000))[None].to(DEV)
    short = l3ac_amd.pitch(x[:, :G8["span"] - 1], 8000, return_cmnd=True)
    assert short["f0"].shape == short["voiced"].shape == short["aperiodicity"].shape == (1, 0) and short["cmnd"].shape == (1, 0, G8["T"] + 1)
    assert short["frames"].tolist() == [0]
    out = l3ac_amd.pitch(x.repeat(2, 1), 8000, lengths=[1000, G8["span"] - 1], return_cmnd=True)  # F = 10 and 0
    assert out["frames"].tolist() == [10, 0] and out["f0"].shape == (2, 10)
    assert torch.isnan(out["f0"][1]).all() and torch.isnan(out["aperiodicity"][1]).all() and not out["voiced"][1].any()
    assert torch.isnan(out["cmnd"][1]).all() and torch.isfinite(out["f0"][0]).all() and torch.isfinite(out["cmnd"][0]).all()


def test_unaligned_and_strided_rows_give_the_same_bits():
    fs = 8000
    a, b = clip(fs)[:6001], R.clip(fs, SEED + 1)[:6001]
    plain = l3ac_amd.pitch(torch.from_numpy(np.stack((a, b))).to(DEV), fs, return_cmnd=True)
    wide = torch.full((2, 6011), 7.0, device=DEV)
    wide[:, 1:6002] = torch.from_numpy(np.stack((a, b))).to(DEV)
    view = wide[:, 1:6002]
    assert view.data_ptr() % 16 != 0 and view.stride(0) % 4 != 0 and not view.is_contiguous()
    shifted = l3ac_amd.pitch(view, fs, return_cmnd=True)
    for k in plain:
        assert same(plain[k], shifted[k]), k
    assert int(plain["frames"][0]) == R.frames(6001, G8) and int(plain["voiced"][0].sum()) > 10


def test_non_finite_samples_stay_in_their_frames():
    fs, g = 8000, G8
    x = clip(fs)[:4000].copy()
    clean = track(x, fs)
    x[2000], x[2001] = np.nan, np.inf
    dirty = track(x, fs)
    start = np.arange(clean["frames"]) * g["hop"]
    untouched = (start + g["span"] <= 2000) | (start > 2001)
    assert untouched.sum() >= 10 and (~untouched).sum() >= 3
    for k in ("f0", "voiced", "aperiodicity", "cmnd"):
        assert np.array_equal(bits(torch.from_numpy(clean[k][untouched])), bits(torch.from_numpy(dirty[k][untouched]))), k
    assert np.isin(dirty["voiced"], (0, 1)).all()


# ---- 6. ragged invariance -----------------------------------------------------------------------------------------------------------------------------
def test_a_clip_does_not_depend_on_its_batch_row_scratch_or_what_follows_it():
    fs = 8000
    lens = [16000, 9003, G8["span"] + 9 * G8["hop"]]
    clips = [R.clip(fs, SEED + i)[:n] for i, n in enumerate(lens)]
    rows = np.empty((3, 16000), dtype=np.float32)
    for i, (c, n) in enumerate(zip(clips, lens)):
        rows[i, :n] = c
        rows[i, n::2] = 1e30  # what lies after a clip's length is not read
        rows[i, n + 1::2] = np.nan
    batch = torch.from_numpy(rows).to(DEV)
    alone = [l3ac_amd.pitch(torch.from_numpy(c)[None].to(DEV), fs, return_cmnd=True) for c in clips]
    need = _capi.load_library().l3ac_pitch_scratch_bytes(3, 16000, fs, 60.0, 500.0, -1, -1)
    f_max = R.frames(16000, G8)
    for order in ([0, 1, 2], [2, 1, 0]):
        for extra in (None, 0, need):  # the minimum scratch (twice: the default is the minimum) and twice the minimum
            out = l3ac_amd.pitch(batch[order], fs, lengths=[lens[i] for i in order], return_cmnd=True, extra_scratch=extra)
            assert out["f0"].shape == (3, f_max)
            for row, i in enumerate(order):
                n = R.frames(lens[i], G8)
                assert int(out["frames"][row]) == n == int(alone[i]["frames"][0])
                for k in ("f0", "voiced", "aperiodicity", "cmnd"):
                    assert same(out[k][row, :n], alone[i][k][0]), (order, extra, i, k)
                assert torch.isnan(out["f0"][row, n:]).all() and torch.isnan(out["aperiodicity"][row, n:]).all()
                assert not out["voiced"][row, n:].any() and torch.isnan(out["cmnd"][row, n:]).all()


# ---- 7. the pair metrics ---------------------------------------------------------------------------------------------------------------------------
def check_metrics(ref, est, fs, lens, **kw):
    """pitch_metrics of a batch against the oracle's formulas on the library's own tracks -> the metrics as numpy."""
    r, e = torch.from_numpy(np.stack(ref)).to(DEV), torch.from_numpy(np.stack(est)).to(DEV)
    pm = l3ac_amd.pitch_metrics(r, e, fs, lengths=lens, **kw)
    assert set(pm) == {"f0_rmse_cents", "gpe", "vde", "ffe", "frames", "voiced_reference", "voiced_estimate", "voiced_both"}
    tr, te = l3ac_amd.pitch(r, fs, lengths=lens, **kw), l3ac_amd.pitch(e, fs, lengths=lens, **kw)
    out = {k: v.cpu().numpy() for k, v in pm.items()}
    for i in range(len(ref)):
        n = int(tr["frames"][i])
        o = R.metrics(tr["f0"][i].cpu().numpy(), tr["voiced"][i].cpu().numpy(), te["f0"][i].cpu().numpy(), te["voiced"][i].cpu().numpy(), n)
        for k in ("frames", "voiced_reference", "voiced_estimate", "voiced_both"):
            assert pm[k].dtype == torch.int32 and int(out[k][i]) == o[k], (i, k)
        bound = R.rmse_bound(o["voiced_both"])
        for k in ("f0_rmse_cents", "gpe", "vde", "ffe"):
            assert pm[k].dtype == torch.float64 and pm[k].is_cuda
            if np.isnan(o[k]):
                assert np.isnan(out[k][i]), (i, k)
            else:
                assert abs(out[k][i] - o[k]) <= bound * abs(o[k]), (i, k, out[k][i], o[k])
    return out


def test_metrics_follow_the_formulas_on_the_librarys_own_tracks():
    """Two noise draws of the 2 s clip at 16 kHz and a shorter pair, over the pairs' own frames.  Measured on an MI355X: see the print."""
    fs = 16000
    a, b, c = R.clip(fs, SEED), R.clip(fs, SEED + 1), R.clip(fs, SEED + 2)
    out = check_metrics([a, b, c], [b, c, a], fs, [32000, 20001, 535 + 160 * 300 // 10])
    assert out["frames"].tolist() == [197, R.frames(20001, R.lags(fs)), 31] and (out["voiced_both"] > 20).all()
    assert (out["f0_rmse_cents"] > 0).all() and (out["f0_rmse_cents"] < 100).all() and (out["gpe"] < 0.1).all() and (out["vde"] < 0.1).all()
    print(f"\n[pitch] metrics of two noise draws: rmse {out['f0_rmse_cents']} cents, vde {out['vde']}, ffe {out['ffe']}")


def test_identical_inputs_give_zero():
    a = R.clip(8000, SEED)
    out = check_metrics([a, a[::-1].copy()], [a, a[::-1].copy()], 8000, None)
    for k in ("f0_rmse_cents", "gpe", "vde", "ffe"):
        assert (out[k] == 0.0).all(), k
    assert (out["voiced_both"] == out["voiced_reference"]).all() and (out["voiced_both"] > 40).all()


def test_an_octave_up_on_half_of_the_voiced_frames_is_a_gross_error_of_one_half():
    """Frames that do not overlap (hop = span), 14 of the glide and 14 of the glide again; the estimate doubles the second glide's f0."""
    fs = 16000
    g = R.lags(fs, hop=535)
    assert g["hop"] == g["span"] == 535
    n = 14 * 535
    first, second, doubled = voiced_clip(n, fs, 11), voiced_clip(n, fs, 12), R.glide(n, fs, np.random.default_rng(12), scale=2.0).astype(np.float32)
    ref, est = np.concatenate((first, second)), np.concatenate((first, doubled))
    for x, name in ((ref, "octave: reference"), (est, "octave: estimate")):
        o = conditions(R.oracle(x, fs, hop=535), name)
        assert (o["voiced"] == 1).all() and len(o["voiced"]) == 28
    out = check_metrics([ref], [est], fs, None, hop=535)
    assert out["frames"][0] == out["voiced_both"][0] == 28 and out["gpe"][0] == 0.5 and out["vde"][0] == 0.0 and out["ffe"][0] == 0.5
    assert abs(out["f0_rmse_cents"][0] / (1200.0 * np.sqrt(0.5)) - 1) < 0.01  # 14 frames at 0, 14 at an octave


def test_no_frame_voiced_on_both_sides_and_no_frame_at_all():
    fs = 8000
    a = R.clip(fs, SEED)
    out = check_metrics([a, a, a], [np.zeros_like(a), a, np.zeros_like(a)], fs, [16000, G8["span"] - 1, 1])
    assert out["voiced_both"].tolist() == [0, 0, 0] and out["frames"].tolist() == [197, 0, 0]
    assert np.isnan(out["gpe"]).all() and np.isnan(out["f0_rmse_cents"]).all()
    assert out["vde"][0] == 96 / 197 == out["ffe"][0] and np.isnan(out["vde"][1:]).all() and np.isnan(out["ffe"][1:]).all()


# ---- 9. codec.evaluate ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_with_pitch_equals_the_composed_calls(codec):
    lens = [6400, 8000]
    audio = torch.zeros(2, 8000)
    for i, n in enumerate(lens):
        audio[i, :n] = torch.from_numpy(voiced_clip(n, 16000, 600 + i))
    audio = audio.to(DEV)
    kw = dict(process_window=2700, prefix_tokens=3)  # windows of 10 tokens with a 3-token look-back: several chunks each
    result = codec.evaluate(audio, lengths=lens, pitch=True, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :8000]
    pm = l3ac_amd.pitch_metrics(audio, decoded, sample_rate=codec.config.sample_rate, lengths=lens)
    for key, src in (("f0_rmse_cents", "f0_rmse_cents"), ("gpe", "gpe"), ("vde", "vde"), ("ffe", "ffe"), ("pitch_frames", "frames"),
                     ("pitch_voiced", "voiced_both")):
        assert same(result[key], pm[src]) and result[key].is_cuda, key
    assert result["pitch_frames"].tolist() == [R.frames(n, R.lags(16000)) for n in lens]
    today = {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
    assert set(result) == today | {"f0_rmse_cents", "gpe", "vde", "ffe", "pitch_frames", "pitch_voiced"}
    assert set(codec.evaluate(audio, lengths=lens, **kw)) == today
