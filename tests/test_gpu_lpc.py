"""Linear prediction and the envelope measures on the GPU (csrc/kernels/lpc.hip) against the fp64 oracle of
tests/lpc_ref.py: the autocorrelation, the recursion, the validity and the quadratic forms bit for bit; integer data exactly, without the
oracle's order; the identities that hold bit for bit; the values behind a log within the bound section 3.18 derives (1 ulp for the device's
log and log10, as HIP's documentation states and nobody has measured on gfx950, plus the count of later roundings); trimming; a pair's bits
independent of its batch, strides, scratch and what follows its length; composition; stream capture; and the sanity of the measure."""
import functools

import numpy as np
import pytest
import torch

import l3ac_amd
from tests import lpc_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIR_KEYS = ("llr", "is_distance", "cepstral_distance_db", "seg_snr_db")
FRAME_KEYS = (("llr_frames", "llr"), ("is_frames", "is"), ("cd_frames", "cd"), ("seg_snr_frames", "snr"))


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


# ---- inputs: three pairs a case, 20 or more frames each, i.e. more than one group of 16 ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_inputs(p, fs, n):
    hop = max(n // 4, 1)
    t = n + 21 * hop + 3
    res = R.resonator(t, fs, seed=1000 * p + n)
    sine = R.sine_plus_noise(t, fs, seed=7 * p + n)
    gap = R.resonator(t, fs, seed=2000 * p + n)
    gap[3 * hop:3 * hop + 2 * n + hop] = 0.0  # frames 3 and 4 (and more for small hops) read nothing but zeros
    ref = np.stack([res, sine, gap])
    est = np.stack([R.add_noise(res, 15.0, 1), R.sine_plus_noise(t, fs, seed=7 * p + n + 1), (0.5 * R.add_noise(gap, 25.0, 2)).astype(np.float32)])
    est[2, 3 * hop:3 * hop + 2 * n + hop] = 0.0
    return ref, est, hop


@functools.lru_cache(maxsize=None)
def case_oracle(p, fs, n):
    ref, est, hop = case_inputs(p, fs, n)
    sides = [(R.lpc(ref[i], fs, p, n, hop), R.lpc(est[i], fs, p, n, hop)) for i in range(3)]
    return sides, [R.frame_values(a, b) for a, b in sides]


ORDERS = ((4, 8000), (10, 8000), (16, 16000), (32, 16000))
CASES = [(p, fs, n) for p, fs in ORDERS for n in sorted({p + 1, 63, 64, 65, 100, 240}) if n > p]


# ---- 1. the bit-exact stage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,fs,n", CASES)
def test_autocorrelation_recursion_validity_and_forms_are_the_oracles_bits(p, fs, n):
    ref, est, hop = case_inputs(p, fs, n)
    sides, values = case_oracle(p, fs, n)
    frames = R.n_frames(ref.shape[1], n, hop)
    assert frames >= 20
    for side, audio in ((0, ref), (1, est)):
        got = l3ac_amd.lpc(torch.from_numpy(audio).to(DEV), sample_rate=fs, order=p, frame=n, hop=hop)
        assert set(got) == {"a", "reflection", "error", "autocorr", "valid", "frames"} and all(v.is_cuda for v in got.values())
        assert got["a"].shape == (3, frames, p + 1) and got["reflection"].shape == (3, frames, p) and got["error"].shape == (3, frames)
        assert got["a"].dtype == torch.float64 and got["valid"].dtype == got["frames"].dtype == torch.int32
        assert cpu(got["frames"]).tolist() == [frames] * 3
        for i in range(3):
            want = sides[i][side]
            for key in ("autocorr", "valid", "a", "reflection", "error"):
                assert same(got[key][i], want[key]), (key, i, side)
    assert sides[1][0]["valid"].all() and sides[1][1]["valid"].all()  # the ill-conditioned sine stays valid in the oracle
    assert not sides[2][0]["valid"][3] and not sides[2][1]["valid"][3] and sides[2][0]["valid"][0]  # the zero stretch is invalid on both sides
    got = l3ac_amd.lpc_metrics(torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV), sample_rate=fs, order=p, frame=n, hop=hop,
                               return_frames=True)
    for i in range(3):
        assert same(got["forms"][i], values[i]["forms"]), i
        assert int(got["lpc_frames"][i]) == int(values[i]["both"].sum()) and int(got["snr_frames"][i]) == int(values[i]["counted"].sum())
        assert np.array_equal(np.isnan(cpu(got["llr_frames"][i])), ~values[i]["both"])
        assert np.array_equal(np.isnan(cpu(got["seg_snr_frames"][i])), ~values[i]["counted"])


@pytest.mark.parametrize("p,fs,n,hop,frames", [(16, 44100, 1323, 330, 20), (32, 16000, 4100, 1000, 5), (16, 16000, 8192, 2048, 3), (10, 8000, 8192, 9000, 2)])
def test_long_frames_take_smaller_groups_and_the_same_bits(p, fs, n, hop, frames):
    """The frames of a group share one staging buffer: 16 frames at the defaults up to 22 kHz, 8 at 44.1 kHz, one frame above about 2600
    samples; a frame of 8192 samples needs more LDS than a launch gets without asking (and hop > frame stages frame by frame)."""
    t = n + (frames - 1) * hop + 7
    ref = R.resonator(t, fs, seed=n + p)
    est = R.add_noise(ref, 15.0, n)
    a, b = R.lpc(ref, fs, p, n, hop), R.lpc(est, fs, p, n, hop)
    fv = R.frame_values(a, b)
    got = l3ac_amd.lpc(dev(ref), sample_rate=fs, order=p, frame=n, hop=hop)
    assert int(got["frames"][0]) == frames and a["valid"].all()
    for key in ("autocorr", "valid", "a", "reflection", "error"):
        assert same(got[key][0], a[key]), key
    pair = l3ac_amd.lpc_metrics(dev(ref), dev(est), sample_rate=fs, order=p, frame=n, hop=hop, return_frames=True)
    assert same(pair["forms"][0], fv["forms"]) and int(pair["lpc_frames"][0]) == frames
    want = R.pair_values(fv)
    for key in PAIR_KEYS:
        assert abs(float(pair[key][0]) - want[key]) <= want["bounds"][key], key


# ---- 2. exact without the oracle's order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n,hop", [(4, 5, 1), (10, 64, 16), (16, 100, 25), (32, 33, 40)])
def test_integer_samples_give_the_integer_sums_exactly(p, n, hop):
    rng = np.random.default_rng(n)
    t = n + 19 * hop + 2
    ref = rng.integers(-8, 9, (2, t)).astype(np.float32)
    est = rng.integers(-8, 9, (2, t)).astype(np.float32)
    frames = R.n_frames(t, n, hop)
    idx = np.arange(frames)[:, None] * hop + np.arange(n)[None, :]
    got = l3ac_amd.lpc(torch.from_numpy(ref).to(DEV), sample_rate=8000, order=p, frame=n, hop=hop, window="rect")
    pair = l3ac_amd.lpc_metrics(torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV), sample_rate=8000, order=p, frame=n, hop=hop,
                                window="rect", return_frames=True)
    for i in range(2):
        fr, fe = ref[i].astype(np.int64)[idx], est[i].astype(np.int64)[idx]
        want = np.stack([(fr[:, :n - k] * fr[:, k:]).sum(axis=1) for k in range(p + 1)], axis=1)
        assert np.array_equal(cpu(got["autocorr"][i]), want.astype(np.float64))
        assert np.array_equal(cpu(pair["forms"][i, :, 3]), (fr * fr).sum(axis=1).astype(np.float64))
        assert np.array_equal(cpu(pair["forms"][i, :, 4]), ((fr - fe) ** 2).sum(axis=1).astype(np.float64))


# ---- 3. identities that hold bit for bit ----------------------------------------------------------------------------------------------------------
def test_a_clip_against_itself_and_against_its_double():
    fs, p, n, hop = 16000, 16, 240, 60
    x = dev(R.resonator(1500, fs, seed=5), R.sine_plus_noise(1500, fs, seed=6))
    own = l3ac_amd.lpc_metrics(x, x.clone(), sample_rate=fs, order=p, frame=n, hop=hop)
    for key in ("llr", "is_distance", "cepstral_distance_db"):
        assert same(own[key], torch.zeros(2, dtype=torch.float64)), key
    assert same(own["seg_snr_db"], torch.full((2,), 35.0, dtype=torch.float64))
    assert cpu(own["lpc_frames"]).tolist() == cpu(own["frames"]).tolist() == [R.n_frames(1500, n, hop)] * 2
    twice = l3ac_amd.lpc_metrics(x, 2.0 * x, sample_rate=fs, order=p, frame=n, hop=hop, return_frames=True)
    for key in ("llr", "cepstral_distance_db", "seg_snr_db"):
        assert same(twice[key], torch.zeros(2, dtype=torch.float64)), key
    ln4 = np.log(4.0)
    want = (0.25 + ln4) - 1.0
    bound = 2.0 * R.U * ln4 + R.U * (0.25 + ln4) + R.U * want  # section 3.18: the log, the sum, the difference
    worst = np.abs(cpu(twice["is_frames"]) - want).max()
    print(f"is_frames of a doubled clip: worst {worst / bound:.3f} of the bound")
    assert worst <= bound
    assert same(twice["forms"][..., 2], 4.0 * twice["forms"][..., 1]) and same(twice["forms"][..., 0], twice["forms"][..., 1])


# ---- 4. the log stage -----------------------------------------------------------------------------------------------------------------------------
def test_values_behind_a_log_are_within_the_derived_bound():
    worst = {}
    for p, fs, n in ((4, 8000, 65), (10, 8000, 240), (16, 16000, 100), (32, 16000, 240)):
        ref, est, hop = case_inputs(p, fs, n)
        _, values = case_oracle(p, fs, n)
        for trim in (0.95, 1.0):
            got = l3ac_amd.lpc_metrics(torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV), sample_rate=fs, order=p, frame=n, hop=hop,
                                       trim=trim, return_frames=True)
            for i in range(3):
                fv = values[i]
                for key, name in FRAME_KEYS:
                    mask = fv["counted"] if name == "snr" else fv["both"]
                    err, bound = np.abs(cpu(got[key][i]) - fv[name])[mask], fv["bounds"][name][mask]
                    assert (err <= bound).all(), (key, p, n, i, (err / np.maximum(bound, 1e-300)).max())
                    live = bound > 0
                    worst[name] = max(worst.get(name, 0.0), float((err[live] / bound[live]).max()) if live.any() else 0.0)
                want = R.pair_values(fv, trim)
                for key in PAIR_KEYS:
                    err, bound = abs(float(got[key][i]) - want[key]), want["bounds"][key]
                    assert err <= bound, (key, p, n, i, trim, err, bound)
                    worst[key] = max(worst.get(key, 0.0), err / bound if bound > 0 else 0.0)
                assert int(got["frames"][i]) == want["frames"] and int(got["lpc_frames"][i]) == want["lpc_frames"]
    print("worst observed error over the derived bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ---- 5. trimming ----------------------------------------------------------------------------------------------------------------------------------
def test_trimming_a_click_one_frame_and_no_frame():
    fs, p, n, hop = 8000, 10, 240, 240  # frames that do not overlap: the click lands in one of them
    ref = R.resonator(n * 20, fs, seed=11)
    est = R.add_noise(ref, 30.0, 3)
    est[7 * n + 100] += 0.9
    r, e = dev(ref), dev(est)
    all_frames = l3ac_amd.lpc_metrics(r, e, sample_rate=fs, order=p, frame=n, hop=hop, trim=1.0)
    trimmed = l3ac_amd.lpc_metrics(r, e, sample_rate=fs, order=p, frame=n, hop=hop, trim=0.95)
    fv = R.frame_values(R.lpc(ref, fs, p, n, hop), R.lpc(est, fs, p, n, hop))
    assert fv["both"].sum() == 20 and R.trim_count(0.95, 20) == 19 and np.argmax(fv["llr"]) == 7
    for got, trim in ((all_frames, 1.0), (trimmed, 0.95)):
        want = R.pair_values(fv, trim)
        for key in PAIR_KEYS:
            assert abs(float(got[key][0]) - want[key]) <= want["bounds"][key], (key, trim)
    assert float(trimmed["llr"][0]) < float(all_frames["llr"][0]) and float(trimmed["cepstral_distance_db"][0]) < float(all_frames["cepstral_distance_db"][0])
    assert same(trimmed["seg_snr_db"], all_frames["seg_snr_db"])  # the SNR is not trimmed
    one = l3ac_amd.lpc_metrics(r[:, :n + 5], e[:, :n + 5], sample_rate=fs, order=p, frame=n, hop=hop, return_frames=True)  # V = 1: k = 1
    assert int(one["lpc_frames"][0]) == 1 and same(one["llr"], one["llr_frames"][:, 0]) and same(one["is_distance"], one["is_frames"][:, 0])
    low = l3ac_amd.lpc_metrics(r[:, :n + 5], e[:, :n + 5], sample_rate=fs, order=p, frame=n, hop=hop, trim=0.4)  # floor(0.4 + 0.5) = 0
    assert np.isnan(cpu(low["llr"])).all() and not np.isnan(cpu(low["seg_snr_db"])).any()
    zero = torch.zeros(1, 3 * n, device=DEV)
    none = l3ac_amd.lpc_metrics(zero, zero.clone(), sample_rate=fs, order=p, frame=n, hop=hop)
    assert int(none["frames"][0]) == 3 and int(none["lpc_frames"][0]) == 0 and int(none["snr_frames"][0]) == 0
    for key in PAIR_KEYS:
        assert np.isnan(cpu(none[key])).all(), key


@pytest.mark.parametrize("frames", [2049, 16384])
def test_a_pair_of_many_frames_sorts_in_several_passes_per_thread(frames):
    """More than 2048 frames: a thread of the pair's workgroup holds more than one compare-exchange per step; 16384 frames: the cap, the
    whole of the sort's LDS."""
    fs, p, n, hop = 8000, 4, 5, 1
    t = n + frames - 1
    ref = R.resonator(t, fs, seed=frames)
    ref[t // 2:t // 2 + 40] = 0.0  # some frames invalid: the padding with +inf is not only at the end
    est = R.add_noise(ref, 10.0, 9)
    fv = R.frame_values(R.lpc(ref, fs, p, n, hop), R.lpc(est, fs, p, n, hop))
    want = R.pair_values(fv)
    got = l3ac_amd.lpc_metrics(dev(ref), dev(est), sample_rate=fs, order=p, frame=n, hop=hop)
    assert int(got["frames"][0]) == frames and int(got["lpc_frames"][0]) == want["lpc_frames"] < frames
    assert int(got["snr_frames"][0]) == want["snr_frames"]
    for key in PAIR_KEYS:
        assert abs(float(got[key][0]) - want[key]) <= want["bounds"][key], (key, float(got[key][0]), want[key])


# ---- 6. ragged batches and independence -------------------------------------------------------------------------------------------------------------
def test_a_pair_does_not_depend_on_its_batch_row_strides_scratch_or_what_follows_it():
    fs, p, n, hop = 16000, 16, 100, 25
    lens = [1500, 733, 99, 100]  # 99 < frame: no frame at all; 100: exactly one
    t = max(lens)
    ref = np.stack([R.resonator(t, fs, seed=30 + i) for i in range(4)])
    est = np.stack([R.add_noise(ref[i], 12.0, 50 + i) for i in range(4)])
    kw = dict(sample_rate=fs, order=p, frame=n, hop=hop)
    alone = [l3ac_amd.lpc_metrics(dev(ref[i, :m]), dev(est[i, :m]), return_frames=True, **kw) for i, m in enumerate(lens)]
    alone_lpc = [l3ac_amd.lpc(dev(ref[i, :m]), **kw) for i, m in enumerate(lens)]
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
    batch = l3ac_amd.lpc_metrics(view_r, view_e, lengths=lens, return_frames=True, extra_scratch=4096 + 256, **kw)
    batch_lpc = l3ac_amd.lpc(view_r, lengths=lens, extra_scratch=1 << 16, **kw)
    f_max = R.n_frames(t, n, hop)
    assert cpu(batch["frames"]).tolist() == cpu(batch_lpc["frames"]).tolist() == [R.n_frames(m, n, hop) for m in lens] == [57, 26, 0, 1]
    for i, m in enumerate(lens):
        f = R.n_frames(m, n, hop)
        for key in PAIR_KEYS + ("frames", "lpc_frames", "snr_frames"):
            assert same(batch[key][i:i + 1], alone[i][key]), (key, i)
        for key in ("llr_frames", "is_frames", "cd_frames", "seg_snr_frames", "forms"):
            assert same(batch[key][i, :f], alone[i][key][0]), (key, i)
            assert np.isnan(cpu(batch[key][i, f:])).all() and batch[key].shape[1] == f_max
        for key in ("a", "reflection", "error", "autocorr", "valid"):
            assert same(batch_lpc[key][i, :f], alone_lpc[i][key][0]), (key, i)
        assert np.isnan(cpu(batch_lpc["a"][i, f:])).all() and np.isnan(cpu(batch_lpc["autocorr"][i, f:])).all() and not cpu(batch_lpc["valid"][i, f:]).any()
    assert np.isnan(cpu(batch["llr"][2])) and np.isnan(cpu(batch["seg_snr_db"][2])) and int(batch["lpc_frames"][2]) == 0
    assert not np.isnan(cpu(batch["llr"][[0, 1, 3]])).any()


# ---- 7. composition -------------------------------------------------------------------------------------------------------------------------------
def test_lpc_metrics_is_lpc_of_each_side_combined_by_the_oracles_formulas():
    fs = 16000
    p, n, hop = R.defaults(fs)
    ref = R.resonator(3000, fs, seed=70)
    est = R.add_noise(ref, 18.0, 71)
    got = l3ac_amd.lpc_metrics(dev(ref), dev(est), sample_rate=fs, return_frames=True)  # the defaults: 16, 480, 120
    side = []
    for x in (ref, est):
        out = l3ac_amd.lpc(dev(x), sample_rate=fs)
        assert out["a"].shape == (1, R.n_frames(3000, n, hop), p + 1)
        side.append({"a": cpu(out["a"][0]), "autocorr": cpu(out["autocorr"][0]), "valid": cpu(out["valid"][0]),
                     "xw": R.frames_xw(x, cpu(l3ac_amd.lpc_window(n)), n, hop)})
    fv = R.frame_values(*side)
    assert same(got["forms"][0], fv["forms"])
    for key, name in FRAME_KEYS:
        assert (np.abs(cpu(got[key][0]) - fv[name]) <= fv["bounds"][name]).all(), key
    want = R.pair_values(fv)
    for key in PAIR_KEYS:
        assert abs(float(got[key][0]) - want[key]) <= want["bounds"][key], key


@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_with_lpc_equals_the_composed_calls(codec):
    lens = [16000, 14400]
    audio = torch.zeros(2, 16000)
    for i, m in enumerate(lens):
        audio[i, :m] = torch.from_numpy(R.resonator(m, 16000, seed=600 + i))
    audio = audio.to(DEV)
    kw = dict(process_window=5400, prefix_tokens=3)  # several chunks each
    result = codec.evaluate(audio, lengths=lens, lpc=True, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :16000]
    composed = l3ac_amd.lpc_metrics(audio, decoded, sample_rate=codec.config.sample_rate, lengths=lens)
    for key in PAIR_KEYS + ("lpc_frames",):
        assert same(result[key], composed[key]) and result[key].is_cuda, key
    assert (result["llr"] > 0).all() and cpu(result["lpc_frames"]).tolist() == [R.n_frames(m, 480, 120) for m in lens]
    today = {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
    assert set(result) == today | set(PAIR_KEYS) | {"lpc_frames"}
    assert set(codec.evaluate(audio, lengths=lens, **kw)) == today


# ---- 8. capture -----------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_one_warm_up_call_and_the_window_refuses_to_upload_under_capture():
    fs, p, n, hop = 8000, 10, 77, 19  # a frame length no other test uses: its window is not on the device yet
    ref = dev(R.resonator(1200, fs, seed=80), R.resonator(1200, fs, seed=81))
    est = dev(R.add_noise(cpu(ref[0]), 10.0, 82), R.add_noise(cpu(ref[1]), 25.0, 83))
    kw = dict(sample_rate=fs, order=p, frame=n, hop=hop, lengths=[1200, 640], return_frames=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside stream capture"):
        with torch.cuda.graph(graph):
            l3ac_amd.lpc_metrics(ref, est, **kw)
    torch.cuda.synchronize()
    eager = l3ac_amd.lpc_metrics(ref, est, **kw)  # (the warm-up: uploads the window)
    eager_lpc = l3ac_amd.lpc(ref, sample_rate=fs, order=p, frame=n, hop=hop)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = l3ac_amd.lpc_metrics(ref, est, **kw)
        out_lpc = l3ac_amd.lpc(ref, sample_rate=fs, order=p, frame=n, hop=hop)
    est.mul_(0.5)  # the replay reads the tensors' current contents ...
    graph.replay()
    torch.cuda.synchronize()
    assert not same(out["seg_snr_db"], eager["seg_snr_db"])
    est.mul_(2.0)  # ... (a power of two: exactly undone)
    graph.replay()
    torch.cuda.synchronize()
    for key in eager:
        assert same(out[key], eager[key]), key
    for key in eager_lpc:
        assert same(out_lpc[key], eager_lpc[key]), key


# ---- 9. the sanity of the measure -------------------------------------------------------------------------------------------------------------------
def test_more_noise_is_a_larger_llr_and_the_segmental_snr_is_the_constructions():
    fs, p, n, hop = 8000, 10, 240, 60  # (tests/test_lpc_host.py checks these inputs on the oracle: 0.31 against 0.003, 19.9 dB)
    ref = R.resonator(3000, fs, seed=7)
    noisy, clean = R.add_noise(ref, 20.0, 1), R.add_noise(ref, 40.0, 1)
    got = l3ac_amd.lpc_metrics(dev(ref, ref), dev(noisy, clean), sample_rate=fs, order=p, frame=n, hop=hop)
    assert float(got["llr"][0]) > 2.0 * float(got["llr"][1]) > 0.0
    assert float(got["cepstral_distance_db"][0]) > float(got["cepstral_distance_db"][1]) > 0.0
    assert abs(float(got["seg_snr_db"][0]) - 20.0) < 1.0
    assert cpu(got["lpc_frames"]).tolist() == cpu(got["frames"]).tolist() == [R.n_frames(3000, n, hop)] * 2  # no frame skipped
    sine = l3ac_amd.lpc_metrics(dev(R.sine_plus_noise(1500, fs, seed=2)), dev(R.sine_plus_noise(1500, fs, seed=3)), sample_rate=fs, order=p, frame=n,
                                hop=hop)
    assert int(sine["lpc_frames"][0]) == int(sine["frames"][0]) == R.n_frames(1500, n, hop) and 0.0 < float(sine["llr"][0]) <= 2.0
