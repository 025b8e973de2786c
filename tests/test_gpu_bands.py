"""The critical-band measures on the GPU (csrc/kernels/bands.hip) against the fp64 oracle of tests/bands_ref.py: the
spectrum, the power, the magnitude and its sum, both band sums, every peak, every first maximum and the frame counts bit for bit, compared
as integers; the values behind a log10 or a pow within the bound section 3.22 derives (1 ulp for each function on each side, as HIP's and
glibc's documentation state, plus the count of later roundings); the exact cases; a custom band table; trimming; a pair's bits independent
of its batch, row, strides, scratch and what follows its length; stream capture; isolation from a non-finite neighbour; composition."""
import functools

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import bands_ref as R
from tests import poison as P
from tests.lpc_ref import add_noise, resonator

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 16000
PAIR_KEYS = ("fw_seg_snr_db", "wss", "lsd_db")
FRAME_KEYS = (("fw_seg_snr_frames", "fw"), ("wss_frames", "wss"), ("lsd_frames", "lsd"))
EXACT_KEYS = ("magnitude_sum", "band_power", "band_magnitude", "peaks", "argmax")
# (n_fft, frame, hop, frames of a group in the kernel): fewer bins than lanes and empty partials; one and two bins a lane; the default; the
# largest transform.  A group is 16 frames up to n_fft = 256, 8 up to 1024, 4 at 2048, 2 at 4096.
CASES = ((16, 5, 1, 16), (16, 16, 4, 16), (64, 40, 10, 16), (128, 128, 32, 16), (1024, 480, 120, 8), (4096, 2048, 512, 2))
IDS = [f"{c[0]}-{c[1]}" for c in CASES]
# a hop above the frame in the one-wave-a-frame and the workgroup-a-frame form, and a hop equal to the frame: the staged frames do not overlap,
# and with a hop above the frame the samples between them are never read
HOP_CASES = ((64, 40, 50, 16), (1024, 480, 500, 8), (64, 40, 40, 16))
EXACT_CASES = CASES + HOP_CASES
EXACT_IDS = IDS + [f"{c[0]}-{c[1]}-hop{c[2]}" for c in HOP_CASES]


def bits(t):
    """A tensor or array as integers: NaN entries compare like any other, -0 differs from +0."""
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    if a.dtype == np.complex128:
        a = a.view(np.float64)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def dev(*arrays):
    return torch.from_numpy(np.stack(arrays)).to(DEV)


def cpu(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def twiddles(n_fft):
    out = np.zeros(n_fft, dtype=np.float64)
    assert _capi.load_library().l3ac_bands_twiddles(n_fft, out.ctypes.data, n_fft) == n_fft
    return out.reshape(n_fft // 2, 2)


@functools.lru_cache(maxsize=None)
def weights(n_fft, table=None):
    return l3ac_amd.band_weights(FS, n_fft, table).numpy()


# ---- inputs: three pairs a case, one frame more than a group, exactly a group, one frame fewer; 1e30 after every clip's length ------------------
@functools.lru_cache(maxsize=None)
def case_inputs(n_fft, n, hop, g):
    lens = [n + g * hop + (hop - 1), n + (g - 1) * hop, n + (g - 2) * hop + hop // 2]
    t = max(lens) + 3
    ref = np.full((3, t), 1e30, dtype=np.float32)
    est = np.full((3, t), 1e30, dtype=np.float32)
    for i, m in enumerate(lens):
        ref[i, :m] = resonator(m, FS, seed=100 * n_fft + i)
        est[i, :m] = add_noise(ref[i, :m], (5.0, 15.0, 30.0)[i], seed=i)
    return ref, est, lens


@functools.lru_cache(maxsize=None)
def case_oracle(n_fft, n, hop, g, normalize=True):
    ref, est, lens = case_inputs(n_fft, n, hop, g)
    tw, w = twiddles(n_fft), weights(n_fft)
    sides = [(R.spectrum(ref[i, :m], n, hop, n_fft, tw), R.spectrum(est[i, :m], n, hop, n_fft, tw)) for i, m in enumerate(lens)]
    return sides, [R.frame_values(a, b, w, normalize=normalize) for a, b in sides]


# ---- 1. the bit-exact stage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n,hop,g", EXACT_CASES, ids=EXACT_IDS)
def test_spectrum_power_magnitude_and_their_sum_are_the_oracles_bits(n_fft, n, hop, g):
    ref, est, lens = case_inputs(n_fft, n, hop, g)
    sides, _ = case_oracle(n_fft, n, hop, g)
    frames = [R.n_frames(m, n, hop) for m in lens]
    assert frames == [g + 1, g, g - 1]  # both sides of the kernel's group
    f_max = R.n_frames(ref.shape[1], n, hop)
    for side, audio in ((0, ref), (1, est)):
        got = l3ac_amd.frame_spectrum(torch.from_numpy(audio).to(DEV), FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens, detail=True)
        assert set(got) == {"spectrum", "frames", "power", "magnitude", "magnitude_sum"} and all(v.is_cuda for v in got.values())
        assert got["spectrum"].shape == (3, f_max, n_fft // 2) and got["spectrum"].dtype == torch.complex128
        assert got["power"].shape == got["magnitude"].shape == (3, f_max, n_fft // 2) and got["magnitude_sum"].shape == (3, f_max)
        assert got["frames"].dtype == torch.int32 and cpu(got["frames"]).tolist() == frames
        for i, f in enumerate(frames):
            want = sides[i][side]
            assert same(got["spectrum"][i, :f].real, want["re"]) and same(got["spectrum"][i, :f].imag, want["im"]), (i, side)
            for key in ("power", "magnitude", "magnitude_sum"):
                assert same(got[key][i, :f], want[key]), (key, i, side)
                assert np.isnan(cpu(got[key][i, f:])).all()
            assert np.isnan(cpu(torch.view_as_real(got["spectrum"][i, f:]))).all()
        plain = l3ac_amd.frame_spectrum(torch.from_numpy(audio).to(DEV), FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens)
        assert set(plain) == {"spectrum", "frames"} and same(plain["spectrum"], got["spectrum"])


@pytest.mark.parametrize("n_fft,n,hop,g", EXACT_CASES, ids=EXACT_IDS)
def test_band_sums_peaks_maxima_and_counts_are_the_oracles_bits(n_fft, n, hop, g):
    ref, est, lens = case_inputs(n_fft, n, hop, g)
    r, e = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    frames = [R.n_frames(m, n, hop) for m in lens]
    f_max = R.n_frames(ref.shape[1], n, hop)
    for normalize in (True, False):
        _, values = case_oracle(n_fft, n, hop, g, normalize)
        got = l3ac_amd.band_metrics(r, e, FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens, normalize=normalize, return_frames=True)
        assert got["peaks"].shape == (3, f_max, 2, 24) and got["argmax"].shape == (3, f_max, 2) and got["peaks"].dtype == torch.int32
        assert cpu(got["frames"]).tolist() == frames
        for i, f in enumerate(frames):
            for key in EXACT_KEYS:
                assert same(got[key][i, :f], values[i][key]), (key, i, normalize)
            assert int(got["snr_frames"][i]) == int(values[i]["counted"].sum()) == f
    energies = [l3ac_amd.band_energies(x, FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens) for x in (r, e)]
    for side in (0, 1):  # (`values` is the un-normalised oracle here)
        assert set(energies[side]) == {"power", "magnitude", "frames"} and cpu(energies[side]["frames"]).tolist() == frames
        for i, f in enumerate(frames):
            assert same(energies[side]["power"][i, :f], values[i]["band_power"][:, side]), (i, side)
            assert same(energies[side]["magnitude"][i, :f], values[i]["band_magnitude"][:, side]), (i, side)
            assert np.isnan(cpu(energies[side]["power"][i, f:])).all() and energies[side]["power"].shape == (3, f_max, 25)


# ---- 2. behind log10 and pow ----------------------------------------------------------------------------------------------------------------
def test_values_behind_log10_and_pow_are_within_the_derived_bound():
    worst = {}
    for n_fft, n, hop, g in CASES:
        ref, est, lens = case_inputs(n_fft, n, hop, g)
        r, e = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
        for normalize, trim in ((True, 0.95), (False, 1.0)):
            _, values = case_oracle(n_fft, n, hop, g, normalize)
            got = l3ac_amd.band_metrics(r, e, FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens, normalize=normalize, trim=trim, return_frames=True)
            for i, m in enumerate(lens):
                fv = values[i]
                f = len(fv["counted"])
                for key, name in FRAME_KEYS:
                    err, bound = np.abs(cpu(got[key][i, :f]) - fv[name]), fv["bounds"][name]
                    assert (err <= bound).all(), (key, n_fft, n, i, normalize, (err / np.maximum(bound, 1e-300)).max())
                    live = bound > 0
                    worst[name] = max(worst.get(name, 0.0), float((err[live] / bound[live]).max()) if live.any() else 0.0)
                want = R.pair_values(fv, trim)
                for key in PAIR_KEYS:
                    err, bound = abs(float(got[key][i]) - want[key]), want["bounds"][key]
                    assert err <= bound, (key, n_fft, n, i, trim, err, bound)
                    worst[key] = max(worst.get(key, 0.0), err / bound if bound > 0 else 0.0)
    print("worst observed error over the derived bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ---- 3. clip lengths around one frame ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n,hop", [(64, 40, 10), (1024, 480, 120)])
def test_clip_lengths_around_a_frame(n_fft, n, hop):
    lens = [n - 1, n, n + hop - 1, n + hop]
    t = max(lens)
    ref = np.stack([resonator(t, FS, seed=40 + i) for i in range(4)])
    est = np.stack([add_noise(ref[i], 12.0, 50 + i) for i in range(4)])
    got = l3ac_amd.band_metrics(dev(*ref), dev(*est), FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens, return_frames=True)
    assert cpu(got["frames"]).tolist() == cpu(got["snr_frames"]).tolist() == [0, 1, 1, 2]
    tw, w = twiddles(n_fft), weights(n_fft)
    for i, m in enumerate(lens):
        want, fv = R.metrics(ref[i, :m], est[i, :m], n, hop, n_fft, tw, w)
        f = want["frames"]
        for key in EXACT_KEYS:
            assert same(got[key][i, :f], fv[key]), (key, i)
            assert (cpu(got[key][i, f:]) == -1).all() if key in ("peaks", "argmax") else np.isnan(cpu(got[key][i, f:])).all()
        for key in PAIR_KEYS:
            if f == 0:
                assert np.isnan(float(got[key][i])) and np.isnan(want[key]), key
            else:
                assert abs(float(got[key][i]) - want[key]) <= want["bounds"][key], (key, i)
    short = l3ac_amd.band_metrics(dev(ref[0, :n - 1]), dev(est[0, :n - 1]), FS, frame=n, hop=hop, n_fft=n_fft, return_frames=True)  # no frame anywhere
    assert short["wss_frames"].shape == (1, 0) and int(short["frames"][0]) == 0 and np.isnan(cpu(short["lsd_db"])).all()
    none = l3ac_amd.frame_spectrum(dev(ref[0, :n - 1]), FS, frame=n, hop=hop, n_fft=n_fft)
    assert none["spectrum"].shape == (1, 0, n_fft // 2) and int(none["frames"][0]) == 0


# ---- 4. exact cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [16, 64, 1024])
def test_constant_and_alternating_frames_are_exact(n_fft):
    c = 0.375
    const = torch.full((1, n_fft + 3), c, device=DEV)
    got = l3ac_amd.frame_spectrum(const, FS, frame=n_fft, hop=1, n_fft=n_fft, window="rect", detail=True)
    assert got["spectrum"].shape == (1, 4, n_fft // 2)
    spec = cpu(got["spectrum"])
    assert (spec[..., 0] == n_fft * c).all() and (spec[..., 1:] == 0).all()  # bin 0 = N c, every other bin +-0
    assert (cpu(got["magnitude_sum"]) == n_fft * c).all() and (cpu(got["power"])[..., 0] == (n_fft * c) ** 2).all()
    alt = torch.full((1, n_fft + 3), c, device=DEV)
    alt[:, 1::2] = -c
    got = l3ac_amd.frame_spectrum(alt, FS, frame=n_fft, hop=1, n_fft=n_fft, window="rect", detail=True)
    assert (cpu(got["spectrum"]) == 0).all() and (cpu(got["magnitude_sum"]) == 0).all()  # everything sits in the Nyquist bin, which is dropped


def test_a_clip_against_itself_and_silence():
    x = dev(resonator(3000, FS, seed=5), resonator(3000, FS, seed=6))
    own = l3ac_amd.band_metrics(x, x, FS)  # estimate is reference
    frames = R.n_frames(3000, 480, 120)
    assert same(own["fw_seg_snr_db"], torch.full((2,), 35.0, dtype=torch.float64))
    assert same(own["wss"], torch.zeros(2, dtype=torch.float64)) and same(own["lsd_db"], torch.zeros(2, dtype=torch.float64))
    assert cpu(own["frames"]).tolist() == cpu(own["snr_frames"]).tolist() == [frames] * 2
    copy = l3ac_amd.band_metrics(x, x.clone(), FS)
    for key in own:
        assert same(own[key], copy[key]), key
    zero = torch.zeros(1, 1000, device=DEV)
    silent = l3ac_amd.band_metrics(zero, zero.clone(), FS)
    assert int(silent["frames"][0]) == 5 and int(silent["snr_frames"][0]) == 0
    assert np.isnan(cpu(silent["fw_seg_snr_db"])).all() and same(silent["lsd_db"], torch.zeros(1, dtype=torch.float64))
    assert same(silent["wss"], torch.zeros(1, dtype=torch.float64))
    half = l3ac_amd.band_metrics(x[:1, :1000], zero, FS)  # a silent estimate: no frame counts for the fwSegSNR, the two others are defined
    assert int(half["snr_frames"][0]) == 0 and np.isnan(cpu(half["fw_seg_snr_db"])).all() and float(half["lsd_db"][0]) > 0 and float(half["wss"][0]) > 0


# ---- 5. a custom table ------------------------------------------------------------------------------------------------------------------------
def test_a_custom_three_band_table_reaching_7_khz():
    table = ((1000.0, 4000.0, 7000.0), (200.0, 400.0, 800.0))
    n, hop, n_fft = 480, 120, 1024
    ref = resonator(1500, FS, seed=61, poles=((1000.0, 0.97), (4000.0, 0.95), (7000.0, 0.93)))
    est = add_noise(ref, 15.0, 62)
    w = weights(n_fft, table)
    assert w.shape == (3, 512) and w[2, 448] > 0
    got = l3ac_amd.band_metrics(dev(ref), dev(est), FS, bands=table, return_frames=True)
    want, fv = R.metrics(ref, est, n, hop, n_fft, twiddles(n_fft), w)
    assert got["peaks"].shape == (1, want["frames"], 2, 2) and got["band_power"].shape == (1, want["frames"], 2, 3)
    for key in EXACT_KEYS:
        assert same(got[key][0], fv[key]), key
    for key in PAIR_KEYS:
        assert abs(float(got[key][0]) - want[key]) <= want["bounds"][key], key
    default = l3ac_amd.band_metrics(dev(ref), dev(est), FS)
    assert not same(default["wss"], got["wss"]) and same(default["lsd_db"], got["lsd_db"])  # the LSD does not see the bands
    en = l3ac_amd.band_energies(dev(ref), FS, bands=table)
    assert same(en["power"][0], fv["band_power"][:, 0]) and en["power"].shape == (1, want["frames"], 3)


# ---- 6. trimming ------------------------------------------------------------------------------------------------------------------------------
def test_trimming_one_frame_and_fewer_than_all():
    n, hop, n_fft = 128, 128, 128  # frames that do not overlap: the click lands in one of them
    ref = resonator(n * 20, FS, seed=11)
    est = add_noise(ref, 30.0, 3)
    est[7 * n + 40:7 * n + 90] = 0.0
    r, e = dev(ref), dev(est)
    kw = dict(frame=n, hop=hop, n_fft=n_fft)
    fv = R.metrics(ref, est, n, hop, n_fft, twiddles(n_fft), weights(n_fft))[1]
    assert len(fv["wss"]) == 20 and R.trim_count(0.95, 20) == 19 and np.argmax(fv["wss"]) == 7
    results = {}
    for trim in (1.0, 0.95, 0.5):
        got = results[trim] = l3ac_amd.band_metrics(r, e, FS, trim=trim, **kw)
        want = R.pair_values(fv, trim)
        for key in PAIR_KEYS:
            assert abs(float(got[key][0]) - want[key]) <= want["bounds"][key], (key, trim)
    assert float(results[0.5]["wss"][0]) < float(results[0.95]["wss"][0]) < float(results[1.0]["wss"][0])
    for key in ("fw_seg_snr_db", "lsd_db"):  # only the WSS is trimmed
        assert same(results[0.5][key], results[1.0][key]) and same(results[0.95][key], results[1.0][key])
    one = l3ac_amd.band_metrics(r[:, :n + 5], e[:, :n + 5], FS, return_frames=True, **kw)  # V = 1: k = 1
    assert int(one["frames"][0]) == 1
    for key, frame_key in (("fw_seg_snr_db", "fw_seg_snr_frames"), ("wss", "wss_frames"), ("lsd_db", "lsd_frames")):
        assert same(one[key], one[frame_key][:, 0]), key
    low = l3ac_amd.band_metrics(r[:, :n + 5], e[:, :n + 5], FS, trim=0.4, **kw)  # floor(0.4 + 0.5) = 0
    assert np.isnan(cpu(low["wss"])).all() and not np.isnan(cpu(low["fw_seg_snr_db"])).any() and not np.isnan(cpu(low["lsd_db"])).any()


# ---- 7. independence ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n,hop", [(64, 40, 10), (1024, 480, 120)])
def test_a_pair_does_not_depend_on_its_batch_row_strides_scratch_or_what_follows_it(n_fft, n, hop):
    lens = [n + 17 * hop + 3, n + 8 * hop, n - 1, n, n + 9 * hop + 1]  # n - 1: no frame at all; n: exactly one
    t = max(lens)
    ref = np.stack([resonator(t, FS, seed=30 + i) for i in range(5)])
    est = np.stack([add_noise(ref[i], 12.0, 50 + i) for i in range(5)])
    kw = dict(frame=n, hop=hop, n_fft=n_fft)
    alone = [l3ac_amd.band_metrics(dev(ref[i, :m]), dev(est[i, :m]), FS, return_frames=True, extra_scratch=0, **kw) for i, m in enumerate(lens)]
    alone_spec = [l3ac_amd.frame_spectrum(dev(ref[i, :m]), FS, detail=True, extra_scratch=0, **kw) for i, m in enumerate(lens)]
    alone_en = [l3ac_amd.band_energies(dev(est[i, :m]), FS, extra_scratch=0, **kw) for i, m in enumerate(lens)]
    junk_r, junk_e = ref.copy(), est.copy()
    for i, m in enumerate(lens):
        junk_r[i, m:] = 1e30
        junk_e[i, m:] = np.inf
    wide_r = torch.full((5, t + 37), float("nan"), device=DEV)
    wide_e = torch.full((5, t + 37), 1e30, device=DEV)
    wide_r[:, 5:5 + t] = torch.from_numpy(junk_r).to(DEV)
    wide_e[:, 9:9 + t] = torch.from_numpy(junk_e).to(DEV)
    view_r, view_e = wide_r[:, 5:5 + t], wide_e[:, 9:9 + t]  # strided row views, 1e30 / inf after every length
    assert not view_r.is_contiguous()
    need = _capi.load_library().l3ac_band_metrics_scratch_bytes(5, t, n, hop, n_fft, 25)
    for extra in (0, 7 * need):  # the minimum scratch and 8 times the minimum
        batch = l3ac_amd.band_metrics(view_r, view_e, FS, lengths=lens, return_frames=True, extra_scratch=extra, **kw)
        batch_spec = l3ac_amd.frame_spectrum(view_r, FS, lengths=lens, detail=True, extra_scratch=extra, **kw)
        batch_en = l3ac_amd.band_energies(view_e, FS, lengths=lens, extra_scratch=extra, **kw)
        assert cpu(batch["frames"]).tolist() == cpu(batch_spec["frames"]).tolist() == [R.n_frames(m, n, hop) for m in lens] == [18, 9, 0, 1, 10]
        for i, m in enumerate(lens):
            f = R.n_frames(m, n, hop)
            for key in PAIR_KEYS + ("frames", "snr_frames"):
                assert same(batch[key][i:i + 1], alone[i][key]), (key, i)
            for key in ("fw_seg_snr_frames", "wss_frames", "lsd_frames") + EXACT_KEYS:
                assert same(batch[key][i, :f], alone[i][key][0]), (key, i)
            for key in ("spectrum", "power", "magnitude", "magnitude_sum"):
                assert same(batch_spec[key][i, :f], alone_spec[i][key][0]), (key, i)
            for key in ("power", "magnitude"):
                assert same(batch_en[key][i, :f], alone_en[i][key][0]), (key, i)
        assert np.isnan(cpu(batch["wss"][2])) and int(batch["frames"][2]) == 0 and not np.isnan(cpu(batch["wss"][[0, 1, 3, 4]])).any()


# ---- 8. capture -----------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_one_warm_up_call_and_the_tables_refuse_to_upload_under_capture():
    n, hop, n_fft = 79, 19, 512  # a frame and a transform no other test of the suite uses: their tables are not on the device yet
    ref = dev(resonator(1200, FS, seed=80), resonator(1200, FS, seed=81))
    est = dev(add_noise(cpu(ref[0]), 10.0, 82), add_noise(cpu(ref[1]), 25.0, 83))
    kw = dict(frame=n, hop=hop, n_fft=n_fft, lengths=[1200, 640], return_frames=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside stream capture"):
        with torch.cuda.graph(graph):
            l3ac_amd.band_metrics(ref, est, FS, **kw)
    torch.cuda.synchronize()
    eager = l3ac_amd.band_metrics(ref, est, FS, **kw)  # (the warm-up: uploads the window, the twiddles and the weights)
    eager_spec = l3ac_amd.frame_spectrum(ref, FS, frame=n, hop=hop, n_fft=n_fft)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = l3ac_amd.band_metrics(ref, est, FS, **kw)
        out_spec = l3ac_amd.frame_spectrum(ref, FS, frame=n, hop=hop, n_fft=n_fft)
    est.mul_(0.5)  # the replay reads the tensors' current contents ...
    graph.replay()
    torch.cuda.synchronize()
    assert not same(out["lsd_db"], eager["lsd_db"])
    est.mul_(2.0)  # ... (a power of two: exactly undone)
    graph.replay()
    torch.cuda.synchronize()
    for key in eager:
        assert same(out[key], eager[key]), key
    for key in eager_spec:
        assert same(out_spec[key], eager_spec[key]), key


# ---- 9. isolation -----------------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_side_spoils_only_its_own_pair():
    n, hop, n_fft = 100, 25, 256
    lens = [1500, 733, 100, 900]
    t = max(lens)
    ref = torch.stack([torch.from_numpy(resonator(t, FS, seed=30 + i)) for i in range(4)])
    est = torch.stack([torch.from_numpy(add_noise(cpu(ref[i]), 12.0, 50 + i)) for i in range(4)])
    batch = torch.stack([ref, est], dim=1).to(DEV)
    for pattern in P.PATTERNS:  # the pattern in the REFERENCE of pair 0 and in the ESTIMATE of the last pair
        bad = batch.clone()
        bad[0, 0, :lens[0]] = P.patterns(batch[0, 0, :lens[0]])[pattern]
        bad[3, 1, :lens[3]] = P.patterns(batch[3, 1, :lens[3]])[pattern]
        P.twin_check(lambda q: l3ac_amd.band_metrics(q[:, 0], q[:, 1], FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens, return_frames=True), batch,
                     [0, 3], pattern, what="band_metrics", bad=bad, finite=False)  # (the rows after a clip's own frames are NaN)
        clean, _ = P.twin_check(lambda q: l3ac_amd.band_metrics(q[:, 0], q[:, 1], FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens), batch, [0, 3],
                                pattern, what="band_metrics", bad=bad)
        P.twin_check(lambda q: l3ac_amd.band_energies(q[:, 1], FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens), batch, [3], pattern,
                     what="band_energies", bad=bad, finite=False)
    assert all(torch.isfinite(clean[key][[1, 2]]).all() for key in PAIR_KEYS)


# ---- 10. composition ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_with_bands_equals_the_composed_calls(codec):
    lens = [16000, 14400]
    audio = torch.zeros(2, 16000)
    for i, m in enumerate(lens):
        audio[i, :m] = torch.from_numpy(resonator(m, 16000, seed=600 + i))
    audio = audio.to(DEV)
    kw = dict(process_window=5400, prefix_tokens=3)  # several chunks each
    result = codec.evaluate(audio, lengths=lens, bands=True, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :16000]
    composed = l3ac_amd.band_metrics(audio, decoded, sample_rate=codec.config.sample_rate, lengths=lens)
    for key in PAIR_KEYS:
        assert same(result[key], composed[key]) and result[key].is_cuda, key
    assert torch.isfinite(result["wss"]).all() and (result["lsd_db"] > 0).all() and (result["fw_seg_snr_db"] < 35.0).all()
    today = {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
    assert set(result) == today | set(PAIR_KEYS)
    plain = codec.evaluate(audio, lengths=lens, **kw)
    assert set(plain) == today
    for key in today - {"per_scale"}:
        assert same(plain[key], result[key]), key
