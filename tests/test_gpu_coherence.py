"""The coherence measures on the GPU (csrc/kernels/coherence.hip) against the fp64 oracle of tests/coherence_ref.py:
the frame energies, classes and counts, the cross-spectral sums of every class, the coherence and both band sums bit for bit, compared as
integers; the values behind a log10 or an exp within the bound section 3.23 derives (1 ulp for each function on each side, as HIP's and
glibc's documentation state, plus the count of later roundings); the exact cases; a pair's bits independent of its batch, row, strides,
scratch and what follows its length; a custom band table; stream capture; isolation from a non-finite neighbour; composition.

The references are the resonator under the envelope 0.02 + 0.98 (0.5 - 0.5 cos(2 pi n / period))^2 so that every level class occurs; the
period is 4000 samples at the default hop of 120 and scales with the hop, so that a frame spans the same part of a cycle in every case."""
import functools

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import coherence_ref as R
from tests import poison as P
from tests.lpc_ref import add_noise, resonator

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 16000
VALUES = ("csii", "csii_high", "csii_mid", "csii_low")
BOUNDED = VALUES + ("i3", "intelligibility")
# (n_fft, frame, hop): fewer bins than lanes; one wave a frame; its largest transform; the smallest transform of a whole workgroup, one bin a
# thread; the default, two bins a thread; four bins a thread; the largest transform, eight bins a thread.  A chunk is 64 frames up to n_fft =
# 256, 32 up to 1024, 16 at 2048, 8 at 4096.
CASES = ((16, 5, 1), (64, 40, 10), (256, 128, 32), (512, 200, 50), (1024, 480, 120), (2048, 1024, 256), (4096, 2048, 512))
IDS = [f"{c[0]}-{c[1]}" for c in CASES]
# a hop above the frame in the one-wave-a-frame and the workgroup-a-frame form, and a hop equal to the frame: the staged frames do not overlap,
# and with a hop above the frame the samples between them are never read
HOP_CASES = ((64, 40, 50), (1024, 480, 500), (64, 40, 40))
EXACT_CASES = CASES + HOP_CASES
EXACT_IDS = IDS + [f"{c[0]}-{c[1]}-hop{c[2]}" for c in HOP_CASES]


def bits(t):
    """A tensor or array as integers: NaN entries compare like any other, -0 differs from +0."""
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    if a.dtype == np.complex128:
        a = a.view(np.float64)
    return a.view(np.int64) if a.dtype == np.float64 else a


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
def tables(n_fft, table=None):
    centre, width, imp = R.sii_table(FS) if table is None else table
    return l3ac_amd.band_weights(FS, n_fft, (centre, width)).numpy(), imp


def swept(samples, hop, seed):
    return (resonator(samples, FS, seed=seed).astype(np.float64) * R.envelope(samples, period=max(8, round(4000 * hop / 120)))).astype(np.float32)


# ---- inputs: four pairs a case: one frame more than a chunk, exactly a chunk, one frame fewer, three chunks and a frame; 1e30 after every length ----
@functools.lru_cache(maxsize=None)
def case_inputs(n_fft, n, hop):
    c = R.chunk_frames(n_fft)
    lens = [n + c * hop + (hop - 1), n + (c - 1) * hop, n + (c - 2) * hop + hop // 2, n + 3 * c * hop]
    t = max(lens) + 3
    ref = np.full((4, t), 1e30, dtype=np.float32)
    est = np.full((4, t), 1e30, dtype=np.float32)
    for i, m in enumerate(lens):
        ref[i, :m] = swept(m, hop, seed=100 * n_fft + i)
        est[i, :m] = add_noise(ref[i, :m], (0.0, 5.0, 15.0, 30.0)[i], seed=i)
    return ref, est, lens


@functools.lru_cache(maxsize=None)
def case_oracle(n_fft, n, hop):
    ref, est, lens = case_inputs(n_fft, n, hop)
    w, imp = tables(n_fft)
    return [R.pair(ref[i, :m], est[i, :m], n, hop, n_fft, twiddles(n_fft), w, imp) for i, m in enumerate(lens)]


def check_exact(got_coh, got_csii, want, i, f):
    """Row i of the two calls' results against one oracle pair, bit for bit."""
    assert int(got_coh["frames"][i]) == int(got_csii["frames"][i]) == want["frames"] == f
    assert cpu(got_coh["level_frames"][i]).tolist() == cpu(got_csii["level_frames"][i]).tolist() == want["level_frames"].tolist()
    assert same(got_coh["frame_energy"][i, :f], want["frame_energy"]) and np.isnan(cpu(got_coh["frame_energy"][i, f:])).all()
    assert same(got_coh["frame_class"][i, :f], want["frame_class"]) and (cpu(got_coh["frame_class"][i, f:]) == -1).all()
    for got in (got_coh, got_csii):
        assert same(got["sxx"][i], want["sums"][:, 0]) and same(got["syy"][i], want["sums"][:, 1])
        assert same(got["sxy"][i].real, want["sums"][:, 2]) and same(got["sxy"][i].imag, want["sums"][:, 3])
    assert same(got_coh["msc"][i], want["msc"]) and same(got_coh["msc_levels"][i], want["msc_levels"])
    assert same(got_csii["band_signal"][i], want["band_signal"]) and same(got_csii["band_distortion"][i], want["band_distortion"])


# ---- 1. the bit-exact stage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n,hop", EXACT_CASES, ids=EXACT_IDS)
def test_energies_classes_sums_coherence_and_band_sums_are_the_oracles_bits(n_fft, n, hop):
    ref, est, lens = case_inputs(n_fft, n, hop)
    want = case_oracle(n_fft, n, hop)
    c = R.chunk_frames(n_fft)
    frames = [R.n_frames(m, n, hop) for m in lens]
    assert frames == [c + 1, c, c - 1, 3 * c + 1]  # both sides of the kernel's chunk, and several chunks
    f_max, h = R.n_frames(ref.shape[1], n, hop), n_fft // 2
    r, e = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    kw = dict(frame=n, hop=hop, n_fft=n_fft, lengths=lens)
    coh = l3ac_amd.coherence(r, e, FS, return_sums=True, **kw)
    assert set(coh) == {"msc", "frames", "level_frames", "msc_levels", "sxx", "syy", "sxy", "frame_class", "frame_energy"}
    assert all(v.is_cuda for v in coh.values())
    assert coh["msc"].shape == (4, h) and coh["msc_levels"].shape == coh["sxx"].shape == coh["syy"].shape == coh["sxy"].shape == (4, 4, h)
    assert coh["sxy"].dtype == torch.complex128 and coh["frame_class"].shape == coh["frame_energy"].shape == (4, f_max)
    assert coh["frames"].dtype == coh["level_frames"].dtype == coh["frame_class"].dtype == torch.int32 and coh["level_frames"].shape == (4, 4)
    cs = l3ac_amd.csii(r, e, FS, return_bands=True, return_sums=True, **kw)
    assert set(cs) == set(BOUNDED) | {"frames", "level_frames", "band_signal", "band_distortion", "band_value", "sxx", "syy", "sxy"}
    assert cs["band_signal"].shape == cs["band_distortion"].shape == cs["band_value"].shape == (4, 4, 20) and cs["csii"].shape == (4,)
    for i, f in enumerate(frames):
        check_exact(coh, cs, want[i], i, f)
    assert (cpu(coh["level_frames"])[:, :3].sum(axis=0) >= 2).all()  # the envelope does its work: every class occurs in the case
    plain = l3ac_amd.coherence(r, e, FS, **kw)
    assert set(plain) == {"msc", "frames", "level_frames"} and all(same(plain[k], coh[k]) for k in plain)
    plain = l3ac_amd.csii(r, e, FS, **kw)
    assert set(plain) == set(BOUNDED) | {"frames", "level_frames"} and all(same(plain[k], cs[k]) for k in plain)


# ---- 2. behind log10 and exp ----------------------------------------------------------------------------------------------------------------
def test_values_behind_log10_and_exp_are_within_the_derived_bound():
    worst = {}
    for n_fft, n, hop in CASES:
        ref, est, lens = case_inputs(n_fft, n, hop)
        want = case_oracle(n_fft, n, hop)
        got = l3ac_amd.csii(torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV), FS, frame=n, hop=hop, n_fft=n_fft, lengths=lens,
                            return_bands=True)
        for i in range(len(lens)):
            err, bound = np.abs(cpu(got["band_value"][i]) - want[i]["band_value"]), want[i]["band_value_bound"]
            assert (err <= bound).all(), ("band_value", n_fft, i, (err / np.maximum(bound, 1e-300)).max())
            live = bound > 0
            worst["band_value"] = max(worst.get("band_value", 0.0), float((err[live] / bound[live]).max()) if live.any() else 0.0)
            for key in BOUNDED:
                v, w, bound = float(got[key][i]), want[i][key], want[i]["bounds"][key]
                if np.isnan(w):
                    assert np.isnan(v), (key, n_fft, i)
                    continue
                assert abs(v - w) <= bound, (key, n_fft, i, abs(v - w), bound)
                worst[key] = max(worst.get(key, 0.0), abs(v - w) / bound if bound > 0 else 0.0)
    assert set(worst) == set(BOUNDED) | {"band_value"}  # every value was compared somewhere
    print("worst observed error over the derived bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ---- 3. exact cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n,hop", [(64, 40, 10), (1024, 480, 120)])
def test_exact_cases(n_fft, n, hop):
    m = n + 70 * hop
    ref = swept(m, hop, seed=5)
    x = dev(ref, ref, ref, np.zeros_like(ref))
    y = dev(ref, -2.0 * ref, np.zeros_like(ref), ref)
    kw = dict(frame=n, hop=hop, n_fft=n_fft)
    got = l3ac_amd.csii(x, y, FS, return_bands=True, **kw)
    coh = l3ac_amd.coherence(x, y, FS, return_sums=True, **kw)
    counts = cpu(got["level_frames"])
    assert (counts[0, :3] >= 2).all() and cpu(got["frames"]).tolist() == [71] * 4
    one, zero = torch.ones(2, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    for key in VALUES:  # the estimate is the reference, or -2 times it: exactly 1; a zero estimate: exactly 0
        assert same(got[key][:2], one) and same(got[key][2:3], zero), key
    assert same(got["i3"][:2], torch.full((2,), (-3.47 + 1.84) + 9.99, dtype=torch.float64)) and float(got["i3"][2]) == -3.47
    assert (cpu(got["band_distortion"][:2]) == 0).all() and (cpu(got["band_signal"][2]) == 0).all()
    live = cpu(coh["sxx"][:2]).sum(axis=1) > 0
    assert (cpu(coh["msc"][:2])[live] == 1.0).all() and (cpu(coh["msc"][2]) == 0.0).all()
    sxx = cpu(coh["sxx"][1])  # (the sums of a class without frames are +0 on every side: compared as numbers)
    assert (cpu(coh["syy"][1]) == 4.0 * sxx).all() and (cpu(coh["sxy"][1].real) == -2.0 * sxx).all() and (cpu(coh["sxy"][:2].imag) == 0).all()
    # an all-zero reference: every frame below, no class value, csii of all frames 0
    assert counts[3].tolist() == [0, 0, 0, 71] and (cpu(coh["frame_class"][3]) == 3).all()
    for key in ("csii_high", "csii_mid", "csii_low", "i3", "intelligibility"):
        assert np.isnan(float(got[key][3])), key
    assert float(got["csii"][3]) == 0.0 and np.isnan(cpu(coh["msc_levels"][3, :3])).all()
    # classes of 0 or 1 frames: one loud frame among silent ones; one frame in all; no frame at all
    lone = np.zeros(n + 5 * hop, dtype=np.float32)
    lone[3 * hop + n - hop:3 * hop + n] = ref[:hop]  # read by frame 3 alone among its last samples, and by later frames at lower window weight
    short = dev(lone, lone, lone)
    few = l3ac_amd.csii(short, short.clone(), FS, lengths=[n + 5 * hop, n + hop - 1, n - 1], **kw)
    assert cpu(few["frames"]).tolist() == [6, 1, 0]
    c0 = cpu(few["level_frames"])[0]
    assert c0.sum() == 6 and (c0[:3] < 2).any()
    for k, key in enumerate(("csii_high", "csii_mid", "csii_low")):
        assert np.isnan(float(few[key][0])) == (c0[k] < 2), (key, c0)
    assert np.isnan(float(few["i3"][0])) == (c0[1] < 2 or c0[2] < 2) and float(few["csii"][0]) == 1.0
    for key in BOUNDED:
        assert np.isnan(cpu(few[key][1:])).all(), key
    none = l3ac_amd.coherence(short[:, :n - 1], short[:, :n - 1].clone(), FS, return_sums=True, **kw)  # no frame anywhere
    assert none["frame_class"].shape == (3, 0) and cpu(none["frames"]).tolist() == [0] * 3 and np.isnan(cpu(none["msc"])).all()


# ---- 4. independence ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n,hop", [(64, 40, 10), (1024, 480, 120)])
def test_a_pair_does_not_depend_on_its_batch_row_strides_scratch_or_what_follows_it(n_fft, n, hop):
    c = R.chunk_frames(n_fft)
    lens = [n + (c + 2) * hop + 3, n + 8 * hop, n - 1, n, n + (2 * c) * hop + 1]  # n - 1: no frame at all; n: exactly one
    t = max(lens)
    ref = np.stack([swept(t, hop, seed=30 + i) for i in range(5)])
    est = np.stack([add_noise(ref[i], 12.0, 50 + i) for i in range(5)])
    kw = dict(frame=n, hop=hop, n_fft=n_fft)
    alone = [l3ac_amd.csii(dev(ref[i, :m]), dev(est[i, :m]), FS, return_bands=True, return_sums=True, extra_scratch=0, **kw) for i, m in enumerate(lens)]
    alone_coh = [l3ac_amd.coherence(dev(ref[i, :m]), dev(est[i, :m]), FS, return_sums=True, extra_scratch=0, **kw) for i, m in enumerate(lens)]
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
    need = _capi.load_library().l3ac_coherence_scratch_bytes(5, t, n, hop, n_fft)
    for extra in (0, 3 * need):
        batch = l3ac_amd.csii(view_r, view_e, FS, lengths=lens, return_bands=True, return_sums=True, extra_scratch=extra, **kw)
        batch_coh = l3ac_amd.coherence(view_r, view_e, FS, lengths=lens, return_sums=True, extra_scratch=extra, **kw)
        assert cpu(batch["frames"]).tolist() == [R.n_frames(m, n, hop) for m in lens] == [c + 3, 9, 0, 1, 2 * c + 1]
        for i, m in enumerate(lens):
            f = R.n_frames(m, n, hop)
            for key in batch:
                assert same(batch[key][i:i + 1], alone[i][key]), (key, i)
            for key in batch_coh:
                got = batch_coh[key][i:i + 1, :f] if key in ("frame_class", "frame_energy") else batch_coh[key][i:i + 1]
                assert same(got, alone_coh[i][key]), (key, i)
    # reversed rows: a pair's place in its batch
    order = [4, 3, 2, 1, 0]
    flipped = l3ac_amd.csii(view_r[order], view_e[order], FS, lengths=[lens[i] for i in order], return_bands=True, **kw)
    for key in flipped:
        assert same(flipped[key], batch[key][order]), key


# ---- 5. the two calls agree; a custom table -------------------------------------------------------------------------------------------------------
def test_the_two_calls_agree_and_a_custom_table_works():
    n, hop, n_fft = 480, 120, 1024
    ref = swept(9000, hop, seed=61)
    est = add_noise(ref, 10.0, 62)
    r, e = dev(ref), dev(est)
    coh = l3ac_amd.coherence(r, e, FS, return_sums=True)
    cs = l3ac_amd.csii(r, e, FS, return_bands=True, return_sums=True)
    for key in ("frames", "level_frames", "sxx", "syy", "sxy"):
        assert same(coh[key], cs[key]), key
    table = ((500.0, 1500.0, 4000.0, 7000.0), (200.0, 400.0, 800.0, 1000.0), (0.4, 0.3, 0.2, 0.1))
    w, imp = tables(n_fft, table)
    want = R.pair(ref, est, n, hop, n_fft, twiddles(n_fft), w, imp)
    got = l3ac_amd.csii(r, e, FS, bands=table, return_bands=True)
    assert got["band_value"].shape == (1, 4, 4)
    assert same(got["band_signal"][0], want["band_signal"]) and same(got["band_distortion"][0], want["band_distortion"])
    for key in BOUNDED:
        assert abs(float(got[key][0]) - want[key]) <= want["bounds"][key], key
    assert not same(got["csii"], cs["csii"]) and same(got["level_frames"], cs["level_frames"])
    tensors = l3ac_amd.csii(r, e, FS, bands=tuple(torch.tensor(v, dtype=torch.float64) for v in table))
    assert all(same(tensors[key], got[key]) for key in tensors)
    rect = l3ac_amd.coherence(r, e, FS, window="rect")
    assert not same(rect["msc"], coh["msc"])


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_one_warm_up_call_and_the_tables_refuse_to_upload_under_capture():
    n, hop, n_fft = 83, 21, 512  # a frame no other test of the suite uses: its window is not on the device yet
    ref = dev(swept(2400, hop, seed=80), swept(2400, hop, seed=81))
    est = dev(add_noise(cpu(ref[0]), 10.0, 82), add_noise(cpu(ref[1]), 25.0, 83))
    kw = dict(frame=n, hop=hop, n_fft=n_fft, lengths=[2400, 1640], return_bands=True, return_sums=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside stream capture"):
        with torch.cuda.graph(graph):
            l3ac_amd.csii(ref, est, FS, **kw)
    torch.cuda.synchronize()
    eager = l3ac_amd.csii(ref, est, FS, **kw)  # (the warm-up: uploads the window, the twiddles, the weights and the importances)
    eager_coh = l3ac_amd.coherence(ref, est, FS, frame=n, hop=hop, n_fft=n_fft, return_sums=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = l3ac_amd.csii(ref, est, FS, **kw)
        out_coh = l3ac_amd.coherence(ref, est, FS, frame=n, hop=hop, n_fft=n_fft, return_sums=True)
    est.mul_(0.0)  # the replay reads the tensors' current contents ...
    graph.replay()
    torch.cuda.synchronize()
    assert same(out["csii"], torch.zeros(2, dtype=torch.float64))
    est.copy_(dev(add_noise(cpu(ref[0]), 10.0, 82), add_noise(cpu(ref[1]), 25.0, 83)))
    graph.replay()
    torch.cuda.synchronize()
    for key in eager:
        assert same(out[key], eager[key]), key
    for key in eager_coh:
        assert same(out_coh[key], eager_coh[key]), key


# ---- 7. isolation -----------------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_side_spoils_only_its_own_pair():
    n, hop, n_fft = 100, 25, 256
    lens = [2500, 1733, 100, 1900]
    t = max(lens)
    ref = torch.stack([torch.from_numpy(swept(t, hop, seed=30 + i)) for i in range(4)])
    est = torch.stack([torch.from_numpy(add_noise(cpu(ref[i]), 12.0, 50 + i)) for i in range(4)])
    batch = torch.stack([ref, est], dim=1).to(DEV)
    kw = dict(frame=n, hop=hop, n_fft=n_fft, lengths=lens)
    for pattern in P.PATTERNS:  # the pattern in the REFERENCE of pair 0 and in the ESTIMATE of the last pair
        bad = batch.clone()
        bad[0, 0, :lens[0]] = P.patterns(batch[0, 0, :lens[0]])[pattern]
        bad[3, 1, :lens[3]] = P.patterns(batch[3, 1, :lens[3]])[pattern]
        P.twin_check(lambda q: l3ac_amd.csii(q[:, 0], q[:, 1], FS, return_bands=True, return_sums=True, **kw), batch, [0, 3], pattern, what="csii",
                     bad=bad, finite=False)  # (pair 2 has one frame: its values are NaN)
        P.twin_check(lambda q: l3ac_amd.coherence(q[:, 0], q[:, 1], FS, return_sums=True, **kw), batch, [0, 3], pattern, what="coherence", bad=bad,
                     finite=False)
    clean =l3ac_amd.csii(batch[:, 0], batch[:, 1], FS, **kw)
    assert torch.isfinite(clean["csii"][[0, 1, 3]]).all() and np.isnan(float(clean["csii"][2]))


# ---- 8. composition ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_with_coherence_equals_the_composed_calls(codec):
    lens = [16000, 14400]
    audio = torch.zeros(2, 16000)
    for i, m in enumerate(lens):
        audio[i, :m] = torch.from_numpy(swept(m, 120, seed=600 + i))
    audio = audio.to(DEV)
    kw = dict(process_window=5400, prefix_tokens=3)  # several chunks each
    result = codec.evaluate(audio, lengths=lens, coherence=True, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :16000]
    composed = l3ac_amd.csii(audio, decoded, sample_rate=codec.config.sample_rate, lengths=lens)
    for key, name in (("csii", "csii"), ("csii_high", "csii_high"), ("csii_mid", "csii_mid"), ("csii_low", "csii_low"), ("csii_i3", "i3")):
        assert same(result[key], composed[name]) and result[key].is_cuda, key
    assert ((result["csii"] >= 0) & (result["csii"] <= 1)).all()
    today = {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
    assert set(result) == today | {"csii", "csii_high", "csii_mid", "csii_low", "csii_i3"}
    plain = codec.evaluate(audio, lengths=lens, **kw)
    assert set(plain) == today
    for key in today - {"per_scale"}:
        assert same(plain[key], result[key]), key
