"""Quality metrics on the MI355X (kernels/metrics.hip): STFT and log-mel against the fp64 restatement (tests/metrics_ref.py) within
a-priori fp32 bounds, the exact cases, signal_metrics against numpy fp64, mel_distance's consistency with log_mel, bit invariance over
batch / row / stride / scratch size, graph capture, and codec.evaluate against the hand-composed calls."""
import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi, bits_per_token
from tests import metrics_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 16000
EPS = 2.0 ** -24
# (n_fft, hop, n_mels, n): (32, 8, 24) has 6 empty filters; n = 5 < n_fft / 2 is all halo; n at k hop and k hop +- 1 is the frame-count edge
SHAPES = [(16, 4, 4, 1), (16, 4, 4, 3), (16, 4, 4, 9), (32, 8, 24, 50), (64, 16, 8, 5), (64, 16, 8, 31), (64, 16, 8, 32), (64, 16, 8, 33),
          (64, 16, 8, 200), (256, 64, 20, 1000), (2048, 512, 80, 8000)]


def signal(n, seed):
    """Seeded noise of 0.1 plus a 0.3 sine at 440 Hz: every non-empty mel filter sees power far above the 1e-10 clamp."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    return (0.1 * torch.randn(n, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2 * np.pi * 440.0 / SR * t + 0.5)).float()


def tables(n_fft, n_mels):
    return l3ac_amd.stft_basis(n_fft).numpy(), l3ac_amd.mel_weights(SR, n_fft, n_mels).numpy()


def check_clip(x, spec, lm, n_fft, hop, n_mels, what):
    """One clip's spectrum (complex [F][bins]) and log-mel ([F][n_mels]) against fp64: (worst STFT ratio, worst log-mel ratio)."""
    basis, weights = tables(n_fft, n_mels)
    ref, absdot = M.stft_ref(x.double().numpy(), n_fft, hop, basis)
    assert spec.shape == ref.shape, what
    bound = (n_fft + 2) * EPS * absdot
    err = np.stack([np.abs(spec.real - ref.real), np.abs(spec.imag - ref.imag)], axis=-1)
    r_stft = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))))
    print(f"\n[metrics] {what}: STFT worst |err| / ((n_fft + 2) 2^-24 sum|w x|) = {r_stft:.4f}")
    assert (err <= bound).all(), f"{what}: STFT worst err / bound {r_stft:.3f}"
    l_ref, _ = M.log_mel_ref(ref, weights)
    d_l, excluded = M.log_mel_bound(ref, bound[..., 0], bound[..., 1], weights)
    empty = ~weights.any(axis=1)
    assert (excluded == np.broadcast_to(empty, excluded.shape)).all(), f"{what}: cells excluded from the bound are not exactly the empty filters"
    assert (lm[:, empty] == -10.0).all(), what
    err_l = np.abs(lm.astype(np.float64) - l_ref)[:, ~empty]
    r_mel = float(np.max(err_l / d_l[:, ~empty])) if err_l.size else 0.0
    print(f"[metrics] {what}: log-mel worst |err| / propagated bound = {r_mel:.4f}")
    assert (err_l <= d_l[:, ~empty]).all(), f"{what}: log-mel worst err / bound {r_mel:.3f}"
    return r_stft, r_mel


@pytest.mark.parametrize("n_fft,hop,n_mels,n", SHAPES)
def test_stft_and_log_mel_within_fp32_bounds(n_fft, hop, n_mels, n):
    x = signal(n, seed=n_fft + n)
    xd = x[None].to(DEV)
    spec = l3ac_amd.stft(xd, n_fft, hop)
    lm = l3ac_amd.log_mel(xd, SR, n_fft, hop, n_mels)
    assert spec.dtype == torch.complex64 and spec.shape == (1, 1 + n // hop, n_fft // 2 + 1)
    assert lm.dtype == torch.float32 and lm.shape == (1, 1 + n // hop, n_mels)
    check_clip(x, spec[0].cpu().numpy(), lm[0].cpu().numpy(), n_fft, hop, n_mels, f"({n_fft}, {hop}, {n_mels}) n = {n}")


@pytest.mark.parametrize("total", [127, 128, 129])
def test_ragged_batch_across_the_gemm_row_panel(total):
    """Three clips whose frame counts add up to 127 / 128 / 129, 1e30 after each clip's own samples: each clip against fp64 within the
    bounds, zero rows after its own frames, nothing of the padding anywhere."""
    n_fft, hop, n_mels = 64, 16, 8
    fr = [40, 60, total - 100]
    lens = [(fr[0] - 1) * hop + 15, (fr[1] - 1) * hop, (fr[2] - 1) * hop + 1]
    t = max(lens) + 7
    batch = torch.full((3, t), 1e30)
    clips = [signal(n, seed=total + i) for i, n in enumerate(lens)]
    for i, c in enumerate(clips):
        batch[i, :lens[i]] = c
    spec = l3ac_amd.stft(batch.to(DEV), n_fft, hop, lengths=lens)
    lm, frames = l3ac_amd.log_mel(batch.to(DEV), SR, n_fft, hop, n_mels, lengths=lens)
    assert frames.tolist() == fr and sum(fr) == total
    assert spec.shape == (3, 1 + t // hop, n_fft // 2 + 1) and lm.shape == (3, 1 + t // hop, n_mels)
    for i in range(3):
        check_clip(clips[i], spec[i, :fr[i]].cpu().numpy(), lm[i, :fr[i]].cpu().numpy(), n_fft, hop, n_mels, f"ragged {total} clip {i}")
        assert not torch.view_as_real(spec[i, fr[i]:]).any() and not lm[i, fr[i]:].any()


def test_silence_is_exactly_the_clamp():
    x = torch.zeros(2, 200, device=DEV)
    assert not torch.view_as_real(l3ac_amd.stft(x, 64, 16)).any()
    assert (l3ac_amd.log_mel(x, SR, 64, 16, 8) == -10.0).all()
    d = l3ac_amd.mel_distance(x, x, SR, scales=[(64, 16, 8), (32, 8, 24)])
    assert (d["mel_distance"] == 0).all() and (d["per_scale"] == 0).all()


def test_identical_and_scaled_estimates_are_exact():
    x = torch.stack([signal(777, 1), signal(777, 2)]).to(DEV)
    d = l3ac_amd.mel_distance(x, x, SR, scales=[(64, 16, 8), (256, 64, 20)])
    assert (d["mel_distance"] == 0).all() and (d["per_scale"] == 0).all()
    m = l3ac_amd.signal_metrics(x, x)
    inf = torch.full((2,), float("inf"), dtype=torch.float64, device=DEV)
    assert (m["mse"] == 0).all() and torch.equal(m["snr_db"], inf) and torch.equal(m["si_sdr_db"], inf)
    m2 = l3ac_amd.signal_metrics(x, 2 * x)
    assert torch.equal(m2["si_sdr_db"], inf) and (m2["snr_db"] == 0).all()


@pytest.mark.parametrize("n", [777, 4001])
def test_signal_metrics_against_numpy_fp64(n):
    """Pairs at about 10, 40 and 80 dB: 1e-12 relative on the sums (mse), 1e-9 dB on both dB values.  At 80 dB a one-pass formula that
    expands the residual's square loses its digits; the second pass does not."""
    g = torch.Generator().manual_seed(n)
    r = torch.stack([signal(n, 10 + i) for i in range(3)])
    noise = torch.randn(3, n, generator=g)
    scale = torch.tensor([10.0, 40.0, 80.0])
    e = (0.8 * r.double() + 0.01 + noise.double() * (r.double().std(dim=1, keepdim=True) * 0.8 * 10 ** (-scale[:, None].double() / 20))).float()
    lens = [n, n - 5, n - 300]
    m = l3ac_amd.signal_metrics(r.to(DEV), e.to(DEV), lengths=lens)
    for i in range(3):
        mse, snr, si = M.signal_metrics_ref(r[i, :lens[i]].numpy(), e[i, :lens[i]].numpy())
        got = [float(m[k][i]) for k in ("mse", "snr_db", "si_sdr_db")]
        print(f"\n[metrics] n = {lens[i]}: si_sdr {si:.6f} dB, mse rel err {abs(got[0] - mse) / mse:.2e}, snr err {abs(got[1] - snr):.2e} dB, "
              f"si_sdr err {abs(got[2] - si):.2e} dB")
        assert abs(si - float(scale[i])) < 1.0  # the pair is where it was meant to be
        assert abs(got[0] - mse) <= 1e-12 * mse
        assert abs(got[1] - snr) <= 1e-9 and abs(got[2] - si) <= 1e-9


def test_mel_distance_is_the_fp64_mean_of_log_mel_cells():
    scales = [(64, 16, 8), (32, 8, 24), (256, 64, 20)]
    lens = [1000, 333, 64]
    r = torch.stack([signal(1000, 20 + i) for i in range(3)]).to(DEV)
    e = (0.7 * r + 0.02 * torch.stack([signal(1000, 30 + i) for i in range(3)]).to(DEV))
    d = l3ac_amd.mel_distance(r, e, SR, scales=scales, lengths=lens)
    assert d["per_scale"].shape == (3, 3) and d["per_scale"].dtype == torch.float64 and d["mel_distance"].shape == (3,)
    assert torch.equal(d["mel_distance"], d["per_scale"].mean(dim=1))
    for s, (n_fft, hop, n_mels) in enumerate(scales):
        lr, fr = l3ac_amd.log_mel(r, SR, n_fft, hop, n_mels, lengths=lens)
        le, _ = l3ac_amd.log_mel(e, SR, n_fft, hop, n_mels, lengths=lens)
        for i in range(3):
            want = float((lr[i, :fr[i]].double() - le[i, :fr[i]].double()).abs().cpu().numpy().mean())
            got = float(d["per_scale"][i, s])
            assert want > 0 and abs(got - want) <= 1e-12 * want, (s, i, got, want)


def test_bits_do_not_depend_on_batch_row_stride_or_scratch():
    """A clip alone (contiguous, minimum scratch) against the same clip at rows 0, 1 and last of a ragged batch with a wider row stride
    and 1e30 padding, at the minimum scratch (several products of 128 frame rows) and at 8 times the minimum (one product)."""
    scales = [(64, 16, 8), (256, 16, 20)]
    n, t = 1000, 1200
    clip, other = signal(n, 41), signal(t, 42)
    est, est_other = 0.9 * clip + 0.01 * signal(n, 43), 0.5 * other
    wide_r, wide_e = torch.full((4, t + 37), 1e30), torch.full((4, t + 37), 1e30)
    lens = [n, n, t, n]
    for i, (a, b) in enumerate([(clip, est), (clip, est), (other, est_other), (clip, est)]):
        wide_r[i, :lens[i]], wide_e[i, :lens[i]] = a, b
    br, be = wide_r.to(DEV)[:, :t], wide_e.to(DEV)[:, :t]
    assert br.stride(0) == t + 37
    ar, ae = clip[None].to(DEV), est[None].to(DEV)
    alone_sm = l3ac_amd.signal_metrics(ar, ae)
    batch_sm = l3ac_amd.signal_metrics(br, be, lengths=lens)
    for k in alone_sm:
        for row in (0, 1, 3):
            assert torch.equal(batch_sm[k][row], alone_sm[k][0]), (k, row)
    alone_d = l3ac_amd.mel_distance(ar, ae, SR, scales=scales, extra_scratch=0)
    for n_fft, hop, n_mels in scales:
        f = 1 + n // hop
        alone_spec = l3ac_amd.stft(ar, n_fft, hop, extra_scratch=0)
        alone_lm = l3ac_amd.log_mel(ar, SR, n_fft, hop, n_mels, extra_scratch=0)
        need = _capi.load_library().l3ac_mel_scratch_bytes(4, t, n_fft, hop, n_mels)
        for extra in (0, 7 * need):
            spec = l3ac_amd.stft(br, n_fft, hop, lengths=lens, extra_scratch=extra)
            lm, _ = l3ac_amd.log_mel(br, SR, n_fft, hop, n_mels, lengths=lens, extra_scratch=extra)
            for row in (0, 1, 3):
                assert torch.equal(torch.view_as_real(spec[row, :f]), torch.view_as_real(alone_spec[0])), (n_fft, extra, row)
                assert torch.equal(lm[row, :f], alone_lm[0]), (n_fft, extra, row)
                assert not torch.view_as_real(spec[row, f:]).any() and not lm[row, f:].any()
    need = max(_capi.load_library().l3ac_mel_scratch_bytes(4, t, n_fft, hop, n_mels) for n_fft, hop, n_mels in scales)
    for extra in (0, 7 * need):  # (8 times the minimum of the larger scale, more for the other)
        d = l3ac_amd.mel_distance(br, be, SR, scales=scales, lengths=lens, extra_scratch=extra)
        for row in (0, 1, 3):
            assert torch.equal(d["per_scale"][row], alone_d["per_scale"][0]) and torch.equal(d["mel_distance"][row], alone_d["mel_distance"][0])


def test_mel_distance_graph_capture_replays_the_eager_bits():
    scales = [(64, 16, 8), (256, 64, 20)]
    lens = [900, 1000]
    r = torch.stack([signal(1000, 51), signal(1000, 52)]).to(DEV)
    e = 0.8 * r + 0.01
    eager = l3ac_amd.mel_distance(r, e, SR, scales=scales, lengths=lens)  # (the warm-up: uploads the tables)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = l3ac_amd.mel_distance(r, e, SR, scales=scales, lengths=lens)
    e.mul_(0.5)  # the replay reads the tensors' current contents ...
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out["per_scale"], eager["per_scale"])
    e.mul_(2.0)  # ... (a power of two: exactly undone)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["per_scale"], eager["per_scale"]) and torch.equal(out["mel_distance"], eager["mel_distance"])


def test_tables_refuse_to_upload_under_capture():
    x = torch.zeros(1, 400, device=DEV)
    l3ac_amd.stft(x, 64, 16)  # this basis is warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside stream capture"):
        with torch.cuda.graph(graph):
            l3ac_amd.stft(x, 64, 16)
            l3ac_amd.stft(x, 48, 12)  # an n_fft no other test uses: its basis is not on the device, raises inside the capture
    torch.cuda.synchronize()
    assert l3ac_amd.stft(x, 48, 12).shape == (1, 34, 25)  # eager, it works (and is warm from now on)


@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_equals_the_composed_calls(codec):
    lens = [4800, 8000]  # 0.3 s and 0.5 s
    audio = torch.zeros(2, 8000)
    for i, n in enumerate(lens):
        audio[i, :n] = signal(n, 60 + i)
    audio = audio.to(DEV)
    # windows of 10 tokens (2700 samples at hop 270); the default look-back, the attention window, is longer than that window, so a
    # 3-token one is named: 18 and 30 tokens are then several chunks each
    kw = dict(process_window=2700, prefix_tokens=3)
    got = codec.evaluate(audio, lengths=lens, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :8000]
    want = l3ac_amd.mel_distance(audio, decoded, sample_rate=codec.config.sample_rate, lengths=lens)
    want.update(l3ac_amd.signal_metrics(audio, decoded, lengths=lens))
    for k, v in want.items():
        assert torch.equal(got[k], v, ) or (torch.isnan(v) & torch.isnan(got[k])).all(), k
        assert v.dtype == torch.float64 and v.is_cuda
    assert torch.isfinite(got["mel_distance"]).all() and torch.isfinite(got["mse"]).all()
    tok = info["lengths"]
    assert torch.equal(got["tokens"], tok)
    bps = bits_per_token(codec.network.mc) * tok.double() / (torch.tensor(lens, dtype=torch.float64) / codec.config.sample_rate)
    assert torch.equal(got["bps"], bps)
    assert set(got) == {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
