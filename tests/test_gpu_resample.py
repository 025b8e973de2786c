"""Sample-rate conversion on the MI355X (kernels/resample.hip): accuracy against the fp64 restatement (tests/resample_ref.py)
within the a-priori bound of an fp32 dot product, bit-exact batch / stride / run invariance, the codec's ``sample_rate=``
keyword, and graph capture."""
import numpy as np
import pytest
import torch

import l3ac_amd
from tests import resample_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000), (11025, 16000), (22050, 16000), (44100, 48000),
         (192000, 16000), (16000, 8000)]
EPS = 2.0 ** -24


def signals(rate, n, seed):
    """(name, (B, n) fp32) test signals: seeded noise, full-scale sines just below the new Nyquist, silence, impulses at both ends."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / rate
    nyq = min(rate, 16000) / 2
    sines = torch.stack([torch.sin(2 * np.pi * f * t + p) for f, p in ((0.97 * nyq, 0.3), (0.999 * nyq, 1.1))]).float()
    imp = torch.zeros(2, n)
    imp[0, 0] = 1.0
    imp[1, -1] = -1.0
    return [("noise", torch.randn(3, n, generator=g) * 0.3), ("sine", sines), ("silence", torch.zeros(1, n)), ("impulse", imp)]


def bound_ratio(y, x, a, b):
    ref, absdot = R.resample_ref(x.double().numpy(), a, b)
    _, K, _ = R.polyphase_taps(a, b)
    err = np.abs(y.double().cpu().numpy() - ref)
    bound = (K + 2) * EPS * absdot
    ok = err <= bound
    return ok.all(), float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0)))), err.max()


@pytest.mark.parametrize("a,b", PAIRS)
def test_resample_within_fp32_dot_bound(a, b):
    worst = 0.0
    for n in (1, 7, 333, a // 4 + 13):
        for name, x in signals(a, n, seed=n + a):
            y = l3ac_amd.resample(x.to(DEV), a, b)
            assert y.shape == (x.shape[0], R.out_length(a, b, n))
            ok, ratio, err = bound_ratio(y, x, a, b)
            assert ok, f"{a}->{b} n={n} {name}: max err {err:.3e}, worst err / bound {ratio:.3f}"
            worst = max(worst, ratio)
            if name == "silence":
                assert not y.any()
    print(f"\n[resample] {a} -> {b}: worst |err| / ((K + 2) 2^-24 sum|h x|) = {worst:.4f}")


def test_resample_equal_rates_is_a_copy():
    x = torch.randn(3, 1001, device=DEV)
    y = l3ac_amd.resample(x, 44100, 44100)
    assert y.data_ptr() != x.data_ptr() and torch.equal(x, y)


@pytest.mark.parametrize("a,b", [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000)])
def test_resample_batch_stride_and_run_invariant(a, b):
    """A clip's bits do not depend on the batch, its position in it, the input's row stride or the run."""
    n = a  # one second
    g = torch.Generator().manual_seed(5)
    big = (torch.randn(256, n, generator=g) * 0.3).to(DEV)
    y_all = l3ac_amd.resample(big, a, b)
    for i in (0, 63, 64, 200, 255):
        assert torch.equal(l3ac_amd.resample(big[i:i + 1], a, b)[0], y_all[i]), i
    wide = torch.zeros(256, n + 37, device=DEV)
    wide[:, :n] = big
    assert torch.equal(l3ac_amd.resample(wide[:, :n], a, b), y_all)
    assert torch.equal(l3ac_amd.resample(big[17:50], a, b), y_all[17:50])
    assert torch.equal(l3ac_amd.resample(big, a, b), y_all)  # run to run


@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def _audio(b, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, n, generator=g) * 0.1).to(DEV)


@pytest.mark.parametrize("rate", [44100, 48000])
def test_encode_decode_sample_rate_keyword(codec, rate):
    x = _audio(4, rate + 321)
    q, ind = codec.encode_audio(x, sample_rate=rate)
    q_ref, ind_ref = codec.encode_audio(l3ac_amd.resample(x, rate, 16000))
    assert torch.equal(q, q_ref) and torch.equal(ind["indices"], ind_ref["indices"])
    assert torch.equal(ind["level_indices"], ind_ref["level_indices"])
    wave = codec.decode_audio(q, sample_rate=rate)
    wave16 = codec.decode_audio(q)
    assert wave.shape == (4, l3ac_amd.resample_length(16000, rate, q.shape[1] * codec.network.mc.hop_length))
    assert torch.equal(wave, l3ac_amd.resample(wave16, 16000, rate))
    assert torch.equal(codec.decode_audio(indices=ind["indices"], sample_rate=rate), wave)


def test_native_rate_keyword_is_the_plain_path(codec):
    x = _audio(3, 16000 + 77)
    q, ind = codec.encode_audio(x)
    for sr in (None, 16000):
        q2, ind2 = codec.encode_audio(x, sample_rate=sr)
        assert torch.equal(q, q2) and torch.equal(ind["indices"], ind2["indices"])
        assert torch.equal(codec.decode_audio(q, sample_rate=sr), codec.decode_audio(q))


def test_graph_capture_of_resampled_encode_decode(codec):
    """Encode at 48 kHz + decode to 44.1 kHz for 32 clips, captured after one eager call, replays to the eager bits."""
    x = _audio(32, 48000, seed=11)
    static_x = x.clone()

    def step():
        q, _ = codec.encode_audio(static_x, sample_rate=48000)
        return codec.decode_audio(q, sample_rate=44100)

    eager = step()  # warm-up: uploads both banks, sizes the workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static_x.copy_(_audio(32, 48000, seed=12))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, step())


def test_cold_rate_pair_under_capture_raises():
    """A rate pair whose bank is not on the device yet cannot be uploaded inside a capture: a clear error, raised before anything is
    enqueued, and the capture itself still ends cleanly."""
    x = torch.randn(2, 24000, device=DEV)
    l3ac_amd.resample(x, 24000, 16000)  # this pair is warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="not on"):
        with torch.cuda.graph(g):
            l3ac_amd.resample(x, 24000, 16000)
            l3ac_amd.resample(x, 32000, 16000)  # cold: raises inside the capture
    torch.cuda.synchronize()
    y = l3ac_amd.resample(x, 32000, 16000)  # eager, the pair works (and is warm from now on)
    assert y.shape == (2, 12000)
