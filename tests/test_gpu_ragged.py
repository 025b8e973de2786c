"""Ragged batches: encode_audio / decode_audio(lengths=...) against the same clips run alone, bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd import weights as W
from tests.helpers import index_mismatch_report, seeded_audio

pytestmark = pytest.mark.gpu

TAU = 1e-4  # as tests/test_gpu_e2e.py: a flipped index must come from a latent within TAU of a rounding boundary

_CODECS = {}


def _codec(tag):
    if tag not in _CODECS:
        codec = l3ac_amd.get_model(tag, synthetic_seed=0)
        codec.network.to(device="cuda").eval()
        _CODECS[tag] = codec
    return _CODECS[tag]


def _boundary_lengths(mc, seed=7):
    """About 30 clip lengths (samples) on the edges the pipeline's forms change at: one sample, one hop, the transformer stack's
    frame limit at the en_encoder input (180 / 192 / 193 frames), one attention window of tokens, several windows; plus random ones."""
    hop, r, win = mc.hop_length, mc.en_coder_compress_rate, mc.en_coder_window_size
    out = [1, hop - 1, hop, hop + 1, 2 * hop + 3]
    for frames in (180, 192, 193):
        n = -(-frames // r)
        out += [n * hop, n * hop - hop // 2]
    out += [(win - 1) * hop + 5, win * hop, win * hop + 1, (win + 1) * hop, 3 * win * hop + 17]
    rng = np.random.default_rng(seed)
    out += [int(v) for v in rng.integers(1, max(out) + 1, size=12)]
    return out


def _audio(lengths, fill, seed=1234):
    t = max(lengths)
    audio = seeded_audio(len(lengths), t, seed)
    for i, n in enumerate(lengths):
        audio[i, n:] = fill
    return audio.cuda()


def _min_tok(mc):
    return -(-2 // mc.en_coder_compress_rate)  # decode needs n_tok * en_coder_compress_rate >= 2


@pytest.mark.parametrize("tag", ["1kbps", "3kbps", "1k5bps"])
@pytest.mark.parametrize("split", [True, False])
def test_ragged_batch_equals_each_clip_alone(tag, split):
    codec = _codec(tag)
    mc = codec.network.mc
    before = codec.network.gemm_split
    codec.network.set_gemm_split(split)
    try:
        lengths = _boundary_lengths(mc)
        audio = _audio(lengths, float("nan"))  # whatever lies after a clip's end is never read
        q, ind = codec.encode_audio(audio, lengths=lengths)
        n_tok = ind["lengths"].tolist()
        assert n_tok == [math.ceil(n / mc.hop_length) for n in lengths] and ind["lengths"].dtype == torch.int32
        assert q.shape[1] == math.ceil(max(lengths) / mc.hop_length)
        for i, n in enumerate(lengths):
            qa, ia = codec.encode_audio(audio[i:i + 1, :n])
            k = n_tok[i]
            assert torch.equal(q[i, :k], qa[0]), f"clip {i} ({n} samples): q_feature"
            assert torch.equal(ind["indices"][i, :k], ia["indices"][0]), f"clip {i} ({n} samples): indices"
            assert torch.equal(ind["level_indices"][i, :k], ia["level_indices"][0]), f"clip {i} ({n} samples): level_indices"
            assert not q[i, k:].any() and not ind["indices"][i, k:].any() and not ind["level_indices"][i, k:].any()
        # decode: each clip's first n tokens alone (clips too short to decode alone get the fewest tokens that can be)
        nd = [max(k, _min_tok(mc)) for k in n_tok]
        hop = mc.hop_length
        wi = codec.decode_audio(indices=ind["indices"], lengths=nd)
        wq = codec.decode_audio(q, lengths=nd)
        assert wi.shape == (len(lengths), q.shape[1] * hop)
        for i, k in enumerate(nd):
            alone_i = codec.decode_audio(indices=ind["indices"][i:i + 1, :k])
            alone_q = codec.decode_audio(q[i:i + 1, :k])
            assert torch.equal(wi[i, :k * hop], alone_i[0]), f"clip {i} ({k} tokens): decode from indices"
            assert torch.equal(wq[i, :k * hop], alone_q[0]), f"clip {i} ({k} tokens): decode from q_feature"
            assert not wi[i, k * hop:].any() and not wq[i, k * hop:].any()
    finally:
        codec.network.set_gemm_split(before)


def test_padding_and_neighbours_do_not_leak_in():
    codec = _codec("1kbps")
    mc = codec.network.mc
    ctx = codec.network.context()
    lengths = _boundary_lengths(mc, seed=11)[:20]
    q0, i0 = codec.encode_audio(_audio(lengths, 0.0), lengths=lengths)
    for fill in (float("nan"), 1e30, -1e30):
        q, ind = codec.encode_audio(_audio(lengths, fill), lengths=lengths)
        assert torch.equal(q, q0) and torch.equal(ind["indices"], i0["indices"]) and torch.equal(ind["level_indices"], i0["level_indices"])
    # decode: tokens after a clip's own are out of range or garbage; they change nothing and are never counted
    nd = [max(k, _min_tok(mc)) for k in i0["lengths"].tolist()]
    w0 = codec.decode_audio(indices=i0["indices"], lengths=nd)
    wq0 = codec.decode_audio(q0, lengths=nd)
    bad_idx = i0["indices"].clone()
    bad_q = q0.clone()
    for i, k in enumerate(nd):
        bad_idx[i, k:] = torch.tensor([10 ** 7, -3], dtype=torch.int32, device="cuda").repeat(bad_idx.shape[1])[: bad_idx.shape[1] - k]
        bad_q[i, k:] = float("nan")
    before = ctx.bad_index_count()
    assert torch.equal(codec.decode_audio(indices=bad_idx, lengths=nd, validate=True), w0)
    assert ctx.bad_index_count() == before
    assert torch.equal(codec.decode_audio(bad_q, lengths=nd), wq0)
    # permuting the clips permutes the outputs
    perm = torch.randperm(len(lengths), generator=torch.Generator().manual_seed(5)).tolist()
    audio = _audio(lengths, 0.0)
    qp, ip = codec.encode_audio(audio[perm], lengths=[lengths[p] for p in perm])
    assert torch.equal(qp, q0[perm]) and torch.equal(ip["indices"], i0["indices"][perm])
    wp = codec.decode_audio(indices=ip["indices"], lengths=[nd[p] for p in perm])
    assert torch.equal(wp, w0[perm])


def test_256_clip_batch_agrees_with_ragged_sub_batches():
    codec = _codec("1kbps")
    rng = np.random.default_rng(3)
    lengths = [int(v) for v in rng.integers(8000, 32001, size=256)]  # 0.5 - 2 s
    audio = _audio(lengths, 0.0, seed=99)
    q, ind = codec.encode_audio(audio, lengths=lengths)
    w = codec.decode_audio(indices=ind["indices"], lengths=ind["lengths"])
    for b0 in range(0, 256, 64):
        sub = lengths[b0:b0 + 64]
        t = max(sub)
        qs, ins = codec.encode_audio(audio[b0:b0 + 64, :t], lengths=sub)
        k = qs.shape[1]
        assert torch.equal(qs, q[b0:b0 + 64, :k]) and torch.equal(ins["indices"], ind["indices"][b0:b0 + 64, :k])
        ws = codec.decode_audio(indices=ins["indices"], lengths=ins["lengths"])
        assert torch.equal(ws, w[b0:b0 + 64, :ws.shape[1]])


@pytest.mark.parametrize("split", [True, False])
def test_uniform_lengths_give_the_plain_bits(split):
    codec = _codec("3kbps")
    before = codec.network.gemm_split
    codec.network.set_gemm_split(split)
    try:
        audio = seeded_audio(6, 16000).cuda()
        q, ind = codec.encode_audio(audio)
        qr, indr = codec.encode_audio(audio, lengths=[16000] * 6)
        assert torch.equal(q, qr) and torch.equal(ind["indices"], indr["indices"])
        assert torch.equal(ind["level_indices"], indr["level_indices"])
        n = q.shape[1]
        assert torch.equal(codec.decode_audio(q), codec.decode_audio(q, lengths=[n] * 6))
        assert torch.equal(codec.decode_audio(indices=ind["indices"]), codec.decode_audio(indices=ind["indices"], lengths=[n] * 6))
    finally:
        codec.network.set_gemm_split(before)


def test_graph_capture_and_host_lengths_owned_by_the_call():
    codec = _codec("1kbps")
    ctx = codec.network.context()
    lengths = [16000, 5000, 27000, 270, 12345, 31999]
    t = max(lengths)
    ctx.reserve(len(lengths), t)
    audio = _audio(lengths, 0.0)
    q0, i0 = codec.encode_audio(audio, lengths=lengths)
    nd = i0["lengths"].tolist()
    w0 = codec.decode_audio(indices=i0["indices"], lengths=nd)
    # the C entry with a host array that is overwritten as soon as the call has returned
    b, n = len(lengths), q0.shape[1]
    q = torch.empty_like(q0)
    idx = torch.empty_like(i0["indices"])
    li = torch.empty_like(i0["level_indices"])
    host = (ctypes.c_int32 * b)(*lengths)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(ctx.lib.l3ac_encode_ragged(ctx.handle, audio.data_ptr(), b, t, t, host, q.data_ptr(), idx.data_ptr(), li.data_ptr(),
                                           stream))
    for i in range(b):
        host[i] = 1
    wave = torch.empty_like(w0)
    toks = (ctypes.c_int32 * b)(*nd)
    _capi.check(ctx.lib.l3ac_decode_ragged(ctx.handle, None, idx.data_ptr(), b, n, toks, wave.data_ptr(), stream))
    for i in range(b):
        toks[i] = n
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and torch.equal(idx, i0["indices"]) and torch.equal(wave, w0)
    # captured: the graph replays the lengths it was captured with
    static_in = torch.zeros_like(audio)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        codec.encode_audio(static_in, lengths=lengths)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qg, ig = codec.encode_audio(static_in, lengths=lengths)
        wg = codec.decode_audio(indices=ig["indices"], lengths=nd)
    codec.encode_audio(audio[:, :100], lengths=[1] * b)  # other lengths in the workspace between capture and replay
    for _ in range(2):
        static_in.copy_(audio)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(qg, q0) and torch.equal(ig["indices"], i0["indices"]) and torch.equal(wg, w0)


def test_ragged_clips_against_the_oracle():
    from oracle import l3ac_oracle as O
    codec = _codec("1kbps")
    mc = codec.network.mc
    w = W.folded_weights(codec.network.state_dicts())
    lengths = [16000, 4321, 270, 8100, 17280, 30000]
    audio = _audio(lengths, float("nan"), seed=42)
    _, ind = codec.encode_audio(audio, lengths=lengths)
    n_bad_total = 0
    for i, n in enumerate(lengths):
        taps = {}
        _, ind_ref = O.encode_audio(w, mc, audio[i:i + 1, :n].cpu(), taps=taps)
        k = int(ind["lengths"][i])
        n_bad, ok = index_mismatch_report(ind["indices"][i:i + 1, :k].cpu().numpy(), ind_ref["indices"].numpy(), taps["latents"].numpy(),
                                          mc.levels, TAU)
        assert ok
        n_bad_total += n_bad
    print(f"[ragged vs oracle] index mismatches: {n_bad_total}")
    assert n_bad_total == 0


def test_sample_rate_with_lengths_equals_each_clip_alone():
    codec = _codec("1kbps")
    mc = codec.network.mc
    lengths = [48000, 15000, 61234, 999]
    audio = _audio(lengths, float("nan"), seed=8)
    q, ind = codec.encode_audio(audio, sample_rate=48000, lengths=lengths)
    for i, n in enumerate(lengths):
        qa, ia = codec.encode_audio(audio[i:i + 1, :n], sample_rate=48000)
        k = int(ind["lengths"][i])
        assert k == qa.shape[1] == math.ceil(l3ac_amd.resample_length(48000, 16000, n) / mc.hop_length)
        assert torch.equal(q[i, :k], qa[0]) and torch.equal(ind["indices"][i, :k], ia["indices"][0])
    nd = ind["lengths"].tolist()
    wave = codec.decode_audio(indices=ind["indices"], lengths=nd, sample_rate=44100)
    for i, k in enumerate(nd):
        alone = codec.decode_audio(indices=ind["indices"][i:i + 1, :k], sample_rate=44100)
        m = alone.shape[1]
        assert m == l3ac_amd.resample_length(16000, 44100, k * mc.hop_length)
        assert torch.equal(wave[i, :m], alone[0]) and not wave[i, m:].any()


def test_argument_errors_before_any_device_work():
    codec = _codec("1kbps")
    mc = codec.network.mc
    audio = seeded_audio(3, 5000).cuda()
    for bad in ([0, 5000, 5000], [5001, 10, 10], [10, 10], [10, 10, 10, 10], [1.5, 10, 10]):
        with pytest.raises(ValueError):
            codec.encode_audio(audio, lengths=bad)
    q, ind = codec.encode_audio(audio)
    n = q.shape[1]
    for bad in ([0, n, n], [n + 1, n, n], [n, n]):
        with pytest.raises(ValueError):
            codec.decode_audio(q, lengths=bad)
    if _min_tok(mc) > 1:
        with pytest.raises(ValueError):
            codec.decode_audio(indices=ind["indices"], lengths=[1, n, n])
    # the C entries refuse the same without touching the device
    ctx = codec.network.context()
    out = torch.empty_like(q)
    idx = torch.empty_like(ind["indices"])
    lib = ctx.lib
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.l3ac_encode_ragged(ctx.handle, audio.data_ptr(), 3, 5000, 5000, (ctypes.c_int32 * 3)(5000, 0, 1), out.data_ptr(),
                                  idx.data_ptr(), None, stream) == -1
    assert "samples[1]" in lib.l3ac_last_error().decode()
    wave = torch.empty(3, n * mc.hop_length, device="cuda")
    assert lib.l3ac_decode_ragged(ctx.handle, q.data_ptr(), None, 3, n, (ctypes.c_int32 * 3)(n, n, n + 1), wave.data_ptr(), stream) == -1
    assert "n_tok[2]" in lib.l3ac_last_error().decode()


def test_grn_exact_context_refuses_ragged_calls():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.grn_exact = True
    codec.network.to(device="cuda").eval()
    audio = seeded_audio(2, 5000).cuda()
    with pytest.raises(_capi.L3acError, match="error -1:.*grn_exact"):
        codec.encode_audio(audio, lengths=[5000, 300])
    q, ind = codec.encode_audio(audio)
    with pytest.raises(_capi.L3acError, match="error -1:.*grn_exact"):
        codec.decode_audio(indices=ind["indices"], lengths=[q.shape[1], 2])
