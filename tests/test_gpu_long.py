"""Batches of long recordings: encode_long / decode_long against extract_unit / decode_unit on each recording alone, bit for bit, and
the cut / merge kernels against ChunkData on the CPU.  Every comparison is exact."""
import ctypes
import math

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.chunking import ChunkData
from tests.helpers import seeded_audio

pytestmark = pytest.mark.gpu

_CODECS = {}


def _codec(tag):
    if tag not in _CODECS:
        codec = l3ac_amd.get_model(tag, synthetic_seed=0)
        codec.network.to(device="cuda").eval()
        _CODECS[tag] = codec
    return _CODECS[tag]


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------
GUARD = 37  # elements each side of every device buffer; odd, so the buffers themselves start at any 4-byte alignment
SENTINEL = 0x7FC0BEEF  # a NaN as fp32


def _guarded(n_elements):
    """A device buffer of n_elements int32 between two guards, everything set to the sentinel: (whole buffer, the inner view)."""
    whole = torch.full((n_elements + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n_elements]


def _guards_intact(whole, n_elements):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n_elements:] == SENTINEL).all())


CUT_CASES = [
    # (c, chunk_len, prefix_len, round_to, frames of the recordings, extra source stride)
    (1, 3 * 135, 135, 1, [1, 404, 405, 406, 3 * 405, 2 * 405 + 135, 20 * 405 + 77, 17 * 405 + 1, 9000, 45 * 405 + 3, 30 * 405], 3),   # starts 135 * (3 j - 1): odd multiples of an odd hop
    (1, 4 * 270, 2 * 270, 270, [1, 269, 270, 271, 1080, 1081, 5 * 1080 + 500, 3 * 1080 + 1], 1),               # audio: rounded to the hop, zeros written
    (1, 296, 295, 1, [1, 296, 297, 1000], 2),                                                                 # the largest prefix
    (6, 37, 5, 1, [1, 36, 37, 38, 400, 3 * 37], 1),                                                           # level indices: c % 4 != 0
    (6, 37, 0, 1, [75, 2], 3),
    (128, 29, 7, 1, [1, 29, 30, 200, 58], 1),                                                                 # features: always 16-byte accesses
]


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("c,chunk_len,prefix_len,round_to,frames,extra", CUT_CASES)
def test_cut_and_merge_kernels_against_chunkdata(c, chunk_len, prefix_len, round_to, frames, extra, as_float):
    """int32 data, and the same bits as fp32 (random bit patterns, NaNs among them): moved bit for bit either way."""
    lib = _capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    b = len(frames)
    stride = max(frames) + extra
    if c == 1 and stride % 4 == 0:
        stride += 1
    assert c != 1 or stride % 4 != 0  # a source row stride that is not a multiple of 4
    gen = torch.Generator().manual_seed(c * 1000 + chunk_len)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (b, stride, c), generator=gen, dtype=torch.int64).to(torch.int32)
    desc = l3ac_amd.chunk_plan(frames, chunk_len, prefix_len, round_to)
    n = len(desc)
    rounded = [-(-f // round_to) * round_to for f in frames]
    # the CPU reference: ChunkData on each recording's own frames, zero-padded to round_to (Network.preprocess)
    want_rows = []
    for i, f in enumerate(frames):
        own = torch.zeros((rounded[i], c), dtype=torch.int32)
        own[:f] = x[i, :f]
        want_rows += ChunkData(chunk_len=chunk_len, prefix_len=prefix_len, original_data=own).chunk_data
    assert len(want_rows) == n
    if prefix_len == 135:
        assert n > 128  # this case spans more than one launch (ChunkBlock::CAP descriptors each)
    row_frames = chunk_len + prefix_len + 3
    src_whole, src = _guarded(b * stride * c)
    src.copy_(x.reshape(-1))
    dst_whole, dst = _guarded(n * row_frames * c)
    view = (lambda t: t.view(torch.float32)) if as_float else (lambda t: t)
    _capi.check(lib.l3ac_chunk_cut(view(src).data_ptr(), b, stride, c, desc, n, view(dst).data_ptr(), n, row_frames, stream))
    torch.cuda.synchronize()
    rows = dst.cpu().view(n, row_frames, c)
    for j, w in enumerate(want_rows):
        assert torch.equal(rows[j, :w.shape[0]], w), f"chunk {j}"
        assert bool((rows[j, w.shape[0]:] == SENTINEL).all()), f"chunk {j}: written beyond its own frames"
    assert _guards_intact(dst_whole, n * row_frames * c) and _guards_intact(src_whole, b * stride * c)
    assert torch.equal(src.cpu(), x.reshape(-1))

    # merge(cut(x)) == x on each recording's own (rounded) frames, zeros up to out_frames, nothing touched after it
    out_frames = max(rounded) + 2
    out_stride = out_frames + 3
    out_whole, out = _guarded(b * out_stride * c)
    _capi.check(lib.l3ac_chunk_merge(view(dst).data_ptr(), n, row_frames, c, desc, n, view(out).data_ptr(), b, out_stride, out_frames, stream))
    torch.cuda.synchronize()
    got = out.cpu().view(b, out_stride, c)
    for i, f in enumerate(frames):
        assert torch.equal(got[i, :f], x[i, :f]), f"recording {i}"
        assert not got[i, f:out_frames].any(), f"recording {i}: zeros after its end"
        assert bool((got[i, out_frames:] == SENTINEL).all()), f"recording {i}: written beyond out_frames"
    assert _guards_intact(out_whole, b * out_stride * c)
    # the CPU merge of the CPU chunks says the same
    row = 0
    for i, f in enumerate(frames):
        k = sum(1 for d in desc if d.rec == i)
        merged = ChunkData(chunk_len=chunk_len, prefix_len=prefix_len, chunk_data=want_rows[row:row + k]).data
        assert torch.equal(got[i, :rounded[i]], merged)
        row += k


def test_a_slice_of_a_plan_in_any_order_and_descriptors_owned_by_the_call():
    lib = _capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    frames = [1000, 77, 512]
    x = torch.arange(3 * 1000, dtype=torch.int32).reshape(3, 1000) + 1
    desc = l3ac_amd.chunk_plan(frames, 128, 16)
    n = len(desc)
    src = x.cuda()
    rows = torch.full((n, 144), -1, dtype=torch.int32, device="cuda")
    picks = list(range(n - 1, -1, -2))  # every other chunk, last first
    part = (_capi.ChunkDesc * len(picks))(*[desc[j] for j in picks])
    _capi.check(lib.l3ac_chunk_cut(src.data_ptr(), 3, 1000, 1, part, len(picks), rows.data_ptr(), n, 144, stream))
    for d in part:  # the array may change as soon as the call has returned
        d.row, d.start, d.frames = 0, 0, 1
    torch.cuda.synchronize()
    got = rows.cpu()
    for j in range(n):
        d = desc[j]
        if j in picks:
            assert torch.equal(got[j, :d.frames], x[d.rec, d.start:d.start + d.frames]) and bool((got[j, d.frames:] == -1).all())
        else:
            assert bool((got[j] == -1).all())


# ---- 2 - 8. encode_long / decode_long --------------------------------------------------------------------------------------
def _lengths(mc, process_window, short_ok=True):
    """Recording lengths (samples) on the edges of the chunk plan."""
    hop = mc.hop_length
    cl = process_window // hop * hop
    out = [cl, cl + 1, 3 * cl, 2 * cl + hop, 2 * cl + 1, cl + 12345 % cl, 2 * cl - hop - 7]
    out.append(10000 if short_ok else cl - 5 * hop)  # shorter than one chunk
    return out


def _audio(lengths, seed=1234):
    """Rows of seeded audio with garbage after each recording's end: NaN in even rows, 1e30 in odd ones."""
    audio = seeded_audio(len(lengths), max(lengths), seed)
    for i, n in enumerate(lengths):
        audio[i, n:] = float("nan") if i % 2 == 0 else 1e30
    return audio.cuda()


def _alone(codec, clip, process_window, prefix_tokens):
    """extract_unit of one recording, merged; and its level indices, chunk by chunk through encode_audio (extract_unit drops them)."""
    mc = codec.network.mc
    hop = mc.hop_length
    idx, feat = codec.extract_unit(clip, process_window=process_window, prefix_tokens=prefix_tokens)
    padded, _ = codec.network.preprocess(clip)
    chunks = ChunkData(chunk_len=idx.chunk_len * hop, prefix_len=idx.prefix_len * hop, original_data=padded[0]).chunk_data
    li = [codec.encode_audio(ch[None])[1]["level_indices"][0] for ch in chunks]
    return idx, feat, ChunkData(chunk_len=idx.chunk_len, prefix_len=idx.prefix_len, chunk_data=li).data


def _check_encode(codec, audio, lengths, process_window, prefix_tokens, **kw):
    mc = codec.network.mc
    hop = mc.hop_length
    q, ind = codec.encode_long(audio, lengths=lengths, process_window=process_window, prefix_tokens=prefix_tokens, **kw)
    n_tok = math.ceil(audio.shape[1] / hop)
    assert q.shape == (len(lengths), n_tok, mc.feature_dim) and q.dtype == torch.float32
    assert ind["indices"].shape == (len(lengths), n_tok) and ind["indices"].dtype == torch.int32
    assert ind["level_indices"].shape == (len(lengths), n_tok, len(mc.levels)) and ind["level_indices"].dtype == torch.float32
    assert ind["lengths"].dtype == torch.int32 and not ind["lengths"].is_cuda
    assert ind["lengths"].tolist() == [math.ceil(n / hop) for n in lengths]
    for i, n in enumerate(lengths):
        idx, feat, li = _alone(codec, audio[i:i + 1, :n], process_window, prefix_tokens)
        k = math.ceil(n / hop)
        assert idx.data.shape[0] == k
        assert torch.equal(ind["indices"][i, :k], idx.data), f"recording {i} ({n} samples): indices"
        assert torch.equal(q[i, :k], feat.data), f"recording {i} ({n} samples): q_feature"
        assert torch.equal(ind["level_indices"][i, :k], li), f"recording {i} ({n} samples): level_indices"
        assert not q[i, k:].any() and not ind["indices"][i, k:].any() and not ind["level_indices"][i, k:].any()
    return q, ind


def _check_decode(codec, q, ind, process_window, prefix_tokens, **kw):
    mc = codec.network.mc
    hop = mc.hop_length
    tok = ind["lengths"].tolist()
    wi = codec.decode_long(indices=ind["indices"], lengths=tok, process_window=process_window, prefix_tokens=prefix_tokens, **kw)
    wq = codec.decode_long(q, lengths=tok, process_window=process_window, prefix_tokens=prefix_tokens, **kw)
    assert wi.shape == (len(tok), q.shape[1] * hop) and wi.dtype == torch.float32
    assert torch.equal(wi, wq)
    cl = process_window // hop
    p = mc.en_coder_window_size if prefix_tokens is None else prefix_tokens
    for i, k in enumerate(tok):
        # the merged stream cut again the way decode_long cuts it (not extract_unit's own chunks: their prefix tokens are the
        # chunk's own encoding of the overlap, which merging drops)
        alone_i = codec.decode_unit(chunk_indices=ChunkData(cl, p, original_data=ind["indices"][i, :k]))
        alone_q = codec.decode_unit(chunk_q_feature=ChunkData(cl, p, original_data=q[i, :k]))
        assert torch.equal(wi[i, :k * hop], alone_i[0]), f"recording {i} ({k} tokens): decode from indices"
        assert torch.equal(wq[i, :k * hop], alone_q[0]), f"recording {i} ({k} tokens): decode from q_feature"
        assert not wi[i, k * hop:].any()
    return wi


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("prefix_tokens", [1, 30])
def test_long_batch_equals_each_recording_alone_1kbps(split, prefix_tokens):
    codec = _codec("1kbps")
    before = codec.network.gemm_split
    codec.network.set_gemm_split(split)
    try:
        lengths = _lengths(codec.network.mc, 2 * 16000)
        audio = _audio(lengths)
        q, ind = _check_encode(codec, audio, lengths, 2 * 16000, prefix_tokens)
        _check_decode(codec, q, ind, 2 * 16000, prefix_tokens)
    finally:
        codec.network.set_gemm_split(before)


@pytest.mark.parametrize("split", [True, False])
def test_long_batch_default_prefix_and_a_window_just_above_it(split):
    codec = _codec("1kbps")
    mc = codec.network.mc
    before = codec.network.gemm_split
    codec.network.set_gemm_split(split)
    try:
        window = (mc.en_coder_window_size + 1) * mc.hop_length + 100  # chunks of window_size + 1 tokens: one new token per chunk
        lengths = [window // mc.hop_length * mc.hop_length + extra for extra in (0, 1, 5 * mc.hop_length, 3 * mc.hop_length + 7)] + [5000]
        audio = _audio(lengths, seed=77)
        q, ind = _check_encode(codec, audio, lengths, window, None)
        _check_decode(codec, q, ind, window, None)
    finally:
        codec.network.set_gemm_split(before)


def test_long_batch_equals_each_recording_alone_3kbps():
    codec = _codec("3kbps")
    lengths = _lengths(codec.network.mc, 2 * 16000, short_ok=True)
    audio = _audio(lengths, seed=5)
    q, ind = _check_encode(codec, audio, lengths, 2 * 16000, 30)
    _check_decode(codec, q, ind, 2 * 16000, 30)


def test_result_does_not_depend_on_grouping_or_order():
    codec = _codec("1kbps")
    lengths = _lengths(codec.network.mc, 2 * 16000)
    audio = _audio(lengths, seed=3)
    kw = dict(process_window=2 * 16000, prefix_tokens=30)
    q0, i0 = codec.encode_long(audio, lengths=lengths, **kw)
    w0 = codec.decode_long(indices=i0["indices"], lengths=i0["lengths"], **kw)
    for per_call in (1, 3):
        q, ind = codec.encode_long(audio, lengths=lengths, chunks_per_call=per_call, **kw)
        assert torch.equal(q, q0) and torch.equal(ind["indices"], i0["indices"]) and torch.equal(ind["level_indices"], i0["level_indices"])
        assert torch.equal(codec.decode_long(indices=ind["indices"], lengths=ind["lengths"], chunks_per_call=per_call, **kw), w0)
        assert torch.equal(codec.decode_long(q, lengths=ind["lengths"], chunks_per_call=per_call, **kw), w0)
    perm = torch.randperm(len(lengths), generator=torch.Generator().manual_seed(5)).tolist()
    qp, ip = codec.encode_long(audio[perm], lengths=[lengths[p] for p in perm], **kw)
    assert torch.equal(qp, q0[perm]) and torch.equal(ip["indices"], i0["indices"][perm]) and torch.equal(ip["lengths"], i0["lengths"][perm])
    assert torch.equal(codec.decode_long(indices=ip["indices"], lengths=ip["lengths"], **kw), w0[perm])
    # lengths absent: every row is T long
    full = seeded_audio(2, 40000, 9).cuda()
    qa, ia = codec.encode_long(full, **kw)
    qb, ib = codec.encode_long(full, lengths=[40000, 40000], **kw)
    assert torch.equal(qa, qb) and torch.equal(ia["indices"], ib["indices"]) and ia["lengths"].tolist() == ib["lengths"].tolist()
    assert torch.equal(codec.decode_long(indices=ia["indices"], **kw), codec.decode_long(indices=ia["indices"], lengths=ia["lengths"], **kw))


def test_one_window_over_everything_is_the_ragged_call():
    codec = _codec("1kbps")
    lengths = [16000, 4321, 270, 8100, 17280, 30000]
    audio = _audio(lengths, seed=42)
    window = 30000 + 270  # one chunk holds the longest recording
    q, ind = codec.encode_long(audio, lengths=lengths, process_window=window, prefix_tokens=3)
    qr, indr = codec.encode_audio(audio, lengths=lengths)
    assert torch.equal(q, qr) and torch.equal(ind["indices"], indr["indices"]) and torch.equal(ind["level_indices"], indr["level_indices"])
    assert torch.equal(ind["lengths"], indr["lengths"])
    tok = ind["lengths"].tolist()
    assert torch.equal(codec.decode_long(indices=ind["indices"], lengths=tok, process_window=window, prefix_tokens=3),
                       codec.decode_audio(indices=ind["indices"], lengths=tok))
    assert torch.equal(codec.decode_long(q, lengths=tok, process_window=window, prefix_tokens=3), codec.decode_audio(q, lengths=tok))


def test_sample_rate_composes_as_in_the_ragged_calls():
    codec = _codec("1kbps")
    sr = codec.config.sample_rate
    lengths = [3 * 48000, 150000, 61234, 999]
    audio = _audio(lengths, seed=8)
    kw = dict(process_window=2 * 16000, prefix_tokens=30)
    q, ind = codec.encode_long(audio, lengths=lengths, sample_rate=48000, **kw)
    masked = audio.clone()
    for i, n in enumerate(lengths):
        masked[i, n:] = 0.0
    lens16 = [l3ac_amd.resample_length(48000, sr, n) for n in lengths]
    q2, ind2 = codec.encode_long(l3ac_amd.resample(masked, 48000, sr), lengths=lens16, **kw)
    assert torch.equal(q, q2) and torch.equal(ind["indices"], ind2["indices"]) and torch.equal(ind["lengths"], ind2["lengths"])
    tok = ind["lengths"].tolist()
    wave = codec.decode_long(indices=ind["indices"], lengths=tok, sample_rate=44100, **kw)
    plain = l3ac_amd.resample(codec.decode_long(indices=ind["indices"], lengths=tok, **kw), sr, 44100)
    assert wave.shape == plain.shape
    for i, k in enumerate(tok):
        m = l3ac_amd.resample_length(sr, 44100, k * codec.network.mc.hop_length)
        assert torch.equal(wave[i, :m], plain[i, :m]) and not wave[i, m:].any()
    assert torch.equal(codec.decode_long(q, lengths=tok, sample_rate=44100, **kw), wave)


def test_graph_capture_replays_on_new_inputs():
    codec = _codec("1kbps")
    mc = codec.network.mc
    hop = mc.hop_length
    ctx = codec.network.context()
    lengths = [70000, 31860, 31861, 95000, 5000]
    kw = dict(process_window=2 * 16000, prefix_tokens=30, chunks_per_call=4)
    row_samples = (2 * 16000) // hop * hop + 30 * hop
    ctx.reserve(4, row_samples)
    inputs = [_audio(lengths, seed=s) for s in (21, 22, 23)]
    eager = []
    for a in inputs:
        q, ind = codec.encode_long(a, lengths=lengths, **kw)
        eager.append((q, ind["indices"], codec.decode_long(indices=ind["indices"], lengths=ind["lengths"], **kw)))
    static_in = inputs[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # the warm-up call
        qw, iw = codec.encode_long(static_in, lengths=lengths, **kw)
        codec.decode_long(indices=iw["indices"], lengths=iw["lengths"], **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qg, ig = codec.encode_long(static_in, lengths=lengths, **kw)
        wg = codec.decode_long(indices=ig["indices"], lengths=ig["lengths"], **kw)
    codec.encode_audio(inputs[0][:, :100], lengths=[1] * len(lengths))  # other lengths in the workspace between capture and replay
    for a, (q, idx, w) in zip(inputs[1:], eager[1:]):
        static_in.copy_(a)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(qg, q) and torch.equal(ig["indices"], idx) and torch.equal(wg, w)


def test_errors():
    codec = _codec("1kbps")
    mc = codec.network.mc
    kw = dict(process_window=2 * 16000, prefix_tokens=30)
    audio = seeded_audio(2, 40000, 1).cuda()
    with pytest.raises(RuntimeError, match="is on cpu"):
        codec.encode_long(audio.cpu(), **kw)
    q, ind = codec.encode_long(audio, lengths=[40000, 33000], **kw)
    with pytest.raises(RuntimeError, match="is on cpu"):
        codec.decode_long(indices=ind["indices"].cpu(), **kw)
    with pytest.raises(ValueError, match="audio_feature or indices"):
        codec.decode_long(**kw)
    with pytest.raises(ValueError, match="must exceed the overlap"):
        codec.encode_long(audio, process_window=30 * mc.hop_length, prefix_tokens=30)
    codec.network.training = True
    try:
        with pytest.raises(RuntimeError, match="eval"):
            codec.encode_long(audio, **kw)
        with pytest.raises(RuntimeError, match="eval"):
            codec.decode_long(indices=ind["indices"], **kw)
    finally:
        codec.network.eval()
    # an out-of-range index inside a recording is met (in its chunk, and again where it is another chunk's prefix); after its end, never
    ctx = codec.network.context()
    tok = ind["lengths"].tolist()
    bad = ind["indices"].clone()
    bad[1, tok[1] - 1] = 10 ** 7
    with pytest.raises(ValueError, match="1 index occurrences"):
        codec.decode_long(indices=bad, lengths=tok, validate=True, **kw)
    bad = ind["indices"].clone()
    cl = (2 * 16000) // mc.hop_length
    bad[0, cl - 1] = -5  # the last token of chunk 0 is also in chunk 1's prefix
    with pytest.raises(ValueError, match="2 index occurrences"):
        codec.decode_long(indices=bad, lengths=tok, validate=True, **kw)
    good = codec.decode_long(indices=ind["indices"], lengths=tok, validate=True, **kw)
    bad = ind["indices"].clone()
    bad[1, tok[1]:] = 10 ** 7
    before = ctx.bad_index_count()
    assert torch.equal(codec.decode_long(indices=bad, lengths=tok, validate=True, **kw), good)
    assert ctx.bad_index_count() == before
    # a chunk of one frame (3kbps: en_coder_compress_rate = 1) is refused before any device work, as in decode_audio
    codec3 = _codec("3kbps")
    assert codec3.network.mc.en_coder_compress_rate == 1
    idx3 = torch.zeros(2, 40, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        codec3.decode_long(indices=idx3, lengths=[40, 13], process_window=6 * codec3.network.mc.hop_length, prefix_tokens=0)


def test_grn_exact_network_refuses():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.grn_exact = True
    codec.network.to(device="cuda").eval()
    audio = seeded_audio(2, 40000).cuda()
    with pytest.raises(_capi.L3acError, match="grn_exact"):
        codec.encode_long(audio, process_window=2 * 16000, prefix_tokens=30)
    idx = torch.zeros(2, 149, dtype=torch.int32, device="cuda")
    with pytest.raises(_capi.L3acError, match="grn_exact"):
        codec.decode_long(indices=idx, process_window=2 * 16000, prefix_tokens=30)
