"""Streaming sample-rate conversion on the GPU: the kernel through its C entry (guards, inputs untouched, the next
state against a NumPy restatement), StreamResampler against l3ac_amd.resample of each whole stream however it is split over pushes and
whatever the other streams do, and the chains resampler -> stream_encoder / stream_decoder -> resampler against encode_long / decode_long
with sample_rate=.  Every comparison is exact.  No test feeds non-finite samples INSIDE a stream: they are outside the guarantee."""
import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.streaming import ResampleState, resample_advance, resample_geometry
from tests.helpers import seeded_audio

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000), (44100, 48000), (48000, 8000)]
LENGTHS = [1, 2999, 3000, 4801]  # below one filter length; one under and at a multiple of `down` (3, 6, 1: 48 kHz and 16 kHz inputs); over it
_CACHE = {}


def _streams(pair):
    """The test streams and resample of each alone (computed once per pair and shared, never changed)."""
    if pair not in _CACHE:
        audio = seeded_audio(len(LENGTHS), max(LENGTHS), seed=pair[0] % 1000 + pair[1] % 7).cuda()
        want = [l3ac_amd.resample(audio[i:i + 1, :n].contiguous(), *pair)[0] for i, n in enumerate(LENGTHS)]
        assert all(w.shape[0] == l3ac_amd.resample_length(*pair, n) and bool(w.abs().sum() > 0) for w, n in zip(want, LENGTHS))
        _CACHE[pair] = (audio, want)
    return _CACHE[pair]


def _garbage(shape):
    buf = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    buf[1::2] = 1e30
    return buf


def _packets(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def _drive(rs, data, packets, first_call=0, end_with_last=True):
    """Feed stream i its packets[i], one per call from call first_call[i] on, with garbage after each packet's end; a stream ends with its
    last packet (or, end_with_last=False, with an empty push one call later) and idles before and afterwards.  Returns per stream the
    concatenation of what it emitted, checking shapes, counts and the zeros behind every stream's outputs on the way."""
    s = rs.streams
    first = [first_call] * s if isinstance(first_call, int) else first_call
    packets = [list(p) + ([] if end_with_last or not p else [0]) for p in packets]
    pos = [0] * s
    parts = [[] for _ in range(s)]
    for j in range(max(f + len(p) for f, p in zip(first, packets))):
        sizes = [p[j - f] if 0 <= j - f < len(p) else 0 for f, p in zip(first, packets)]
        ends = [j - f == len(p) - 1 for f, p in zip(first, packets)]
        buf = _garbage((s, max(sizes) + (j % 2)))
        for i in range(s):
            buf[i, :sizes[i]] = data[i, pos[i]:pos[i] + sizes[i]]
            pos[i] += sizes[i]
        y, n = rs.push(buf, lengths=sizes, end=ends)
        assert n.dtype == torch.int32 and not n.is_cuda and y.dtype == torch.float32 and y.shape == (s, int(n.max()))
        for i, k in enumerate(n.tolist()):
            assert not y[i, k:].any()
            parts[i].append(y[i, :k])
    return [torch.cat(p) for p in parts]


# ---- 1. the kernel through the C entry ---------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF  # a NaN as fp32


def _guarded(n_elements, guard):
    whole = torch.full((n_elements + 2 * guard,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole[guard:guard + n_elements]


def _guards_intact(whole, n_elements, guard):
    return bool((whole[:guard] == SENTINEL).all()) and bool((whole[guard + n_elements:] == SENTINEL).all())


@pytest.mark.parametrize("pair", [(44100, 16000), (48000, 8000), (16000, 48000)])
def test_kernel_against_numpy_and_resample(pair):
    """Four streams in the middle of their lives — one young (its window starts before its first sample), one idle, one steady, one ending
    — in buffers that start 4 bytes apart (guards of 37 and 38 elements: dword and 16-byte copy paths), rows longer than what is used,
    NaN and 1e30 wherever nothing may be read."""
    lib = _capi.load_library()
    geo = resample_geometry(*pair)
    before, take, ends = [0, 37, 1000, 1000], [500, 0, 441, 300], [False, False, False, True]
    s = len(before)
    x = seeded_audio(s, 1500, seed=11).cuda()
    plan, states = [], []
    for i in range(s):
        _, st = resample_advance(ResampleState(), before[i], False, geo)
        states.append(st)
        plan.append(resample_advance(st, take[i], ends[i], geo)[0])
    sf, ff, fstride = l3ac_amd.stream_resampler(1, *pair).state_frames + 4, 500, 503
    of = max(p.count for p in plan)
    ostride = of + 5
    state0 = _garbage((s, sf))
    fresh0 = _garbage((s, fstride))
    for i in range(s):
        state0[i, :states[i].held] = x[i, before[i] - states[i].held:before[i]]
        fresh0[i, :take[i]] = x[i, before[i]:before[i] + take[i]]
    view = lambda t: t.view(torch.float32)
    (in_w, st_in), (out_w, st_out), (fresh_w, fresh), (y_w, y) = _guarded(s * sf, 37), _guarded(s * sf, 38), _guarded(s * fstride, 38), _guarded(s * ostride, 37)
    st_in.copy_(state0.reshape(-1).view(torch.int32))
    fresh.copy_(fresh0.reshape(-1).view(torch.int32))
    bank = l3ac_amd._resample_bank(x.device, *pair)
    order = [2, 0, 3, 1]  # descriptors in another order than the streams
    desc = (_capi.ResampleStreamDesc * s)(*[_capi.ResampleStreamDesc(i, plan[i].held, plan[i].take, plan[i].count, plan[i].keep, plan[i].q0) for i in order])
    _capi.check(lib.l3ac_resample_stream(view(st_in).data_ptr(), view(st_out).data_ptr(), s, sf, view(fresh).data_ptr(), ff, fstride, pair[0], pair[1],
                                         bank.data_ptr(), desc, s, view(y).data_ptr(), of, ostride, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    # inputs untouched, guards intact
    assert torch.equal(st_in.cpu(), state0.reshape(-1).view(torch.int32).cpu()) and torch.equal(fresh.cpu(), fresh0.reshape(-1).view(torch.int32).cpu())
    assert _guards_intact(in_w, s * sf, 37) and _guards_intact(out_w, s * sf, 38) and _guards_intact(fresh_w, s * fstride, 38) and _guards_intact(y_w, s * ostride, 37)
    # the next state: the last `keep` of held ++ new; what lies after it in a row is not written
    st, fr = state0.cpu().numpy().view(np.int32), fresh0.cpu().numpy().view(np.int32)
    want_state = np.full((s, sf), np.int32(SENTINEL), dtype=np.int32)
    for i, p in enumerate(plan):
        row = np.concatenate([st[i, :p.held], fr[i, :p.take]])
        want_state[i, :p.keep] = row[len(row) - p.keep:]
    assert np.array_equal(st_out.cpu().view(s, sf).numpy(), want_state)
    assert [p.keep for p in plan][1] == states[1].held > 0 and plan[3].keep == 0  # (the idle stream's state follows; the ended one keeps nothing)
    # the outputs: resample of the whole stream, the slice this push emits; zeros up to out_frames; nothing behind
    got = view(y).cpu().view(s, ostride)
    for i, p in enumerate(plan):
        n = before[i] + take[i]
        whole = l3ac_amd.resample(x[i:i + 1, :n].contiguous(), *pair)[0].cpu()
        assert torch.equal(got[i, :p.count], whole[states[i].emitted:states[i].emitted + p.count]), f"stream {i}"
        assert not got[i, p.count:of].any() and bool((got[i, of:].view(torch.int32) == SENTINEL).all())
    assert plan[0].count > 0 and plan[1].count == 0 and states[3].emitted + plan[3].count == l3ac_amd.resample_length(*pair, 1300)


# ---- 2. the session against resample -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
def test_any_split_is_resample_of_the_whole_stream(pair):
    audio, want = _streams(pair)
    rs = l3ac_amd.stream_resampler(len(LENGTHS), *pair)
    assert rs.state_frames >= resample_geometry(*pair).K - 1 and (pair != (48000, 8000) or resample_geometry(*pair).K == 121)
    for size, end_with_last in ((7, True), (441, False), (960, True), (None, True), (None, False)):
        packets = [_packets(n, size) if size else [n] for n in LENGTHS]
        got = _drive(rs, audio, packets, end_with_last=end_with_last)  # (the same session throughout: every slot is reused)
        for i, n in enumerate(LENGTHS):
            assert got[i].shape == want[i].shape and torch.equal(got[i], want[i]), f"packets of {size}: stream {i} ({n} samples)"
        assert rs.states == [ResampleState()] * len(LENGTHS)
    # before its end a stream has emitted exactly the outputs whose newest input has arrived
    geo = resample_geometry(*pair)
    y, n = rs.push(audio[:, :3000].contiguous())
    assert n.tolist() == [max(0, -(-(3000 * geo.up - geo.half_len) // geo.down))] * 4 and all(st.held <= geo.K - 1 for st in rs.states)
    assert 0 < int(n[2]) < want[2].shape[0] and torch.equal(y[2], want[2][:int(n[2])])  # (stream 2 IS 3000 samples: all but its tail)
    rs.reset()


def test_the_shortest_stream_in_packets_of_one():
    for pair in PAIRS:
        audio, want = _streams(pair)
        rs = l3ac_amd.stream_resampler(2, *pair)
        got = _drive(rs, audio[[0, 3]], [[1], [1] * 150], end_with_last=False)
        assert torch.equal(got[0], want[0])
        whole = l3ac_amd.resample(audio[3:4, :150].contiguous(), *pair)[0]
        assert torch.equal(got[1], whole)


def test_streams_are_independent_slots_reusable_and_reset_is_fresh():
    pair = (44100, 16000)
    audio, want = _streams(pair)
    n0 = LENGTHS[3]
    packets0 = _packets(n0, 441)
    lone = torch.zeros_like(audio)
    lone[0] = audio[3]
    # the neighbours idle all the way
    got = _drive(l3ac_amd.stream_resampler(4, *pair), lone, [packets0, [], [], []])
    assert torch.equal(got[0], want[3])
    # the neighbours push packets of their own sizes, start late, end early and restart in the same slots
    rs = l3ac_amd.stream_resampler(4, *pair)
    twice = torch.cat([audio, audio], dim=1)
    for i, n in enumerate(LENGTHS):
        twice[i, n:2 * n] = audio[i, :n]
    data = twice.clone()
    data[0, :n0] = audio[3, :n0]
    data[1, :2] = audio[0, 0]
    p7 = _packets(n0, 7)
    # stream 1: its one sample, ended, then the same sample again in the reused slot; streams 2, 3: their stream twice, back to back
    pk = [p7, [1, 1], _packets(LENGTHS[2], 441) + _packets(LENGTHS[2], 960), [LENGTHS[3], 100, LENGTHS[3] - 100]]
    ends = {1: (0, 1), 2: (len(_packets(LENGTHS[2], 441)) - 1, len(pk[2]) - 1), 3: (0, 2)}
    pos, parts = [0] * 4, [[] for _ in range(4)]
    for j in range(len(p7)):
        sizes = [pk[i][j] if j < len(pk[i]) else 0 for i in range(4)]
        flags = [j == len(p7) - 1] + [j in ends[i] for i in (1, 2, 3)]
        buf = _garbage((4, max(sizes)))
        for i in range(4):
            buf[i, :sizes[i]] = data[i, pos[i]:pos[i] + sizes[i]]
            pos[i] += sizes[i]
        y, n = rs.push(buf, lengths=sizes, end=flags)
        for i, k in enumerate(n.tolist()):
            parts[i].append(y[i, :k])
    assert torch.equal(torch.cat(parts[0]), want[3]), "busy neighbours"
    assert torch.equal(torch.cat(parts[1]), torch.cat([want[0], want[0]]))
    assert torch.equal(torch.cat(parts[2]), torch.cat([want[2], want[2]])) and torch.equal(torch.cat(parts[3]), torch.cat([want[3], want[3]]))
    # reset: a session in the middle of its streams, reset, emits what a fresh session emits
    rs.push(audio[:, :1000].contiguous())
    assert all(st.held > 0 for st in rs.states)
    rs.reset()
    assert rs.states == [ResampleState()] * 4
    got = _drive(rs, audio, [_packets(n, 960) for n in LENGTHS])
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    rs.push(audio[:, :1000].contiguous())
    rs.reset(streams=[1])
    assert [st.seen for st in rs.states] == [1000, 0, 1000, 1000]


def test_more_streams_than_one_launch_carries_descriptors_for():
    """130 streams: two launches per push (128 descriptors each at most); every stream has its own samples and its own length."""
    pair, s = (44100, 16000), 130
    x = seeded_audio(s, 700, seed=5).cuda()
    lengths = [700 - 3 * i for i in range(s)]
    rs = l3ac_amd.stream_resampler(s, *pair)
    parts = [[] for _ in range(s)]
    for a, b in ((0, 300), (300, 700)):
        sizes = [max(0, min(b, n) - a) for n in lengths]
        y, n = rs.push(x[:, a:b].contiguous(), lengths=sizes, end=b == 700)
        for i, k in enumerate(n.tolist()):
            assert not y[i, k:].any()
            parts[i].append(y[i, :k])
    for i, n in enumerate(lengths):
        assert torch.equal(torch.cat(parts[i]), l3ac_amd.resample(x[i:i + 1, :n].contiguous(), *pair)[0]), f"stream {i}"


def test_equal_rates_are_bit_copies():
    rs = l3ac_amd.stream_resampler(3, 16000, 16000)
    x = seeded_audio(3, 1001, seed=3).cuda()
    x[:, ::5] = -0.0
    x[1, 7] = float("inf")  # a copy moves bits: nothing is computed
    sent = []
    for j, (a, b) in enumerate(((0, 1), (1, 1), (1, 400), (400, 1001))):
        sizes = [b - a, (b - a) // 2, 0]
        buf = _garbage((3, b - a + 1))
        for i in range(3):
            buf[i, :sizes[i]] = x[i, a:a + sizes[i]]
        y, n = rs.push(buf, lengths=sizes, end=[j == 3, False, False])
        assert n.tolist() == sizes and y.shape == (3, b - a)
        for i in range(3):
            assert torch.equal(y[i, :sizes[i]].view(torch.int32), x[i, a:a + sizes[i]].view(torch.int32)) and not y[i, sizes[i]:].view(torch.int32).any()
    assert rs.states[0] == ResampleState() and rs.states[1].held == 0 and rs.delay == 0.0
    assert torch.equal(l3ac_amd.resample(x, 16000, 16000).view(torch.int32), x.view(torch.int32))


def test_errors_leave_the_session_as_it_was():
    pair = (48000, 16000)
    audio, want = _streams(pair)
    rs = l3ac_amd.stream_resampler(4, *pair)
    y0, n0 = rs.push(audio[:, :1000].contiguous(), lengths=[1, 1000, 1000, 1000])
    states = rs.states
    piece = audio[:, 1000:1100].contiguous()
    with pytest.raises(RuntimeError, match="is on cpu"):
        rs.push(piece.cpu())
    for bad in (audio[0, :100], audio[:3, :100], audio[:, :100, None]):
        with pytest.raises(ValueError):
            rs.push(bad)
    for bad in ([-1, 5, 5, 5], [101, 5, 5, 5], [5, 5, 5], [1.5, 5, 5, 5], "abcd"):
        with pytest.raises(ValueError):
            rs.push(piece, lengths=bad)
    with pytest.raises(ValueError):
        rs.push(piece, end=[True, False])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="captured"):
            rs.push(piece)
        doubled = piece * 2  # (something to capture)
    assert rs.states == states
    # ... and goes on with the right bits
    rest = _drive(rs, audio[:, 1000:], [[0], [1999], [2000], [3801]])
    for i in (1, 2, 3):
        assert torch.equal(torch.cat([y0[i, :int(n0[i])], rest[i]]), want[i]), f"stream {i}"
    assert torch.equal(torch.cat([y0[0, :int(n0[0])], rest[0]]), want[0])


# ---- 3. the chains: a live stream at another rate through the codec's sessions -------------------------------------------------------------
def test_chains_are_encode_long_and_decode_long_with_a_sample_rate():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.to(device="cuda").eval()
    hop, sr = codec.network.mc.hop_length, codec.config.sample_rate
    lengths = [int(2.2 * 48000), int(1.3 * 48000)]
    audio = (seeded_audio(2, max(lengths), seed=77) * 1.7).cuda()  # (white noise keeps a third of its power below 8 kHz)
    audio[1, lengths[1]:] = float("nan")
    kw = dict(process_window=16000, prefix_tokens=8)
    q, ind = codec.encode_long(audio, lengths=lengths, sample_rate=48000, **kw)
    tok = ind["lengths"].tolist()
    assert tok == [-(-l3ac_amd.resample_length(48000, sr, n) // hop) for n in lengths] and ind["indices"].unique().numel() > 8  # (not a degenerate stream that anything would equal)
    rs, enc = l3ac_amd.stream_resampler(2, 48000, sr), codec.stream_encoder(streams=2, **kw)
    got_q, got_i = [[], []], [[], []]
    packets = [_packets(n, 960) for n in lengths]
    for j in range(len(packets[0])):
        sizes = [p[j] if j < len(p) else 0 for p in packets]
        ends = [j == len(p) - 1 for p in packets]
        buf = _garbage((2, 960))
        for i in range(2):
            buf[i, :sizes[i]] = audio[i, j * 960:j * 960 + sizes[i]]
        y, n = rs.push(buf, lengths=sizes, end=ends)
        qf, out = enc.push(y, lengths=n, end=ends)
        for i, k in enumerate(out["lengths"].tolist()):
            got_q[i].append(qf[i, :k]), got_i[i].append(out["indices"][i, :k])
    for i, k in enumerate(tok):
        assert torch.equal(torch.cat(got_i[i]), ind["indices"][i, :k]) and torch.equal(torch.cat(got_q[i]), q[i, :k]), f"encoder chain: stream {i}"
    # decoding side: tokens in packets of 3, the audio out at 44.1 kHz
    want = codec.decode_long(indices=ind["indices"], lengths=tok, sample_rate=44100, **kw)
    dec, rs_out = codec.stream_decoder(streams=2, **kw), l3ac_amd.stream_resampler(2, sr, 44100)
    parts = [[], []]
    packets = [_packets(k, 3) for k in tok]
    pos = [0, 0]
    for j in range(len(packets[0])):
        sizes = [p[j] if j < len(p) else 0 for p in packets]
        ends = [j == len(p) - 1 for p in packets]
        buf = torch.full((2, 3), 10 ** 7, dtype=torch.int32, device="cuda")
        for i in range(2):
            buf[i, :sizes[i]] = ind["indices"][i, pos[i]:pos[i] + sizes[i]]
            pos[i] += sizes[i]
        wave, n_tok = dec.push(indices=buf, lengths=sizes, end=ends)
        out, n_out = rs_out.push(wave, lengths=n_tok * hop, end=ends)
        for i, k in enumerate(n_out.tolist()):
            parts[i].append(out[i, :k])
    for i, k in enumerate(tok):
        n = l3ac_amd.resample_length(sr, 44100, k * hop)
        got = torch.cat(parts[i])
        assert got.shape[0] == n and torch.equal(got, want[i, :n]), f"decoder chain: stream {i}"
