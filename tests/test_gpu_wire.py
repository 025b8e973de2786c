"""The streaming token wire format on the GPU: the two kernels through their C entries (guards, inputs untouched,
outputs and next state against a restatement of the format on Python integers), StreamPacker / StreamUnpacker against pack_indices /
unpack_indices of each whole stream however it is split over pushes and whatever the other streams do, the ragged forms of the two
functions, the chain encoder -> packer -> unpacker -> decoder against encode_long / decode_long, and compress / decompress.
Every comparison is exact."""
import random
import struct

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.wire import PackState, UnpackState, packed_bytes
from tests.helpers import seeded_audio

pytestmark = pytest.mark.gpu

COUNTS = [1, 8, 33, 600]  # tokens per stream: total bits = 17, 8, 17, 24 mod 32 at 17 bits; 600 tokens cross a 256-thread block both ways
_CACHE = {}


def _mask(bits):
    return (1 << bits) - 1


def _random_tokens(shape, seed):
    """int32 over the whole 32-bit range (garbage above `bits` wherever bits < 32), every fifth token all ones (-1)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
    t.view(-1)[::5] = -1
    return t


def _bytes_of(tokens, bits, held_value=0, held=0):
    """The format on Python integers: held bits ++ tokens as one big integer (its value, its length in bits)."""
    value = held_value & _mask(held)
    for k, t in enumerate(tokens):
        value |= (int(t) & _mask(bits)) << (held + k * bits)
    return value, held + len(tokens) * bits


def _numpy_pack(idx, bits):
    """pack_indices' rectangle restated: every row zero-padded to whole 32-bit words."""
    b, n = idx.shape
    row_bytes = 4 * (-(-n * bits // 32))
    out = np.zeros((b, row_bytes), dtype=np.uint8)
    for i in range(b):
        value, _ = _bytes_of(idx[i].tolist(), bits)
        out[i] = np.frombuffer(value.to_bytes(row_bytes, "little"), dtype=np.uint8)
    return out


# ---- 1. the kernels through the C entries ---------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF  # a NaN as fp32
SENTINEL_BYTES = list(struct.pack("<I", SENTINEL))


def _guarded(n_elements, guard):
    whole = torch.full((n_elements + 2 * guard,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole[guard:guard + n_elements]


def _guards_intact(whole, n_elements, guard):
    return bool((whole[:guard] == SENTINEL).all()) and bool((whole[guard + n_elements:] == SENTINEL).all())


def _sentinel_bytes(n, offset=0):
    return np.array([SENTINEL_BYTES[(offset + k) % 4] for k in range(n)], dtype=np.uint8)


@pytest.mark.parametrize("bits", [8, 17, 18, 31, 32])
def test_pack_kernel_against_the_restatement(bits):
    """Four streams: one fresh, one idle with bits pending, one ending with 7 bits pending and 1100 tokens (more than one block of dwords),
    one without a descriptor.  Rows of an odd stride, all-ones tokens wherever nothing may be read, garbage above the held bits."""
    lib = _capi.load_library()
    s, ft, fstride = 4, 1100, 1103
    #       slot held take ended
    rows = [(0, 0, 37, False), (1, 5, 0, False), (2, 7, 1100, True)]
    tokens = _random_tokens((s, ft), seed=bits)
    fresh0 = torch.full((s, fstride), -1, dtype=torch.int32)
    for slot, _, take, _ in rows:
        fresh0[slot, :take] = tokens[slot, :take]
    state0 = _random_tokens((s,), seed=100 + bits)
    state0[2] = -1
    plan, want_out, want_state = [], {}, {}
    for slot, held, take, ended in rows:
        value, total = _bytes_of(fresh0[slot, :take].tolist(), bits, int(state0[slot]) & 0xFFFFFFFF, held)
        count, keep = (-(-total // 8), 0) if ended else divmod(total, 8)
        plan.append((slot, held, take, count, keep))
        want_out[slot] = (value & _mask(8 * count)).to_bytes(count, "little")
        want_state[slot] = (value >> (8 * count)) & _mask(keep)
    out_bytes = max(p[3] for p in plan) + 3
    out_bytes += out_bytes % 4 == 0
    ostride = -(-out_bytes // 4) * 4 + 4
    assert out_bytes % 4 and out_bytes > 4 * 256  # (a last dword stored byte by byte; more than one workgroup per stream)
    (in_w, st_in), (out_w, st_out), (fresh_w, fresh), (y_w, y) = _guarded(s, 37), _guarded(s, 38), _guarded(s * fstride, 38), _guarded(s * ostride // 4, 37)
    st_in.copy_(state0)
    fresh.copy_(fresh0.reshape(-1))
    order = [2, 0, 1]  # descriptors in another order than the streams
    desc = (_capi.PackStreamDesc * len(order))(*[_capi.PackStreamDesc(*plan[k]) for k in order])
    _capi.check(lib.l3ac_pack_stream(st_in.data_ptr(), st_out.data_ptr(), s, fresh.data_ptr(), ft, fstride, bits, desc, len(order), y.data_ptr(),
                                     out_bytes, ostride, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(st_in.cpu(), state0) and torch.equal(fresh.cpu(), fresh0.reshape(-1))  # inputs untouched
    assert _guards_intact(in_w, s, 37) and _guards_intact(out_w, s, 38) and _guards_intact(fresh_w, s * fstride, 38) and _guards_intact(y_w, s * ostride // 4, 37)
    got = y.cpu().view(torch.uint8).view(s, ostride).numpy()
    got_state = st_out.cpu().tolist()
    for slot, held, take, count, keep in plan:
        assert got[slot, :count].tobytes() == want_out[slot], f"stream {slot}"
        assert not got[slot, count:out_bytes].any(), f"stream {slot}: zeros up to out_bytes"
        assert np.array_equal(got[slot, out_bytes:], _sentinel_bytes(ostride - out_bytes, out_bytes)), f"stream {slot}: nothing behind out_bytes"
        assert got_state[slot] & 0xFFFFFFFF == want_state[slot], f"stream {slot}: next state"
    assert np.array_equal(got[3], _sentinel_bytes(ostride)) and got_state[3] == SENTINEL  # the row without a descriptor
    assert want_state[1] == int(state0[1]) & 31 and want_state[2] == 0 and plan[0][4] == (37 * bits) % 8  # idle: the state follows; ended: none


@pytest.mark.parametrize("bits", [8, 17, 18, 31, 32])
def test_unpack_kernel_against_the_restatement(bits):
    """The mirror: byte rows of an odd stride, so the four rows start at the four byte alignments, the whole buffer moved through the four
    alignments as well; one stream with 1275 bytes (more than one block of tokens), one idle with bits - 1 bits pending, one ending, one
    without a descriptor; 0xFF wherever nothing may be read."""
    lib = _capi.load_library()
    s, fb, fstride = 4, 1275, 1301
    #       slot held      take  ended
    rows = [(0, 0, 1275, False), (1, bits - 1, 0, False), (2, 5, 101, True)]
    g = torch.Generator().manual_seed(bits)
    data = torch.randint(0, 256, (s, fb), generator=g, dtype=torch.int64).to(torch.uint8)
    data[:, ::7] = 255
    fresh0 = torch.full((s, fstride), 255, dtype=torch.uint8)
    for slot, _, take, _ in rows:
        fresh0[slot, :take] = data[slot, :take]
    state0 = _random_tokens((s,), seed=200 + bits)
    state0[1] = -1
    plan, want_out, want_state = [], {}, {}
    for slot, held, take, ended in rows:
        total = held + 8 * take
        value = (int(state0[slot]) & _mask(held)) | (int.from_bytes(fresh0[slot, :take].numpy().tobytes(), "little") << held)
        count, keep = total // bits, 0 if ended else total % bits
        plan.append((slot, held, take, count, keep))
        want_out[slot] = [(value >> (k * bits)) & _mask(bits) for k in range(count)]
        want_state[slot] = (value >> (count * bits)) & _mask(keep)
    out_tokens = max(p[3] for p in plan) + 3
    ostride = out_tokens + 5
    assert max(p[3] for p in plan) > 256
    for align in range(4):
        (in_w, st_in), (out_w, st_out), (y_w, y) = _guarded(s, 37), _guarded(s, 38), _guarded(s * ostride, 37)
        fresh_w = torch.full((s * fstride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        fresh = fresh_w[16 + align:16 + align + s * fstride]
        assert fresh.data_ptr() % 4 == align
        fresh.copy_(fresh0.reshape(-1))
        before = fresh_w.cpu()
        st_in.copy_(state0)
        desc = (_capi.UnpackStreamDesc * 3)(*[_capi.UnpackStreamDesc(*plan[k]) for k in (1, 2, 0)])
        _capi.check(lib.l3ac_unpack_stream(st_in.data_ptr(), st_out.data_ptr(), s, fresh.data_ptr(), fb, fstride, bits, desc, 3, y.data_ptr(),
                                           out_tokens, ostride, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(st_in.cpu(), state0) and torch.equal(fresh_w.cpu(), before)
        assert _guards_intact(in_w, s, 37) and _guards_intact(out_w, s, 38) and _guards_intact(y_w, s * ostride, 37)
        got = y.cpu().view(s, ostride)
        got_state = st_out.cpu().tolist()
        for slot, held, take, count, keep in plan:
            assert [v & 0xFFFFFFFF for v in got[slot, :count].tolist()] == want_out[slot], f"alignment {align}: stream {slot}"
            assert not got[slot, count:out_tokens].any() and bool((got[slot, out_tokens:] == SENTINEL).all())
            assert got_state[slot] & 0xFFFFFFFF == want_state[slot], f"alignment {align}: stream {slot}: next state"
        assert bool((got[3] == SENTINEL).all()) and got_state[3] == SENTINEL
    assert want_state[1] == _mask(bits - 1) and want_state[2] == 0


# ---- 2. the sessions against the offline functions ----------------------------------------------------------------------------------------
def _streams(bits):
    """The test streams with pack_indices / unpack_indices of each alone (computed once per width and shared, never changed): per stream its
    tokens as given (garbage above `bits`), its bytes and its tokens as unpacked."""
    if bits not in _CACHE:
        tokens = _random_tokens((len(COUNTS), max(COUNTS)), seed=7 * bits).cuda()
        wire, back = [], []
        for i, n in enumerate(COUNTS):
            row = l3ac_amd.pack_indices(tokens[i:i + 1, :n].contiguous(), bits)
            assert row.dtype == torch.uint8 and row.shape == (1, 4 * (-(-n * bits // 32))) and not row[0, packed_bytes(n, bits):].any()
            wire.append(row[0, :packed_bytes(n, bits)].clone())
            back.append(l3ac_amd.unpack_indices(row, n, bits)[0])
            want = tokens[i, :n] if bits == 32 else tokens[i, :n] & _mask(bits)
            assert torch.equal(back[-1], want)
        _CACHE[bits] = (tokens, wire, back)
    return _CACHE[bits]


def _packets(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def _random_packets(n, rng):
    cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(1, 6)))
    parts = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    parts.insert(rng.randint(0, len(parts)), 0)
    return parts


def _drive(session, data, packets, garbage, first_call=0, end_with_last=True):
    """Feed stream i its packets[i] of data[i], one per call from call first_call[i] on, with garbage after each packet's end; a stream ends
    with its last packet (or, end_with_last=False, with an empty push one call later) and idles before and afterwards.  Returns per stream
    the concatenation of what it emitted, checking shapes, counts and the zeros behind every stream's outputs on the way."""
    s = session.streams
    first = [first_call] * s if isinstance(first_call, int) else first_call
    packets = [list(p) + ([] if end_with_last or not p else [0]) for p in packets]
    out_dtype = torch.uint8 if isinstance(session, l3ac_amd.StreamPacker) else torch.int32
    pos = [0] * s
    parts = [[] for _ in range(s)]
    for j in range(max(f + len(p) for f, p in zip(first, packets))):
        sizes = [p[j - f] if 0 <= j - f < len(p) else 0 for f, p in zip(first, packets)]
        ends = [j - f == len(p) - 1 for f, p in zip(first, packets)]
        buf = torch.full((s, max(sizes) + (j % 2)), garbage, dtype=data[0].dtype, device="cuda")
        for i in range(s):
            buf[i, :sizes[i]] = data[i][pos[i]:pos[i] + sizes[i]]
            pos[i] += sizes[i]
        y, n = session.push(buf, lengths=sizes, end=ends)
        assert n.dtype == torch.int32 and not n.is_cuda and y.dtype == out_dtype and y.shape == (s, int(n.max()))
        host = y.cpu()
        for i, k in enumerate(n.tolist()):
            assert not host[i, k:].any()
            parts[i].append(host[i, :k])
    return [torch.cat(p) for p in parts]


def _deliveries(lengths, seed):
    rng = random.Random(seed)
    s = len(lengths)
    yield "all at once", [[n] for n in lengths], 0, True
    yield "all at once, ended one call later", [[n] for n in lengths], 0, False
    yield "packets of 7", [_packets(n, 7) for n in lengths], 0, True
    yield "random packets with empty pushes", [_random_packets(n, rng) for n in lengths], 0, rng.random() < 0.5
    yield "staggered starts", [_random_packets(n, rng) for n in lengths], [3, 0, 2, 5][:s], False


@pytest.mark.parametrize("bits", [17, 18, 32])
def test_any_split_of_the_tokens_is_pack_indices_of_the_whole_stream(bits):
    tokens, wire, _ = _streams(bits)
    packer = l3ac_amd.stream_packer(len(COUNTS), bits)
    data = [tokens[i, :n] for i, n in enumerate(COUNTS)]
    for what, packets, first, end_with_last in _deliveries(COUNTS, seed=bits):
        got = _drive(packer, data, packets, garbage=SENTINEL, first_call=first, end_with_last=end_with_last)  # (one session: every slot is reused)
        for i, n in enumerate(COUNTS):
            assert got[i].shape == wire[i].shape and torch.equal(got[i], wire[i].cpu()), f"{what}: stream {i} ({n} tokens)"
        assert packer.states == [PackState()] * len(COUNTS)
    # before its end a stream has emitted its whole bytes
    y, n = packer.push(tokens[:, :33].contiguous())
    assert n.tolist() == [33 * bits // 8] * 4 and [st.held_bits for st in packer.states] == [(33 * bits) % 8] * 4
    assert torch.equal(y[3].cpu(), wire[3][:33 * bits // 8].cpu())


@pytest.mark.parametrize("bits", [17, 18, 32])
def test_tokens_one_by_one(bits):
    tokens, wire, _ = _streams(bits)
    packer = l3ac_amd.stream_packer(len(COUNTS), bits)
    got = _drive(packer, [tokens[i, :n] for i, n in enumerate(COUNTS)], [[1] * n for n in COUNTS], garbage=-1)
    assert all(torch.equal(g, w.cpu()) for g, w in zip(got, wire))


@pytest.mark.parametrize("bits", [17, 18, 32])
def test_any_split_of_the_bytes_is_unpack_indices_of_the_whole_stream(bits):
    _, wire, back = _streams(bits)
    unpacker = l3ac_amd.stream_unpacker(len(COUNTS), bits)
    sizes = [w.shape[0] for w in wire]
    ways = [(f"packets of {k}", [_packets(n, k) for n in sizes], 0, k != 3) for k in (1, 3, 5)]
    for what, packets, first, end_with_last in ways + list(_deliveries(sizes, seed=bits)):
        got = _drive(unpacker, wire, packets, garbage=0xFF, first_call=first, end_with_last=end_with_last)
        for i, n in enumerate(COUNTS):
            assert got[i].shape == back[i].shape and torch.equal(got[i], back[i].cpu()), f"{what}: stream {i} ({n} tokens)"
        assert unpacker.states == [UnpackState()] * len(COUNTS)
    # pack_indices' word-padded row instead of the stream's own bytes: the padding can hold (zero) tokens
    row = l3ac_amd.pack_indices(_streams(bits)[0][2:3, :33].contiguous(), bits)
    idx, n = l3ac_amd.stream_unpacker(1, bits).push(row, end=True)
    assert int(n[0]) == 8 * row.shape[1] // bits >= 33 and torch.equal(idx[0, :33], back[2]) and not idx[0, 33:].any()


def test_streams_are_independent_and_reset_is_fresh():
    bits = 17
    tokens, wire, back = _streams(bits)
    packer, unpacker = l3ac_amd.stream_packer(4, bits), l3ac_amd.stream_unpacker(4, bits)
    # every stream half way, then stream 3 is reset and starts again while the others go on
    half = [n // 2 for n in COUNTS]
    first = torch.full((4, max(half)), -1, dtype=torch.int32, device="cuda")
    for i, h in enumerate(half):
        first[i, :h] = tokens[i, :h]
    y0, n0 = packer.push(first, lengths=half)
    assert packer.states[3].held_bits == (300 * bits) % 8 != 0
    packer.reset(streams=3)
    assert packer.states[3] == PackState() and packer.states[2] == PackState((16 * bits) % 8, 16, 16 * bits // 8)
    rest = _drive(packer, [tokens[i, h:n] for i, (h, n) in enumerate(zip(half, COUNTS))][:3] + [tokens[3, :600]],
                  [[n - h] for h, n in zip(half, COUNTS)][:3] + [_packets(600, 7)], garbage=-1)
    for i in range(3):
        assert torch.equal(torch.cat([y0[i, :int(n0[i])].cpu(), rest[i]]), wire[i].cpu()), f"stream {i}"
    assert torch.equal(rest[3], wire[3].cpu())
    # the same on the receiving side, the reset stream restarting in bytes one by one
    halfb = [w.shape[0] // 2 for w in wire]
    firstb = torch.full((4, max(halfb)), 0xFF, dtype=torch.uint8, device="cuda")
    for i, h in enumerate(halfb):
        firstb[i, :h] = wire[i][:h]
    i0, m0 = unpacker.push(firstb, lengths=halfb)
    assert unpacker.states[3].held_bits == (8 * halfb[3]) % bits != 0
    unpacker.reset(streams=[3])
    rest = _drive(unpacker, [w[h:] for w, h in zip(wire, halfb)][:3] + [wire[3]], [[w.shape[0] - h] for w, h in zip(wire, halfb)][:3] + [[1] * wire[3].shape[0]],
                  garbage=0xFF)
    for i in range(3):
        assert torch.equal(torch.cat([i0[i, :int(m0[i])].cpu(), rest[i]]), back[i].cpu()), f"stream {i}"
    assert torch.equal(rest[3], back[3].cpu())


def test_errors_leave_the_sessions_as_they_were():
    bits = 18
    tokens, wire, back = _streams(bits)
    packer = l3ac_amd.stream_packer(4, bits)
    y0, n0 = packer.push(tokens[:, :5].contiguous(), lengths=[1, 5, 5, 5])
    states = packer.states
    piece = tokens[:, 5:8].contiguous()
    with pytest.raises(RuntimeError, match="is on cpu"):
        packer.push(piece.cpu())
    for bad in (tokens[0, :3], tokens[:3, :3], tokens[:, :3, None], piece.to(torch.float32)):
        with pytest.raises(ValueError):
            packer.push(bad)
    for bad in ([-1, 3, 3, 3], [4, 3, 3, 3], [3, 3, 3], [1.5, 3, 3, 3]):
        with pytest.raises(ValueError):
            packer.push(piece, lengths=bad)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="captured"):
            packer.push(piece)
        doubled = piece * 2  # (something to capture)
    assert packer.states == states
    rest = _drive(packer, [tokens[0, 1:1], tokens[1, 5:8], tokens[2, 5:33], tokens[3, 5:600]], [[0], [3], [28], [595]], garbage=-1)
    for i in range(4):
        assert torch.equal(torch.cat([y0[i, :int(n0[i])].cpu(), rest[i]]), wire[i].cpu()), f"stream {i}"


# ---- 3. the ragged forms of pack_indices / unpack_indices ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [5, 17, 18, 32])
def test_ragged_pack_and_unpack_are_the_rectangular_calls_row_by_row(bits):
    t_tok = 70
    lengths = [0, 1, 33, t_tok]
    clean = _random_tokens((4, t_tok), seed=bits + 1).cuda()
    idx = clean.clone()
    for i, n in enumerate(lengths):
        idx[i, n:] = SENTINEL  # NaN-pattern garbage behind each row's own tokens
    packed, nbytes = l3ac_amd.pack_indices(idx, bits, lengths=lengths)
    row_bytes = 4 * (-(-t_tok * bits // 32))
    assert packed.dtype == torch.uint8 and packed.shape == (4, row_bytes) and nbytes.dtype == torch.int32 and not nbytes.is_cuda
    assert nbytes.tolist() == [packed_bytes(n, bits) for n in lengths]
    for i, n in enumerate(lengths):
        if n:
            alone = l3ac_amd.pack_indices(clean[i:i + 1, :n].contiguous(), bits)[0]
            assert torch.equal(packed[i, :alone.shape[0]], alone), f"row {i}"
        assert not packed[i, int(nbytes[i]):].any(), f"row {i}: zeros after its own bytes"
    # the way back: garbage behind each row's own bytes
    dirty = packed.clone()
    for i, k in enumerate(nbytes.tolist()):
        dirty[i, k:] = torch.tensor((SENTINEL_BYTES * row_bytes)[k:row_bytes], dtype=torch.uint8)
    got = l3ac_amd.unpack_indices(dirty, t_tok, bits, lengths=lengths)
    assert got.dtype == torch.int32 and got.shape == (4, t_tok)
    for i, n in enumerate(lengths):
        if n:
            alone = l3ac_amd.unpack_indices(packed[i:i + 1], n, bits)[0]
            assert torch.equal(got[i, :n], alone) and torch.equal(alone, clean[i, :n] if bits == 32 else clean[i, :n] & _mask(bits)), f"row {i}"
        assert not got[i, n:].any(), f"row {i}: zeros after its own tokens"
    for bad in ([-1, 1, 1, 1], [71, 1, 1, 1], [1, 1, 1], [1.5, 1, 1, 1]):
        with pytest.raises(ValueError):
            l3ac_amd.pack_indices(idx, bits, lengths=bad)
        with pytest.raises(ValueError):
            l3ac_amd.unpack_indices(packed, t_tok, bits, lengths=bad)


@pytest.mark.parametrize("bits", [1, 8, 17, 18, 31, 32])
def test_calls_without_lengths_are_unchanged(bits):
    idx = _random_tokens((3, 601), seed=bits + 50)
    want = _numpy_pack(idx, bits)
    packed = l3ac_amd.pack_indices(idx.cuda(), bits)
    assert isinstance(packed, torch.Tensor) and packed.dtype == torch.uint8 and np.array_equal(packed.cpu().numpy(), want)
    back = l3ac_amd.unpack_indices(packed, 601, bits)
    assert back.dtype == torch.int32 and torch.equal(back.cpu(), idx if bits == 32 else idx & _mask(bits))
    # ... and the ragged form with every row full agrees with them
    full, nbytes = l3ac_amd.pack_indices(idx.cuda(), bits, lengths=[601] * 3)
    assert np.array_equal(full.cpu().numpy(), want) and nbytes.tolist() == [packed_bytes(601, bits)] * 3
    assert torch.equal(l3ac_amd.unpack_indices(packed, 601, bits, lengths=[601] * 3), back)


# ---- 4. the chain and the frames, with the tiny model of the other stream tests -----------------------------------------------------------
def _codec():
    if "codec" not in _CACHE:
        codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
        codec.network.to(device="cuda").eval()
        _CACHE["codec"] = codec
    return _CACHE["codec"]


def test_chain_encoder_packer_unpacker_decoder():
    codec = _codec()
    mc, sr = codec.network.mc, codec.config.sample_rate
    hop, bits = mc.hop_length, l3ac_amd.bits_per_token(mc)
    lengths = [int(1.6 * sr) + 7, int(0.9 * sr)]
    audio = (seeded_audio(2, max(lengths), seed=41) * 1.7).cuda()
    audio[1, lengths[1]:] = float("nan")
    kw = dict(process_window=8000, prefix_tokens=8)
    _, ind = codec.encode_long(audio, lengths=lengths, **kw)
    tok = ind["lengths"].tolist()
    want = codec.decode_long(indices=ind["indices"], lengths=tok, **kw)
    assert tok == [-(-n // hop) for n in lengths] and ind["indices"].unique().numel() > 8
    enc, dec = codec.stream_encoder(streams=2, **kw), codec.stream_decoder(streams=2, **kw)
    packer, unpacker = l3ac_amd.stream_packer(2, bits), l3ac_amd.stream_unpacker(2, bits)
    step = int(0.3 * sr)
    packets = [_packets(n, step) for n in lengths]
    got_i, got_w, sent = [[], []], [[], []], [0, 0]
    for j in range(len(packets[0])):
        sizes = [p[j] if j < len(p) else 0 for p in packets]
        ends = [j == len(p) - 1 for p in packets]
        buf = torch.full((2, step), float("nan"), dtype=torch.float32, device="cuda")
        for i in range(2):
            buf[i, :sizes[i]] = audio[i, j * step:j * step + sizes[i]]
        _, out = enc.push(buf, lengths=sizes, end=ends)
        wire, n_bytes = packer.push(out["indices"], lengths=out["lengths"], end=ends)
        idx, n_tok = unpacker.push(wire, lengths=n_bytes, end=ends)
        wave, n_out = dec.push(indices=idx, lengths=n_tok, end=ends)
        for i in range(2):
            sent[i] += int(n_bytes[i])
            got_i[i].append(idx[i, :int(n_tok[i])]), got_w[i].append(wave[i, :int(n_out[i]) * hop])
    for i, k in enumerate(tok):
        assert sent[i] == packed_bytes(k, bits), f"stream {i}: bytes on the wire"
        assert torch.equal(torch.cat(got_i[i]), ind["indices"][i, :k]), f"stream {i}: tokens"
        got = torch.cat(got_w[i])
        assert got.shape[0] == k * hop and torch.equal(got, want[i, :k * hop]), f"stream {i}: audio"


def test_compress_and_decompress():
    codec = _codec()
    mc, sr = codec.network.mc, codec.config.sample_rate
    hop, bits = mc.hop_length, l3ac_amd.bits_per_token(mc)
    kw = dict(process_window=8000, prefix_tokens=8)
    lengths = [int(1.1 * sr) + 3, int(0.6 * sr)]
    audio = (seeded_audio(2, max(lengths), seed=43) * 1.7).cuda()
    audio[1, lengths[1]:] = float("nan")
    for rate in (None, 48000):
        x, n_in = (audio, lengths) if rate is None else (l3ac_amd.resample(audio[:1, :lengths[0]].contiguous(), sr, rate), None)
        _, ind = codec.encode_long(x, lengths=n_in, sample_rate=rate, **kw)
        tok = ind["lengths"].tolist()
        want = codec.decode_long(indices=ind["indices"], lengths=tok, sample_rate=rate, **kw)
        frames = codec.compress(x, lengths=n_in, sample_rate=rate, **kw)
        samples_in = n_in if n_in is not None else [x.shape[1]]
        samples = samples_in if rate is None else [l3ac_amd.resample_length(rate, sr, n) for n in samples_in]
        assert isinstance(frames, list) and len(frames) == len(tok) and all(isinstance(f, bytes) for f in frames)
        packed, _ = l3ac_amd.pack_indices(ind["indices"], bits, lengths=tok)
        for i, f in enumerate(frames):
            assert len(f) == 24 + packed_bytes(tok[i], bits)
            assert struct.unpack("<4sBBHIIII", f[:24]) == (b"L3AC", 1, bits, hop, mc.codebook_size, sr, tok[i], samples[i])
            assert f[24:] == packed[i, :packed_bytes(tok[i], bits)].cpu().numpy().tobytes()
        got, n_out = codec.decompress(frames, sample_rate=rate, **kw)
        out_len = samples if rate is None else [l3ac_amd.resample_length(sr, rate, n) for n in samples]
        assert n_out.dtype == torch.int32 and not n_out.is_cuda and n_out.tolist() == out_len and got.shape == (len(tok), max(out_len))
        for i, n in enumerate(out_len):
            assert torch.equal(got[i, :n], want[i, :n]) and not got[i, n:].any(), f"rate {rate}: recording {i}"
    # a frame of another model is refused before any device work
    other = l3ac_amd.L3ACConfig(config_file=l3ac_amd.config.resolve_config_file("3kbps")).network_config
    theirs = l3ac_amd.frame_header(other, sr, 2, other.hop_length + 1) + bytes(packed_bytes(2, l3ac_amd.bits_per_token(other)))
    with pytest.raises(ValueError, match="bits"):
        codec.decompress([frames[0], theirs])
