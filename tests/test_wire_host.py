"""The streaming token wire format, host side (no GPU; needs the built library): the push geometry of l3ac_amd/wire.py against a bit-level
restatement of the format push by push, its independence of a stream's age, the C surface of the new entries, the argument checks that
need no device and the frame header.  Every comparison is exact."""
import ctypes
import random
import re
import struct
from pathlib import Path

import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi, wire
from l3ac_amd.wire import PackPush, PackState, UnpackPush, UnpackState, pack_advance, packed_bytes, unpack_advance

REPO = Path(__file__).resolve().parent.parent
BITS = [8, 9, 17, 18, 31, 32]
COUNTS = [0, 1, 8, 32, 33, 600]


# ---- the format, restated: a recording's tokens as one big integer, bytes taken from it -------------------------------------------------
def _tokens(n, bits, seed):
    rng = random.Random(seed)
    return [rng.getrandbits(bits) if k % 5 else (1 << bits) - 1 for k in range(n)]  # (every fifth token all ones)


def _stream_int(tokens, bits):
    return sum((t & ((1 << bits) - 1)) << (k * bits) for k, t in enumerate(tokens))


def _stream_bytes(tokens, bits):
    n_bytes = -(-len(tokens) * bits // 8)
    return _stream_int(tokens, bits).to_bytes(n_bytes, "little")


def _deliveries(n, rng):
    """Ways to deliver n elements: all at once, one by one, random cuts with empty pushes in between; each with `end` on the last data push
    and on an empty push after it."""
    ways = [[n], [1] * n]
    for _ in range(3):
        cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(1, 6)))
        parts = [b - a for a, b in zip([0] + cuts, cuts + [n])]
        parts.insert(rng.randint(0, len(parts)), 0)
        ways.append(parts)
    return [(parts, end_on_last) for parts in ways for end_on_last in (True, False)]


def _pushes(parts, end_on_last):
    return [(m, end_on_last and i == len(parts) - 1) for i, m in enumerate(parts)] + ([] if end_on_last else [(0, True)])


def _run_pack(tokens, bits, parts, end_on_last):
    """Push `parts` through pack_advance, doing on Python ints what the descriptor tells the device to do; returns the bytes emitted and the
    held values met."""
    state, pending, pos = PackState(), 0, 0
    out, helds = b"", []
    for m, end in _pushes(parts, end_on_last):
        push, after = pack_advance(state, m, end, bits)
        assert isinstance(push, PackPush) and push.held == state.held_bits and push.take == m
        assert 0 <= push.held <= 7 and 0 <= push.keep <= 7 and push.count >= 0
        total = push.held + m * bits
        assert (push.count, push.keep) == ((-(-total // 8), 0) if end else divmod(total, 8))
        # the descriptor does not grow with the stream's age
        old = PackState(state.held_bits, state.tokens_seen + 2 ** 40, state.bytes_emitted + 2 ** 41)
        push_old, after_old = pack_advance(old, m, end, bits)
        assert push_old == push and all(0 <= v < 2 ** 31 for v in push_old)
        assert after_old == (PackState() if end else PackState(after.held_bits, after.tokens_seen + 2 ** 40, after.bytes_emitted + 2 ** 41))
        # the device's view: held bits ++ take tokens; the first count bytes out, the last keep bits kept
        string = pending | (_stream_int(tokens[pos:pos + m], bits) << push.held)
        out += (string & ((1 << (8 * push.count)) - 1)).to_bytes(push.count, "little")
        pending = (string >> (8 * push.count)) & ((1 << push.keep) - 1)
        assert end or string >> (8 * push.count) == pending  # (nothing is lost while the stream goes on)
        pos += m
        helds.append(push.held)
        if end:
            assert after == PackState()
            pending = 0
        else:
            assert after == PackState(push.keep, pos, len(out))
            assert len(out) == pos * bits // 8
        state = after
    assert pos == len(tokens)
    return out, helds


def _run_unpack(data, bits, parts, end_on_last):
    state, pending, pos = UnpackState(), 0, 0
    out, helds = [], []
    for m, end in _pushes(parts, end_on_last):
        push, after = unpack_advance(state, m, end, bits)
        assert isinstance(push, UnpackPush) and push.held == state.held_bits and push.take == m
        assert 0 <= push.held < bits and 0 <= push.keep < bits
        total = push.held + 8 * m
        assert push.count == total // bits and push.keep == (0 if end else total % bits)
        old = UnpackState(state.held_bits, state.bytes_seen + 2 ** 40, state.tokens_emitted + 2 ** 41)
        push_old, after_old = unpack_advance(old, m, end, bits)
        assert push_old == push and all(0 <= v < 2 ** 31 for v in push_old)
        assert after_old == (UnpackState() if end else UnpackState(after.held_bits, after.bytes_seen + 2 ** 40, after.tokens_emitted + 2 ** 41))
        string = pending | (int.from_bytes(data[pos:pos + m], "little") << push.held)
        out += [(string >> (k * bits)) & ((1 << bits) - 1) for k in range(push.count)]
        pending = (string >> (push.count * bits)) & ((1 << push.keep) - 1)
        pos += m
        helds.append(push.held)
        if end:
            assert after == UnpackState()
            pending = 0
        else:
            assert after == UnpackState(push.keep, pos, len(out))
            assert len(out) == 8 * pos // bits
        state = after
    assert pos == len(data)
    return out, helds


@pytest.mark.parametrize("bits", BITS)
def test_any_delivery_gives_the_bytes_and_tokens_of_the_whole_stream(bits):
    rng = random.Random(bits)
    lib = _capi.load_library()
    for n in COUNTS:
        tokens = _tokens(n, bits, seed=100 * bits + n)
        want = _stream_bytes(tokens, bits)
        assert len(want) == packed_bytes(n, bits) == lib.l3ac_packed_bytes(n, bits)
        for parts, end_on_last in _deliveries(n, rng):
            got, _ = _run_pack(tokens, bits, parts, end_on_last)
            assert got == want, (n, parts, end_on_last)
        for parts, end_on_last in _deliveries(len(want), rng):
            got, _ = _run_unpack(want, bits, parts, end_on_last)
            assert len(got) == 8 * len(want) // bits == n and got == tokens, (n, parts, end_on_last)
        # the word-padded row of the rectangular call holds the stream's bytes, then zeros: more bytes can mean more (zero) tokens
        padded = want + bytes(-len(want) % 4)
        got, _ = _run_unpack(padded, bits, [len(padded)], True)
        assert len(got) == 8 * len(padded) // bits and got[:n] == tokens and not any(got[n:])


def test_one_element_pushes_visit_every_phase():
    """gcd(8, 17) = gcd(8, 31) = 1: tokens one by one meet every held value 0..7, bytes one by one at 17 bits every held value 0..16."""
    for bits in (17, 31):
        _, helds = _run_pack(_tokens(600, bits, seed=bits), bits, [1] * 600, True)
        assert set(helds[:8]) == set(range(8)) and set(helds) == set(range(8))
    data = _stream_bytes(_tokens(600, 17, seed=3), 17)
    _, helds = _run_unpack(data, 17, [1] * len(data), True)
    assert set(helds[:17]) == set(range(17)) and set(helds) == set(range(17))


def test_geometry_refuses_bad_arguments():
    for bits in (0, 33, -1, 1.5, True):
        with pytest.raises(ValueError):
            pack_advance(PackState(), 1, False, bits)
        with pytest.raises(ValueError):
            unpack_advance(UnpackState(), 1, False, bits)
        with pytest.raises(ValueError):
            packed_bytes(1, bits)
    with pytest.raises(ValueError):
        pack_advance(PackState(), -1, False, 17)
    with pytest.raises(ValueError):
        unpack_advance(UnpackState(), -1, False, 17)
    with pytest.raises(ValueError):
        packed_bytes(-1, 17)
    assert packed_bytes(0, 17) == 0 and packed_bytes(1, 1) == 1 and packed_bytes(3, 17) == 7 and packed_bytes(2 ** 40, 32) == 2 ** 42


# ---- the C surface ----------------------------------------------------------------------------------------------------------------------
def test_packed_bytes_of_the_library():
    lib = _capi.load_library()
    for bits in range(1, 33):
        for n in (0, 1, 7, 8, 9, 33):
            assert lib.l3ac_packed_bytes(n, bits) == len(_stream_bytes([1 << (bits - 1)] * n, bits)) == packed_bytes(n, bits)
        for n in (600, 2 ** 31, 2 ** 40 + 1):
            assert lib.l3ac_packed_bytes(n, bits) == (n * bits + 7) // 8 == packed_bytes(n, bits)
    for n, bits in ((1, 0), (1, 33), (1, -1), (-1, 17), (-2 ** 40, 8)):
        assert lib.l3ac_packed_bytes(n, bits) < 0


def test_header_and_binding_agree_on_the_wire_entries():
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5
    assert _capi.load_library().l3ac_abi_version() == 5
    for struct_name, binding in (("l3ac_pack_stream_desc", _capi.PackStreamDesc), ("l3ac_unpack_stream_desc", _capi.UnpackStreamDesc)):
        m = re.search(r"typedef struct " + struct_name + r" \{(.*?)\} " + struct_name + ";", header, re.S)
        fields = re.findall(r"\b(int32_t|int64_t)\s+(\w+);", m.group(1))
        assert fields == [("int32_t", n) for n in ("slot", "held", "take", "count", "keep")]
        assert [n for n, _ in binding._fields_] == [n for _, n in fields] and all(t is ctypes.c_int32 for _, t in binding._fields_)
        assert ctypes.sizeof(binding) == 20
    for name in ("StreamPacker", "StreamUnpacker", "stream_packer", "stream_unpacker", "packed_bytes", "pack_advance", "unpack_advance",
                 "frame_header", "parse_frame"):
        assert name in l3ac_amd.__all__ and hasattr(l3ac_amd, name)
    from l3ac_amd import build
    assert "kernels/bitpack_stream.hip" in build.SOURCES and "kernels/bitpack.hip" in build.SOURCES


def test_pack_entry_checks_its_descriptors_before_any_launch():
    """Null stream, bogus (never dereferenced) device pointers: the host-side checks refuse first."""
    lib = _capi.load_library()
    a, b, f, y = (ctypes.c_void_p(1 << k) for k in (20, 24, 28, 32))

    def call(rows, state_in=a, state_out=b, streams=2, fresh=f, tokens=10, stride=None, bits=17, out=y, out_bytes=24, out_stride=24):
        desc = (_capi.PackStreamDesc * len(rows))(*[_capi.PackStreamDesc(*r) for r in rows])
        return lib.l3ac_pack_stream(state_in, state_out, streams, fresh, tokens, tokens if stride is None else stride, bits, desc, len(rows), out,
                                    out_bytes, out_stride, None)
    #       slot held take count keep          3 + 10 * 17 = 173 bits: 21 bytes and 5 bits, or 22 bytes ended
    good = (0, 3, 10, 21, 5)
    assert call([(2,) + good[1:]]) == -1 and b"stream 2 of 2" in lib.l3ac_last_error()          # slot out of range
    assert call([(-1,) + good[1:]]) == -1
    assert call([good, good]) == -1 and b"one stream" in lib.l3ac_last_error()                 # two descriptors for one stream
    assert call([(0, 8, 10, 22, 2)]) == -1 and b"holds 8 bits" in lib.l3ac_last_error()        # held out of range
    assert call([(0, -1, 10, 21, 1)]) == -1
    assert call([(0, 3, 11, 23, 6)]) == -1 and b"takes 11 of 10" in lib.l3ac_last_error()      # take beyond the packet
    assert call([good], fresh=None) == -1                                                      # ... from nowhere
    assert call([good], out_bytes=20) == -1 and b"emits 21" in lib.l3ac_last_error()           # count beyond the output row
    assert call([(0, 3, 10, 21, 4)]) == -1 and b"21 bytes and 5 bits" in lib.l3ac_last_error()  # keep inconsistent
    assert call([(0, 3, 10, 20, 5)]) == -1 and call([(0, 3, 10, 22, 5)]) == -1                 # count inconsistent (either form)
    assert call([(0, 3, 10, 23, 0)]) == -1
    assert call([good], state_in=None) == -1 and call([good], state_out=None) == -1            # bits to carry and nowhere to carry them
    assert b"state buffer is null" in lib.l3ac_last_error()
    assert call([good], state_out=a) == -1 and b"overlap" in lib.l3ac_last_error()             # next state on top of the state
    assert call([good], out=f) == -1 and b"overlap" in lib.l3ac_last_error()                   # output on top of the packet
    assert call([good], out=None) == -1 and call([good], out_bytes=25) == -1                   # no output; out_bytes above the stride
    assert call([good], out_stride=26, out_bytes=24) == -1 and b"multiple of 4" in lib.l3ac_last_error()
    assert call([good], out=ctypes.c_void_p((1 << 32) + 2)) == -1 and b"aligned" in lib.l3ac_last_error()
    assert call([good], fresh=ctypes.c_void_p((1 << 28) + 2)) == -1
    assert call([good], stride=9) == -1                                                        # rows shorter than the packet
    assert call([good], bits=0) == -1 and call([good], bits=33) == -1 and b"outside 1..32" in lib.l3ac_last_error()
    assert call([]) == -1 and call([good], streams=0) == -1
    assert call([(0, 0, 2 ** 31 - 1, 0, 0)], tokens=2 ** 31 - 1, bits=32) == -1                # 2^33 bytes do not fit a descriptor
    # nothing to emit and nothing to keep: accepted with every buffer null, and nothing is launched
    assert call([(0, 0, 0, 0, 0), (1, 0, 0, 0, 0)], state_in=None, state_out=None, fresh=None, tokens=0, stride=1, out=None, out_bytes=0, out_stride=0) == 0


def test_unpack_entry_checks_its_descriptors_before_any_launch():
    lib = _capi.load_library()
    a, b, f, y = (ctypes.c_void_p(1 << k) for k in (20, 24, 28, 32))

    def call(rows, state_in=a, state_out=b, streams=2, fresh=f, nbytes=22, stride=None, bits=17, out=y, out_tokens=10, out_stride=10):
        desc = (_capi.UnpackStreamDesc * len(rows))(*[_capi.UnpackStreamDesc(*r) for r in rows])
        return lib.l3ac_unpack_stream(state_in, state_out, streams, fresh, nbytes, nbytes if stride is None else stride, bits, desc, len(rows), out,
                                      out_tokens, out_stride, None)
    #       slot held take count keep          5 + 8 * 21 = 173 bits: 10 tokens and 3 bits
    good = (0, 5, 21, 10, 3)
    assert call([(2,) + good[1:]]) == -1 and b"stream 2 of 2" in lib.l3ac_last_error()
    assert call([good, good]) == -1 and b"one stream" in lib.l3ac_last_error()
    assert call([(0, 17, 21, 10, 15)]) == -1 and b"holds 17 bits, outside 0..16" in lib.l3ac_last_error()
    assert call([(0, -1, 21, 9, 14)]) == -1
    assert call([(0, 5, 23, 11, 2)]) == -1 and b"takes 23 of 22" in lib.l3ac_last_error()
    assert call([good], fresh=None) == -1
    assert call([good], out_tokens=9) == -1 and b"emits 10" in lib.l3ac_last_error()
    assert call([(0, 5, 21, 10, 4)]) == -1 and b"10 tokens of 17 bits and 3 bits" in lib.l3ac_last_error()
    assert call([(0, 5, 21, 9, 3)]) == -1 and call([(0, 5, 21, 11, 0)]) == -1 and call([(0, 5, 21, 9, 0)]) == -1
    assert call([good], state_in=None) == -1 and call([good], state_out=None) == -1
    assert call([good], state_out=a) == -1 and b"overlap" in lib.l3ac_last_error()
    assert call([good], out=f) == -1 and b"overlap" in lib.l3ac_last_error()
    assert call([good], out=None) == -1 and call([good], out_tokens=11) == -1
    assert call([good], out=ctypes.c_void_p((1 << 32) + 2)) == -1 and b"aligned" in lib.l3ac_last_error()
    assert call([good], bits=0) == -1 and call([good], bits=33) == -1
    assert call([]) == -1 and call([good], streams=0) == -1
    # the byte rows may start anywhere; an ended stream drops its padding: both forms pass the checks up to the launch, which a null-sized
    # output with nothing to keep skips
    assert call([(0, 0, 0, 0, 0)], state_in=None, state_out=None, fresh=None, nbytes=0, stride=1, out=None, out_tokens=0, out_stride=0) == 0


# ---- sessions and functions: the checks that need no device ---------------------------------------------------------------------------
@pytest.mark.parametrize("make,fresh", [(l3ac_amd.stream_packer, PackState()), (l3ac_amd.stream_unpacker, UnpackState())])
def test_session_arguments_are_checked_before_a_device_is_needed(make, fresh):
    for bits in (7, 33, 0, 17.5, True):
        with pytest.raises(ValueError, match="bits"):
            make(2, bits)
    for streams in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="streams"):
            make(streams, 17)
    for bits in (8, 17, 18, 32):
        assert make(1, bits).bits == bits
    s = make(2, 17)
    assert isinstance(s, (l3ac_amd.StreamPacker, l3ac_amd.StreamUnpacker)) and s.states == [fresh] * 2 and s.streams == 2
    piece = torch.zeros(2, 100, dtype=torch.uint8 if make is l3ac_amd.stream_unpacker else torch.int32)
    for bad in (piece[0], torch.zeros(3, 100, dtype=piece.dtype), piece[:, :, None], piece.to(torch.float32), "abc", None):
        with pytest.raises(ValueError):
            s.push(bad)
    for bad in ([-1, 5], [101, 5], [5], [5] * 3, [1.5, 5], "ab"):
        with pytest.raises(ValueError):
            s.push(piece, lengths=bad)
    with pytest.raises(ValueError):
        s.push(piece, end=[True])
    with pytest.raises(RuntimeError, match="is on cpu"):
        s.push(piece, lengths=[100, 3], end=[False, True])
    assert s.states == [fresh] * 2
    with pytest.raises(ValueError):
        s.reset(streams=2)
    s.reset(streams=[1])
    s.reset()


def test_ragged_functions_check_their_arguments_before_a_device_is_needed():
    idx = torch.zeros(2, 10, dtype=torch.int32)
    with pytest.raises(ValueError):
        l3ac_amd.pack_indices(idx, 17, lengths=[1, 2])  # no CPU path
    with pytest.raises(ValueError):
        l3ac_amd.unpack_indices(torch.zeros(2, 24, dtype=torch.uint8), 10, 17, lengths=[1, 2])
    assert wire.token_lengths([0, 10], 2, 10) == [0, 10] and wire.token_lengths(torch.tensor([3, 0]), 2, 10) == [3, 0]
    for bad in ([-1, 5], [11, 5], [5], [5] * 3, [1.5, 5], "ab", 5):
        with pytest.raises(ValueError):
            wire.token_lengths(bad, 2, 10)


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
def _mc(tag):
    return l3ac_amd.L3ACConfig(config_file=l3ac_amd.config.resolve_config_file(tag)).network_config


def test_frame_header_round_trip_and_every_corrupted_field():
    mc, rate = _mc("1kbps"), 16000
    bits, hop = l3ac_amd.bits_per_token(mc), mc.hop_length
    assert bits == 17
    n_samples = 7 * hop + 1
    n_tok = 8
    payload = bytes(range(packed_bytes(n_tok, bits)))
    head = l3ac_amd.frame_header(mc, rate, n_tok, n_samples)
    assert len(head) == 24 == wire.FRAME_HEADER_BYTES
    assert head == b"L3AC" + struct.pack("<BBHIIII", 1, bits, hop, mc.codebook_size, rate, n_tok, n_samples)
    frame = l3ac_amd.parse_frame(head + payload, mc, rate)
    assert frame == (n_tok, n_samples, payload) and frame.n_tok == n_tok and frame.n_samples == n_samples and frame.payload == payload
    assert l3ac_amd.parse_frame(bytearray(head + payload), mc, rate).payload == payload

    def corrupt(offset, fmt, value):
        blob = bytearray(head + payload)
        struct.pack_into(fmt, blob, offset, value)
        return bytes(blob)
    for blob, field in ((corrupt(0, "<4s", b"L3AD"), "magic"), (corrupt(4, "<B", 2), "version"), (corrupt(5, "<B", bits + 1), "bits"),
                        (corrupt(6, "<H", hop + 1), "hop"), (corrupt(8, "<I", mc.codebook_size + 1), "codebook size"),
                        (corrupt(12, "<I", 48000), "sample rate"), (corrupt(16, "<I", n_tok + 1), "token count"),
                        (corrupt(16, "<I", 0), "token count"), (corrupt(20, "<I", n_samples + hop), "sample count"),
                        (head + payload[:-1], "payload"), (head + payload + b"\0", "payload"), (head, "payload"), (head[:23], "header")):
        with pytest.raises(ValueError, match=field):
            l3ac_amd.parse_frame(blob, mc, rate)
    with pytest.raises(ValueError, match="sample rate"):
        l3ac_amd.parse_frame(head + payload, mc, 44100)
    with pytest.raises(ValueError):
        l3ac_amd.parse_frame(12, mc, rate)
    # a frame of another model is refused by this one, field by field
    other = _mc("3kbps")
    assert l3ac_amd.bits_per_token(other) == 18
    theirs = l3ac_amd.frame_header(other, rate, n_tok, (n_tok - 1) * other.hop_length + 1) + bytes(packed_bytes(n_tok, 18))
    assert l3ac_amd.parse_frame(theirs, other, rate).n_tok == n_tok
    with pytest.raises(ValueError, match="bits"):
        l3ac_amd.parse_frame(theirs, mc, rate)


def test_decompress_refuses_bad_frames_before_any_device_work():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)  # stays on the CPU: everything below raises before it needs a device
    mc = codec.network.mc
    good = l3ac_amd.frame_header(mc, codec.config.sample_rate, 2, mc.hop_length + 1) + bytes(packed_bytes(2, 17))
    for frames in ([good, good[:-1]], [good + b"\0"], [b"XXXX" + good[4:]], [], good):
        with pytest.raises(ValueError):
            codec.decompress(frames)
    with pytest.raises(ValueError, match="bits"):
        other = _mc("3kbps")
        codec.decompress([l3ac_amd.frame_header(other, 16000, 2, other.hop_length + 1) + bytes(packed_bytes(2, 18))])
