"""Batches of long recordings, host side (no GPU): the library's chunk planner against ChunkData, the C surface of the chunk
entries, and the argument checks of encode_long / decode_long that happen before any device work."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.chunking import ChunkData

REPO = Path(__file__).resolve().parent.parent
ENTRIES = ("l3ac_chunk_plan", "l3ac_chunk_cut", "l3ac_chunk_merge")


def _plan(frames, chunk_len, prefix_len, round_to=1):
    return [(d.rec, d.row, d.start, d.frames, d.prefix, d.pad, d.last) for d in l3ac_amd.chunk_plan(frames, chunk_len, prefix_len, round_to)]


def _grid():
    """(n, chunk_len, prefix_len): n below, at and one over whole chunks, the largest prefix, no prefix."""
    out = []
    for chunk_len in (2, 5, 16, 296):
        for prefix_len in sorted({0, 1, chunk_len // 2, chunk_len - 1}):
            if prefix_len >= chunk_len:
                continue
            for k in (1, 2, 3, 7):
                for n in (k * chunk_len - 1, k * chunk_len, k * chunk_len + 1):
                    if n >= 1:
                        out.append((n, chunk_len, prefix_len))
            out.append((1, chunk_len, prefix_len))
    return out


@pytest.mark.parametrize("n,chunk_len,prefix_len", _grid())
def test_plan_is_chunkdata(n, chunk_len, prefix_len):
    data = torch.arange(n)
    want = ChunkData(chunk_len=chunk_len, prefix_len=prefix_len, original_data=data).chunk_data
    got = _plan([n], chunk_len, prefix_len)
    assert len(got) == len(want)
    parts = []
    for j, ((rec, row, start, frames, prefix, pad, last), w) in enumerate(zip(got, want)):
        assert (rec, row, pad) == (0, j, 0)
        assert (start, frames) == (int(w[0]), w.numel()), (j, start, frames)  # w is a narrow of arange: its first value is its start
        assert prefix == (0 if j == 0 else prefix_len)
        assert last == int(j == len(want) - 1)
        parts.append(data[start + prefix:start + frames])  # drop the prefix, concatenate
    assert torch.equal(torch.cat(parts), data)


def test_plan_of_several_recordings_is_the_single_plans_in_a_row():
    frames = [1, 296, 297, 5 * 296, 5 * 296 + 1, 40, 3000]
    got = _plan(frames, 296, 30)
    row = 0
    for b, n in enumerate(frames):
        alone = _plan([n], 296, 30)
        mine = [d for d in got if d[0] == b]
        assert [d[1] for d in mine] == list(range(row, row + len(alone)))  # rows numbered consecutively
        assert [d[2:] for d in mine] == [d[2:] for d in alone]
        row += len(alone)
    assert row == len(got)


def test_plan_rounds_each_recording_up_and_marks_the_added_frames():
    """Audio: a recording is padded to whole hops first (Network.preprocess); the frames that adds are `pad` of its last chunk."""
    hop = 270
    for n in (1, 269, 270, 271, 540, 541, 2 * 540 + 5):
        got = _plan([n], 540, 270, hop)
        padded = -(-n // hop) * hop
        assert [d[2:4] for d in got] == [d[2:4] for d in _plan([padded], 540, 270)]
        assert sum(d[5] for d in got) == got[-1][5] == padded - n
        assert got[-1][2] + got[-1][3] == padded


@pytest.mark.parametrize("frames,chunk_len,prefix_len,round_to", [([10], 3, 3, 1), ([10], 3, 4, 1), ([10], 0, 0, 1), ([10], 3, -1, 1), ([0], 3, 1, 1),
                                                                  ([5, -2], 3, 1, 1), ([10], 3, 1, 0), ([], 3, 1, 1)])
def test_plan_refuses_bad_arguments(frames, chunk_len, prefix_len, round_to):
    lib = _capi.load_library()
    host = (ctypes.c_int64 * max(len(frames), 1))(*frames)
    desc = (_capi.ChunkDesc * 16)()
    for d in desc:
        d.row = -7
    assert lib.l3ac_chunk_plan(host, len(frames), chunk_len, prefix_len, round_to, desc, 16) < 0
    assert b"chunk_plan" in lib.l3ac_last_error()
    assert all(d.row == -7 for d in desc)  # an error, not a partial plan
    with pytest.raises(ValueError):
        l3ac_amd.chunk_plan(frames, chunk_len, prefix_len, round_to)


def test_plan_refuses_a_cap_that_is_too_small():
    lib = _capi.load_library()
    host = (ctypes.c_int64 * 2)(100, 35)
    assert lib.l3ac_chunk_plan(host, 2, 10, 2, 1, None, 0) == 14
    desc = (_capi.ChunkDesc * 14)()
    for d in desc:
        d.row = -7
    assert lib.l3ac_chunk_plan(host, 2, 10, 2, 1, desc, 13) < 0
    assert all(d.row == -7 for d in desc)
    assert lib.l3ac_chunk_plan(host, 2, 10, 2, 1, desc, 14) == 14
    assert [d.row for d in desc] == list(range(14))


def test_plan_offsets_are_64_bit():
    """Ten hours of 16 kHz audio: starts pass 2^31 only far beyond any clip, but the field must not wrap."""
    n = 3 * 2 ** 30
    got = _plan([n], 2 ** 20, 2 ** 10)
    assert got[-1][2] + got[-1][3] == n and got[-1][2] > 2 ** 31


def test_cut_and_merge_check_their_descriptors_before_any_launch():
    """Null stream, bogus (never dereferenced) device pointers: the host-side checks refuse first."""
    lib = _capi.load_library()
    desc = l3ac_amd.chunk_plan([25], 10, 3)
    fake = ctypes.c_void_p(4096)
    assert lib.l3ac_chunk_cut(fake, 1, 24, 1, desc, len(desc), fake, 3, 13, None) == -1   # source row shorter than the recording
    assert lib.l3ac_chunk_cut(fake, 1, 25, 1, desc, len(desc), fake, 3, 12, None) == -1   # chunk rows too short
    assert lib.l3ac_chunk_cut(fake, 1, 25, 1, desc, len(desc), fake, 2, 13, None) == -1   # too few chunk rows
    assert lib.l3ac_chunk_cut(fake, 1, 25, 0, desc, len(desc), fake, 3, 13, None) == -1   # c
    assert lib.l3ac_chunk_cut(None, 1, 25, 1, desc, len(desc), fake, 3, 13, None) == -1
    assert lib.l3ac_chunk_merge(fake, 3, 13, 1, desc, len(desc), fake, 1, 25, 24, None) == -1  # out_frames below the recording's end
    assert lib.l3ac_chunk_merge(fake, 3, 13, 1, desc, len(desc), fake, 1, 24, 25, None) == -1  # out_frames above the row stride
    assert lib.l3ac_chunk_merge(fake, 3, 13, 1, desc, len(desc), fake, 0, 25, 25, None) == -1  # recording 0 of 0
    assert b"chunk_merge" in lib.l3ac_last_error()


def test_header_and_binding_agree_on_the_chunk_entries():
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5
    # the descriptor's layout: two int32, one int64, four int32
    m = re.search(r"typedef struct l3ac_chunk_desc \{(.*?)\} l3ac_chunk_desc;", header, re.S)
    fields = re.findall(r"\b(int32_t|int64_t)\s+(\w+);", m.group(1))
    assert [(t, n) for t, n in fields] == [({ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t"}[t], n) for n, t in _capi.ChunkDesc._fields_]
    assert ctypes.sizeof(_capi.ChunkDesc) == 32
    assert "chunk_plan" in l3ac_amd.__all__


def test_chunk_kernels_are_built_and_declared():
    from l3ac_amd import build
    assert "kernels/chunk.hip" in build.SOURCES
    assert (REPO / "l3ac_amd" / "csrc" / "kernels" / "chunk.hip").exists()
    # the header is the entries' one declaration; they are defined in the family's own file, not forwarded from capi.hip
    hip = (REPO / "l3ac_amd" / "csrc" / "kernels" / "chunk.hip").read_text()
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    for name in ("l3ac_chunk_cut", "l3ac_chunk_merge"):
        assert re.search(r"^int " + name + r"\(", header, re.M) and re.search(r"^int " + name + r"\([^;{]*\) \{", hip, re.M), name


@pytest.fixture(scope="module")
def codec():
    return l3ac_amd.get_model("1kbps", synthetic_seed=0)  # stays on the CPU: everything below raises before it needs a device


def test_encode_long_checks_arguments_before_any_device_work(codec):
    audio = torch.zeros(3, 5000)
    for bad in ([0, 5000, 5000], [5001, 10, 10], [10, 10], [10, 10, 10, 10], [1.5, 10, 10]):
        with pytest.raises(ValueError):
            codec.encode_long(audio, lengths=bad)
    with pytest.raises(ValueError):
        codec.encode_long(torch.zeros(5000))
    hop, win = codec.network.mc.hop_length, codec.network.mc.en_coder_window_size
    with pytest.raises(ValueError, match="must exceed the overlap"):
        codec.encode_long(audio, process_window=win * hop)          # default prefix: the attention window
    with pytest.raises(ValueError, match="must exceed the overlap"):
        codec.encode_long(audio, process_window=2 * hop + 5, prefix_tokens=2)
    with pytest.raises(ValueError):
        codec.encode_long(audio, chunks_per_call=0)
    with pytest.raises(ValueError):
        codec.encode_long(audio, sample_rate=16001)
    with pytest.raises(RuntimeError):  # arguments fine: now the missing device / training mode speaks
        codec.encode_long(audio, lengths=[5000, 10, 10])


def test_decode_long_checks_arguments_before_any_device_work(codec):
    mc = codec.network.mc
    with pytest.raises(ValueError, match="audio_feature or indices"):
        codec.decode_long()
    idx = torch.zeros(2, 40, dtype=torch.int32)
    for bad in ([0, 40], [41, 40], [40], [40, 40, 40], [2.5, 40]):
        with pytest.raises(ValueError):
            codec.decode_long(indices=idx, lengths=bad)
    with pytest.raises(ValueError):
        codec.decode_long(indices=torch.zeros(40, dtype=torch.int32))
    with pytest.raises(ValueError):
        codec.decode_long(torch.zeros(2, 40, mc.feature_dim + 1))
    with pytest.raises(ValueError, match="must exceed the overlap"):
        codec.decode_long(indices=idx, process_window=mc.en_coder_window_size * mc.hop_length)
    with pytest.raises(ValueError):
        codec.decode_long(indices=idx, sample_rate=-1)
    with pytest.raises(RuntimeError):
        codec.decode_long(indices=idx)


def test_decode_long_refuses_a_chunk_too_short_for_the_first_enhance_block():
    codec3 = l3ac_amd.get_model("3kbps", synthetic_seed=0)
    mc = codec3.network.mc
    assert mc.en_coder_compress_rate == 1  # a one-token chunk is a single frame there
    idx = torch.zeros(2, 40, dtype=torch.int32)
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        codec3.decode_long(indices=idx, lengths=[40, 1])
    with pytest.raises(ValueError, match="more than 1 spatial element"):  # 13 tokens = chunks of 6, 6 and 1 (no prefix)
        codec3.decode_long(indices=idx, lengths=[40, 13], process_window=6 * mc.hop_length, prefix_tokens=0)
    with pytest.raises(RuntimeError):  # with a prefix the last chunk has two tokens: fine until the device is needed
        codec3.decode_long(indices=idx, lengths=[40, 13], process_window=6 * mc.hop_length, prefix_tokens=1)
