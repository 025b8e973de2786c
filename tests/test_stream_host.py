"""Streaming sessions, host side (no GPU): the push geometry of l3ac_amd/streaming.py against the library's chunk planner (look-back
below the step) and against a brute-force restatement of the formula (any look-back), the emitted counts, the C surface of the stream
entries and the argument checks that need no device."""
import ctypes
import random
import re
from pathlib import Path

import pytest

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.streaming import StreamRow, StreamState, advance, check_geometry, emitted, leftover

REPO = Path(__file__).resolve().parent.parent
ENTRIES = ("l3ac_stream_gather", "l3ac_stream_carry", "l3ac_stream_append", "l3ac_stream_emit")


def _grid():
    """(n, CL, P, hop): P below, at and above CL; n below, at and one frame over whole steps and whole hops."""
    out = []
    for hop, cl_tok in ((1, 1), (1, 5), (3, 2), (270, 8), (270, 1)):
        cl = cl_tok * hop
        for p_tok in sorted({0, 1, cl_tok // 2, max(cl_tok - 1, 0), cl_tok, cl_tok + 1, 3 * cl_tok + 1}):
            p = p_tok * hop
            ns = {1, hop - 1, hop, hop + 1}
            for k in (1, 2, 5):
                ns |= {k * cl - 1, k * cl, k * cl + 1, k * cl + hop - 1, k * cl + hop, k * cl + hop + 1}
            out += [(n, cl, p, hop) for n in sorted(ns) if n >= 1]
    return out


GRID = _grid()


def _brute(n, cl, p, hop):
    """The formula of DESIGN.md section 3.9, restated frame by frame: chunk k covers [max(0, k CL - P), min(n', (k + 1) CL))."""
    padded = n
    while padded % hop:
        padded += 1
    rows, k = [], 0
    while k * cl < padded:
        start = max(0, k * cl - p)
        stop = min(padded, (k + 1) * cl)
        real = [f for f in range(start, stop) if f < n]
        rows.append((start, stop - start, k * cl - start, (stop - start) - len(real)))
        k += 1
    return rows


def _splits(n, rng, count=4):
    """Ways to deliver n frames: all at once, frame-sized packets' worth of random cuts, zero-length pushes in between, and either
    `end` on the last data push or a final empty `end` push."""
    out = [([n], True), ([n], False)]
    for _ in range(count):
        cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(1, 6)))
        parts = [b - a for a, b in zip([0] + cuts, cuts + [n])]
        if rng.random() < 0.5:
            parts.insert(rng.randint(0, len(parts)), 0)
        out.append((parts, rng.random() < 0.5))
    return out


def _run(parts, end_on_last, cl, p, hop):
    """Push `parts`, checking every push on the way; returns (rows as (start, frames, prefix, pad), the states after every push)."""
    state = StreamState()
    rows, states = [], []
    seen = 0
    pushes = [(m, end_on_last and i == len(parts) - 1) for i, m in enumerate(parts)] + ([] if end_on_last else [(0, True)])
    for m, end in pushes:
        got, after = advance(state, m, end, cl, p, hop)
        # every row is what the state holds, then new frames, then zeros; offsets walk through the push
        off = 0
        held = state.held
        for r in got:
            assert isinstance(r, StreamRow)
            assert r.held == held and r.off == off and r.frames == r.held + r.take + r.pad and r.prefix <= r.held
            assert 0 <= r.keep <= r.frames - r.pad and r.keep <= p
            off += r.take
            held = r.keep
        tail = leftover(got, after, m)
        if end:
            assert after == StreamState() and tail is None and off == m
        else:
            seen += m
            assert after.seen == seen and after.held <= p + cl - 1 and after.pending < cl and after.context <= p
            assert after.pending == seen % cl and after.context == min(p, seen // cl * cl)
            if tail is None:
                assert off == m and after.held == held
            else:
                assert tail == (held, off, m - off) and after.held == held + m - off
            emitted_so_far = sum(r.frames - r.prefix for r in rows + got) // hop
            assert emitted_so_far == seen // cl * (cl // hop) == emitted(seen, False, cl, hop)
        rows += got
        states.append(after)
        state = after
    return [(r.start, r.frames, r.prefix, r.pad) for r in rows], states


@pytest.mark.parametrize("n,cl,p,hop", GRID)
def test_rows_of_any_split_are_the_plan(n, cl, p, hop):
    rng = random.Random(n * 7919 + cl * 31 + p)
    want = _brute(n, cl, p, hop)
    if p < cl:  # the offline chunker's geometry: the library's planner says the same
        plan = [(d.start, d.frames, d.prefix, d.pad) for d in l3ac_amd.chunk_plan([n], cl, p, hop)]
        assert plan == want
    for parts, end_on_last in _splits(n, rng):
        rows, _ = _run(parts, end_on_last, cl, p, hop)
        assert rows == want, (parts, end_on_last)
        assert sum(f - pre for _, f, pre, _ in rows) // hop == -(-n // hop) == emitted(n, True, cl, hop)


def test_grid_covers_look_backs_on_both_sides_of_the_step():
    assert any(p < cl for _, cl, p, _ in GRID) and any(p == cl for _, cl, p, _ in GRID) and any(p > 2 * cl for _, cl, p, _ in GRID)


def test_look_back_grows_until_it_is_full():
    state = StreamState()
    seen = []
    for _ in range(6):
        rows, state = advance(state, 8, False, 8, 20)
        seen.append((rows[0].prefix, rows[0].frames, rows[0].keep))
    assert seen == [(0, 8, 8), (8, 16, 16), (16, 24, 20), (20, 28, 20), (20, 28, 20), (20, 28, 20)]
    assert state == StreamState(20, 0, 48)
    rows, after = advance(state, 8, False, 8, 20)  # the steady push: the state it leaves is the state it found, but for the count
    assert after[:2] == state[:2]


def test_an_empty_end_on_a_fresh_or_whole_step_stream_emits_nothing():
    assert advance(StreamState(), 0, True, 8, 3) == ([], StreamState())
    rows, state = advance(StreamState(), 16, False, 8, 3)
    assert len(rows) == 2 and advance(state, 0, True, 8, 3) == ([], StreamState())


def test_geometry_refuses_bad_arguments():
    for step, lookback, hop in ((0, 0, 1), (5, -1, 1), (271, 0, 270), (270, 5, 270), (100, 0, 270)):
        with pytest.raises(ValueError):
            check_geometry(step, lookback, hop)
    with pytest.raises(ValueError):
        advance(StreamState(), -1, False, 8, 3)


def test_header_and_binding_agree_on_the_stream_entries():
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5
    m = re.search(r"typedef struct l3ac_stream_desc \{(.*?)\} l3ac_stream_desc;", header, re.S)
    fields = re.findall(r"\b(int32_t|int64_t)\s+(\w+);", m.group(1))
    assert fields == [({ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t"}[t], n) for n, t in _capi.StreamDesc._fields_]
    assert ctypes.sizeof(_capi.StreamDesc) == 48
    for name in ("StreamEncoder", "StreamDecoder"):
        assert name in l3ac_amd.__all__ and hasattr(l3ac_amd, name)
    assert hasattr(l3ac_amd.L3AC, "stream_encoder") and hasattr(l3ac_amd.L3AC, "stream_decoder")
    from l3ac_amd import build
    assert "kernels/stream.hip" in build.SOURCES


def test_stream_kernels_check_their_descriptors_before_any_launch():
    """Null stream, bogus (never dereferenced) device pointers: the host-side checks refuse first."""
    lib = _capi.load_library()
    a, b, f = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p(1 << 28)

    def desc(*rows):
        return (_capi.StreamDesc * len(rows))(*[_capi.StreamDesc(*r) for r in rows])
    #             slot row held take off pad keep prefix zero out
    ok = desc((0, 0, 3, 5, 0, 1, 4, 3, 0, 0))
    assert lib.l3ac_stream_gather(a, 1, 8, f, 4, 4, 1, ok, 1, b, 1, 12, None) == -1        # takes 5 of 4 new frames
    assert lib.l3ac_stream_gather(a, 1, 2, f, 5, 5, 1, ok, 1, b, 1, 12, None) == -1        # holds 3 of a 2-frame state row
    assert lib.l3ac_stream_gather(a, 1, 8, f, 5, 5, 1, ok, 1, b, 1, 8, None) == -1         # 9 frames in rows of 8
    assert lib.l3ac_stream_gather(a, 1, 8, None, 5, 5, 1, ok, 1, b, 1, 12, None) == -1     # new frames taken from nowhere
    assert lib.l3ac_stream_gather(a, 1, 8, f, 5, 5, 1, ok, 1, a, 1, 12, None) == -1        # rows on top of the state
    two = desc((0, 0, 3, 5, 0, 0, 4, 3, 0, 0), (1, 0, 3, 5, 0, 0, 4, 3, 0, 0))
    assert lib.l3ac_stream_gather(a, 2, 8, f, 5, 5, 1, two, 2, b, 1, 12, None) == -1       # two chunks into one row
    assert b"stream_gather" in lib.l3ac_last_error()
    assert lib.l3ac_stream_carry(b, 1, 12, 1, desc((0, 0, 3, 5, 0, 0, 9, 0, 0, 0)), 1, a, 1, 16, None) == -1   # keeps 9 of 8 frames
    assert lib.l3ac_stream_carry(b, 1, 12, 1, desc((0, 0, 3, 5, 0, 0, 8, 0, 0, 0)), 1, a, 1, 7, None) == -1    # ... in a 7-frame state row
    assert lib.l3ac_stream_carry(b, 1, 12, 1, desc((2, 0, 3, 5, 0, 0, 8, 0, 0, 0)), 1, a, 2, 8, None) == -1    # stream 2 of 2
    assert b"stream_carry" in lib.l3ac_last_error()
    assert lib.l3ac_stream_append(f, 5, 5, 1, desc((0, 0, 4, 5, 0, 0, 0, 0, 0, 0)), 1, a, 1, 8, None) == -1    # 4 + 5 frames in 8
    assert lib.l3ac_stream_append(f, 5, 5, 1, desc((0, 0, 1, 5, 1, 0, 0, 0, 0, 0)), 1, a, 1, 8, None) == -1    # reads to frame 6 of 5
    assert b"stream_append" in lib.l3ac_last_error()
    assert lib.l3ac_stream_emit(b, 1, 12, 1, desc((0, 0, 8, 0, 0, 0, 0, 3, 2, 0)), 1, a, 1, 6, 6, None) == -1  # 5 + 2 frames of 6
    assert lib.l3ac_stream_emit(b, 1, 12, 1, desc((0, 0, 8, 0, 0, 0, 0, 9, 0, 0)), 1, a, 1, 6, 6, None) == -1  # prefix beyond the row
    assert lib.l3ac_stream_emit(b, 1, 12, 1, desc((0, 0, 8, 0, 0, 0, 0, 3, 0, 0), (0, 0, 8, 0, 0, 0, 0, 3, 0, 4)), 2, a, 1, 16, 16, None) == -1  # overlap
    assert lib.l3ac_stream_emit(b, 1, 12, 1, desc((0, 0, 8, 0, 0, 0, 0, 3, 0, 0)), 1, a, 1, 6, 7, None) == -1  # out_frames above the stride
    assert b"stream_emit" in lib.l3ac_last_error()


@pytest.fixture(scope="module")
def codec():
    return l3ac_amd.get_model("1kbps", synthetic_seed=0)  # stays on the CPU: everything below raises before it needs a device


@pytest.mark.parametrize("make", ["stream_encoder", "stream_decoder"])
def test_session_arguments_are_checked_before_a_device_is_needed(codec, make):
    hop = codec.network.mc.hop_length
    fn = getattr(codec, make)
    for kw in (dict(streams=0), dict(streams=-1), dict(streams=1.5), dict(streams=2, process_window=hop - 1), dict(streams=2, prefix_tokens=-1),
               dict(streams=2, prefix_tokens=2.5), dict(streams=2, chunks_per_call=0)):
        with pytest.raises(ValueError):
            fn(**kw)
    with pytest.raises(RuntimeError, match="not on a GPU"):  # arguments fine (a step of one hop, a look-back far above it)
        fn(streams=2, process_window=hop, prefix_tokens=250)
    with pytest.raises(TypeError):
        fn(streams=2, sample_rate=48000)  # not part of a session
