"""Streaming sample-rate conversion, host side (no GPU): the push geometry of l3ac_amd/streaming.py against a restatement output by output,
its independence of a stream's age, the C surface of the new entries and the argument checks that need no device."""
import ctypes
import random
import re
from pathlib import Path

import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.streaming import ResamplePush, ResampleState, resample_advance, resample_geometry, round4

REPO = Path(__file__).resolve().parent.parent
PAIRS = [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000), (48000, 8000), (44100, 48000), (16000, 11025), (1024, 1), (1, 1024)]
EQUAL = (16000, 16000)


def _lengths(geo, rng):
    return sorted({1, 2, geo.down, geo.down + 1, geo.half_len // geo.up + 1} | {rng.randint(1, 5000) for _ in range(3)})


def _splits(n, rng, count=3):
    """Ways to deliver n inputs: all at once, random cuts with zero-length pushes in between; always followed by a final empty `end` push,
    and once more with `end` on the last data push."""
    out = [([n], False), ([n], True)]
    for _ in range(count):
        cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(1, 6)))
        parts = [b - a for a, b in zip([0] + cuts, cuts + [n])]
        parts.insert(rng.randint(0, len(parts)), 0)
        out.append((parts, rng.random() < 0.5))
    return out


def _run(geo, parts, end_on_last):
    """Push `parts`, checking every push; returns the descriptors."""
    up, down, half_len, K = geo
    state = ResampleState()
    pushes = [(m, end_on_last and i == len(parts) - 1) for i, m in enumerate(parts)] + ([] if end_on_last else [(0, True)])
    n = sum(parts)
    seen = done = 0
    out = []
    for m, end in pushes:
        push, after = resample_advance(state, m, end, geo)
        assert isinstance(push, ResamplePush) and push.held == state.held and push.take == m
        assert push.count >= 0 and 0 <= push.keep <= K - 1 and push.keep <= push.held + push.take
        assert 0 <= push.q0 < K * up
        assert push.q0 == done * down + half_len - (seen - state.held) * up
        seen += m
        first = seen - m - state.held  # the stream's input at row position 0
        for j in (range(push.count) if push.count < 64 else (0, 1, push.count // 2, push.count - 2, push.count - 1)):
            q = push.q0 + j * down
            assert (q // up + first, q % up) == (geo.newest(done + j), ((done + j) * down + half_len) % up)  # the device's view is the formula's
            assert q // up - (K - 1) >= 0 or first == 0  # nothing is needed that the stream no longer holds
            if not end:
                assert geo.newest(done + j) < seen, "an output was emitted before its newest input existed"
        done += push.count
        if end:
            assert after == ResampleState() and done == geo.length(n) and seen == n
        else:
            assert after == ResampleState(push.keep, seen, done)
            assert geo.newest(done) >= seen, "an output whose newest input exists was held back"
            assert seen - after.held <= max(0, geo.newest(done) - (K - 1)), "the next output's oldest input was dropped"
        out.append(push)
        state = after
    return out


@pytest.mark.parametrize("orig,target", PAIRS)
def test_emitted_ranges_tile_the_output_of_any_split(orig, target):
    geo = resample_geometry(orig, target)
    lib = _capi.load_library()
    assert lib.l3ac_resample_stream_state(orig, target) == round4(geo.K - 1)
    rng = random.Random(orig * 31 + target)
    for n in _lengths(geo, rng):
        assert geo.length(n) == l3ac_amd.resample_length(orig, target, n)
        for parts, end_on_last in _splits(n, rng):
            pushes = _run(geo, parts, end_on_last)
            assert sum(p.count for p in pushes) == geo.length(n), (n, parts, end_on_last)


def test_equal_rates_pass_through_without_delay():
    geo = resample_geometry(*EQUAL)
    assert geo.up == geo.down == 1
    state = ResampleState()
    for m, end in ((5, False), (0, False), (7, False), (3, True)):
        push, state = resample_advance(state, m, end, geo)
        assert (push.count, push.held, push.keep) == (m, 0, 0) and 0 <= push.q0 < geo.K * geo.up
    assert state == ResampleState()
    assert l3ac_amd.stream_resampler(2, *EQUAL).delay == 0.0
    assert l3ac_amd.stream_resampler(2, 48000, 16000).delay == 30.0 and l3ac_amd.stream_resampler(2, 44100, 16000).delay == 4410 / 160


@pytest.mark.parametrize("orig,target", PAIRS)
def test_descriptors_do_not_depend_on_the_age_of_a_stream(orig, target):
    geo = resample_geometry(orig, target)
    rng = random.Random(orig + target)
    c = 2 ** 40
    state = ResampleState()
    warm = geo.K + geo.half_len // geo.up + 1  # inputs after which neither max(0, ...) of the geometry binds: (N, E) -> (N + c down, E + c up) is then a state too
    for _ in range(16):
        if state.seen < warm:  # a young stream (at first, and after every end) has no older twin
            _, state = resample_advance(state, warm, False, geo)
        old =ResampleState(state.held, state.seen + c * geo.down, state.emitted + c * geo.up)
        m, end = rng.choice((0, 1, geo.down, rng.randint(0, 3000))), rng.random() < 0.1
        push, after = resample_advance(state, m, end, geo)
        push_old, after_old = resample_advance(old, m, end, geo)
        assert push_old == push
        assert after_old == (ResampleState() if end else ResampleState(after.held, after.seen + c * geo.down, after.emitted + c * geo.up))
        assert all(-2 ** 31 <= v < 2 ** 31 for v in push_old)
        state = after


def test_geometry_refuses_bad_arguments():
    with pytest.raises(ValueError):
        resample_advance(ResampleState(), -1, False, resample_geometry(48000, 16000))
    for rates in ((0, 16000), (16000, -1)):
        with pytest.raises(ValueError):
            resample_geometry(*rates)


def test_header_and_binding_agree_on_the_new_entries():
    header = (REPO / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5
    lib = _capi.load_library()
    m = re.search(r"typedef struct l3ac_resample_stream_desc \{(.*?)\} l3ac_resample_stream_desc;", header, re.S)
    fields = re.findall(r"\b(int32_t|int64_t)\s+(\w+);", m.group(1))
    assert fields == [({ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t"}[t], n) for n, t in _capi.ResampleStreamDesc._fields_]
    assert ctypes.sizeof(_capi.ResampleStreamDesc) == 24
    for name in ("StreamResampler", "stream_resampler"):
        assert name in l3ac_amd.__all__ and hasattr(l3ac_amd, name)
    from l3ac_amd import build
    assert "kernels/resample_stream.hip" in build.SOURCES
    assert lib.l3ac_resample_stream_state(48000, 16000) == 60 and lib.l3ac_resample_stream_state(48000, 8000) == 120
    assert lib.l3ac_resample_stream_state(16000, 16001) == -1 and b"1024" in lib.l3ac_last_error()


def test_the_launch_entry_checks_its_descriptors_before_any_launch():
    """Null stream, bogus (never dereferenced) device pointers: the host-side checks refuse first."""
    lib = _capi.load_library()
    a, b, f, bank, y = (ctypes.c_void_p(1 << k) for k in (20, 24, 28, 30, 32))
    geo = resample_geometry(48000, 16000)
    sf = round4(geo.K - 1)

    def call(rows, state_in=a, state_out=b, streams=2, stride=sf, fresh=f, frames=100, rates=(48000, 16000), bank=bank, out=y, out_frames=40,
             out_stride=40):
        desc = (_capi.ResampleStreamDesc * len(rows))(*[_capi.ResampleStreamDesc(*r) for r in rows])
        return lib.l3ac_resample_stream(state_in, state_out, streams, stride, fresh, frames, frames, rates[0], rates[1], bank, desc, len(rows), out,
                                        out_frames, out_stride, None)
    #      slot held take count keep q0
    good = (0, 60, 100, 33, 60, 30)
    assert call([(2,) + good[1:]]) == -1 and b"stream 2 of 2" in lib.l3ac_last_error()       # slot out of range
    assert call([(-1,) + good[1:]]) == -1
    assert call([(0, sf + 1, 100, 33, 60, 30)]) == -1 and b"state row" in lib.l3ac_last_error()  # holds more than a state row
    assert call([(0, 60, 101, 33, 60, 30)]) == -1 and b"new frames" in lib.l3ac_last_error()     # takes 101 of 100 new frames
    assert call([good], fresh=None) == -1                                                       # ... from nowhere
    assert call([(0, 60, 100, 41, 60, 30)]) == -1 and b"emits 41" in lib.l3ac_last_error()       # 41 outputs into rows of 40
    assert call([(0, 60, 100, 33, 61, 30)]) == -1                                               # keeps 61 in a state row of 60
    assert call([(0, 3, 2, 0, 6, 30)]) == -1 and b"keeps 6 of 3 + 2" in lib.l3ac_last_error()    # keeps more than there is
    assert call([(0, 60, 100, 33, 60, -1)]) == -1 and b"origin" in lib.l3ac_last_error()         # q0 below 0
    assert call([(0, 60, 100, 33, 60, geo.K * geo.up)]) == -1 and b"origin" in lib.l3ac_last_error()  # q0 at K up
    assert call([good, good]) == -1 and b"one stream" in lib.l3ac_last_error()                  # two descriptors for one stream
    assert call([good], state_out=a) == -1 and b"overlap" in lib.l3ac_last_error()              # next state on top of the state
    assert call([good], out=f) == -1 and b"overlap" in lib.l3ac_last_error()                    # output on top of the packet
    assert call([good], state_in=None) == -1 and call([good], bank=None) == -1 and call([good], out=None) == -1
    assert call([good], out_frames=41) == -1                                                    # out_frames above the stride
    assert call([], ) == -1 and call([good], streams=0) == -1
    assert call([good], rates=(16000, 16001)) == -1 and b"1024" in lib.l3ac_last_error()        # unsupported pair
    # equal rates: a pass-through has no state and emits what it takes
    assert call([(0, 1, 40, 40, 0, 10)], rates=EQUAL) == -1 and call([(0, 0, 40, 39, 0, 10)], rates=EQUAL) == -1
    assert b"equal rates" in lib.l3ac_last_error()
    # nothing to emit and nothing to keep: accepted, and nothing is launched
    assert call([(0, 0, 0, 0, 0, 30)], out=None, out_frames=0, out_stride=1) == 0


def test_session_arguments_are_checked_before_a_device_is_needed():
    for kw in (dict(streams=0), dict(streams=-1), dict(streams=1.5), dict(streams=True)):
        with pytest.raises(ValueError):
            l3ac_amd.stream_resampler(orig_sr=48000, target_sr=16000, **kw)
    for rates in ((0, 16000), (16000, -5), (16000, 16001), (44100.5, 16000), (2 ** 33, 16000)):
        with pytest.raises(ValueError):
            l3ac_amd.stream_resampler(2, *rates)
    with pytest.raises(ValueError, match="1024"):
        l3ac_amd.stream_resampler(2, 16000, 16001)
    rs = l3ac_amd.stream_resampler(2, 48000, 16000)
    assert isinstance(rs, l3ac_amd.StreamResampler) and rs.states == [ResampleState()] * 2 and rs.state_frames == 60
    piece = torch.zeros(2, 100)
    for bad in (piece[0], torch.zeros(3, 100), piece[:, :, None], "abc", None):
        with pytest.raises(ValueError):
            rs.push(bad)
    for bad in ([-1, 5], [101, 5], [5], [5] * 3, [1.5, 5], "ab"):
        with pytest.raises(ValueError):
            rs.push(piece, lengths=bad)
    with pytest.raises(ValueError):
        rs.push(piece, end=[True])
    with pytest.raises(RuntimeError, match="is on cpu"):
        rs.push(piece, lengths=[100, 3], end=[False, True])
    assert rs.states == [ResampleState()] * 2
    with pytest.raises(ValueError):
        rs.reset(streams=2)
    rs.reset(streams=[1])
    rs.reset()
    with pytest.raises(TypeError):
        rs.push(piece, sample_rate=48000)
