"""IIR filtering on the MI355X (kernels/iir.hip) against the CPU oracle (tests/iir_ref.py): the fp64 output bit for bit against the numpy
restatement of the three phases on the library's own M, M itself bit for bit against its restated design, the accuracy within 4 E of a
long-double filter (E = what scipy's fp64 filter costs the case), exact cases, the state hand-over between segments, clip isolation,
the streaming session against the one-shot call, graph capture as the first filtering call of the process, and the composed calls.

Filters, signal and lengths are tests/iir_ref.py's: F1 .. F5 over 1 .. 130 SEG + 7 samples, the longest three lengths crossing the
boundary between workgroups of 64 segments.  The capture test is the first of this file, and no other file filters."""
import functools

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _metric
from tests import iir_ref as R
from tests import loudness_ref as L
from tests import poison

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEG = R.SEG
IDENTITY = [[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def library_sos(name):
    order, fc, fs, kind = R.FILTERS[name]
    return l3ac_amd.butter_sos(order, fc, fs, kind)


@functools.lru_cache(maxsize=None)
def library_matrix(name):
    hi, lo = l3ac_amd.sosfilt_matrix(library_sos(name), DEV)
    return hi.cpu().numpy(), lo.cpu().numpy()


def padded(clips, fill=0.0):
    out = np.full((len(clips), max(len(c) for c in clips)), fill, dtype=np.float32)
    for i, c in enumerate(clips):
        out[i, :len(c)] = c
    return torch.from_numpy(out).to(DEV)


def alone(x, sos, dtype=torch.float64):
    """One clip by itself -> (n,) on the host."""
    return l3ac_amd.sosfilt(torch.from_numpy(np.ascontiguousarray(x))[None].to(DEV), sos, dtype=dtype)[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def outputs(name):
    """The filter's eight clips as one ragged batch -> the fp64 and the fp32 output on the host, once for the tests that read them."""
    clips = R.case_signals(name)
    x = padded(clips)
    lens = [len(c) for c in clips]
    y64 = l3ac_amd.sosfilt(x, library_sos(name), lengths=lens, dtype=torch.float64)
    y32 = l3ac_amd.sosfilt(x, library_sos(name), lengths=lens)
    assert y64.dtype == torch.float64 and y32.dtype == torch.float32 and y64.shape == y32.shape == x.shape
    return y64.cpu().numpy(), y32.cpu().numpy()


# ---- 7. capture: the first filtering call of the process -------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits_without_a_warm_up():
    """Nothing is uploaded and M is designed inside the call: the captured call may be the first one."""
    sos = l3ac_amd.butter_sos(*R.FILTERS["F3"])
    x = torch.from_numpy(np.stack([R.clip_signal(SEG + 1, 16000, seed=71), R.clip_signal(SEG + 1, 16000, seed=72)])).to(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = l3ac_amd.sosfilt(x, sos, dtype=torch.float64)
    graph.replay()
    torch.cuda.synchronize()
    eager = l3ac_amd.sosfilt(x, sos, dtype=torch.float64)
    assert same_bits(y, eager) and float(eager.abs().max()) > 0.1
    m_hi, m_lo = l3ac_amd.sosfilt_matrix(sos, DEV)
    assert same_bits(eager[1], R.restate(sos.numpy(), x[1].cpu().numpy(), m_hi.cpu().numpy(), m_lo.cpu().numpy()))
    saved = x.clone()
    x.mul_(0.5)  # the replay reads the tensor's current contents: halving is exact all the way through
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(y, eager * 0.5)
    x.copy_(saved)


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.FILTERS))
def test_matrix_is_its_restated_design_bit_for_bit(name):
    hi, lo = library_matrix(name)
    want_hi, want_lo = R.design_matrix(library_sos(name).numpy())
    assert hi.shape == want_hi.shape == (2 * len(library_sos(name)),) * 2
    assert same_bits(hi, want_hi) and same_bits(lo, want_lo)


@pytest.mark.parametrize("name", sorted(R.FILTERS))
def test_output_is_the_restatement_bit_for_bit(name):
    y64, y32 = outputs(name)
    hi, lo = library_matrix(name)
    sos = library_sos(name).numpy()
    for i, x in enumerate(R.case_signals(name)):
        n = len(x)
        want = R.restate(sos, x, hi, lo)
        assert same_bits(y64[i, :n], want), f"{name} n = {n}: {int((bits(y64[i, :n]) != bits(want)).sum())} of {n} samples differ"
        assert not y64[i, n:].any() and not y32[i, n:].any(), f"{name} n = {n}: not zero after the clip"
    assert same_bits(y32, y64.astype(np.float32))


# ---- 2. accuracy -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.FILTERS))
def test_output_is_within_four_times_what_fp64_costs(name):
    """Against the long-double loop, relative to its peak: the bound the restatement meets on the CPU (tests/test_iir_host.py).  Measured
    on an MI355X: the restatement's own figures, as the bits are its bits: E from 4.6e-17 (one sample) to 6.3e-13 (F2), the output
    between 0.53 E and 1.88 E (F2 at 64 SEG + 1 and 64 SEG - 1); exactly 1.00 E up to SEG + 1 samples."""
    y64, _ = outputs(name)
    sos = library_sos(name).numpy()
    for i, (x, (_, long, e)) in enumerate(zip(R.case_signals(name), R.case_references(name, sos.tobytes()))):
        assert e <= 1e-11, (name, len(x), e)
        err = R.error(y64[i, :len(x)], long)
        print(f"{name} n = {len(x)}: E = {e:.3g}, sosfilt {err:.3g} = {err / e:.2f} E")
        assert err <= 4 * e, (name, len(x), err, e)


# ---- 3. exact cases --------------------------------------------------------------------------------------------------------------------------
def test_exact_cases():
    n = 64 * SEG + 1
    x = R.clip_signal(n, 16000, seed=31)
    assert same_bits(alone(x, IDENTITY, torch.float32), x)
    assert same_bits(alone(x, IDENTITY), x.astype(np.float64))
    assert same_bits(alone(x, [[0.5, 0.0, 0.0, 1.0, 0.0, 0.0]], torch.float32), 0.5 * x)
    assert same_bits(alone(x, [[1.0, 0.0, 0.0, 2.0, 0.0, 0.0]], torch.float32), 0.5 * x)  # the division by a0
    delayed = np.concatenate([[0.0], x[:-1]]).astype(np.float32)
    assert same_bits(alone(np.abs(x), [[0.0, 1.0, 0.0, 1.0, 0.0, 0.0]], torch.float32), np.abs(delayed))  # (|x|: no -0 to lose in 0 x + s1)
    # a cascade of FIR sections with small integer coefficients on integers below 2^20: the integer convolution, exactly
    rng = np.random.default_rng(32)
    ints = rng.integers(-(1 << 20) + 1, 1 << 20, size=n)
    taps = ([1, 2, -1], [3, -1, 2], [1, 1, 1])
    want = ints.astype(np.int64)
    for b in taps:
        want = np.convolve(want, np.array(b, dtype=np.int64))[:n]
    got = alone(ints.astype(np.float32), [b + [1, 0, 0] for b in taps])
    assert np.abs(want).max() < 2.0 ** 53 and np.array_equal(got, want.astype(np.float64))
    assert np.count_nonzero(got[SEG:2 * SEG]) > SEG // 2


# ---- 4. hand-over ----------------------------------------------------------------------------------------------------------------------------
def test_state_is_handed_over_between_segments():
    sos = library_sos("F1").numpy()
    hi, lo = library_matrix("F1")
    n = 20 * SEG
    impulse = np.zeros(n, dtype=np.float32)
    impulse[SEG - 1] = 1.0  # the last sample of segment 0: everything later is the filter's tail, handed over as state
    got = alone(impulse, sos)
    ref = R.reference(sos, impulse)
    assert same_bits(got, R.restate(sos, impulse, hi, lo))
    assert not got[:SEG - 1].any() and np.all(got[ref != 0.0] != 0.0)
    assert all(np.count_nonzero(got[s * SEG:(s + 1) * SEG]) == SEG for s in range(1, 20)), "a later segment is silent: a zero state was handed over"
    long = R.reference_long(sos, impulse)
    e = R.error(ref, long)
    assert R.error(got, long) <= 4 * e
    dc = np.full(n, 0.25, dtype=np.float32)
    got = alone(dc, sos)
    long = R.reference_long(sos, dc)
    e = R.error(R.reference(sos, dc), long)
    assert same_bits(got, R.restate(sos, dc, hi, lo))
    assert e <= 1e-11 and R.error(got, long) <= 4 * e
    assert abs(got[-1]) < 1e-3 * abs(got[0])  # a high-pass: the step decays, as the oracle's does
    assert abs(float(long[-1])) < 1e-3 * abs(float(long[0]))


# ---- 5. isolation ----------------------------------------------------------------------------------------------------------------------------
def test_a_clips_bits_do_not_depend_on_the_batch():
    lens = [SEG + 1, 64 * SEG + 1, 1]
    clips = [R.clip_signal(n, 16000, seed=41 + i) for i, n in enumerate(lens)]
    for name in ("F1", "F5"):
        sos = library_sos(name)
        want = [alone(c, sos) for c in clips]
        x = padded(clips, fill=1e30)
        for i, n in enumerate(lens):
            x[i, n + 1::2] = float("nan")  # 1e30 and NaN after every length
        wide = torch.full((3, x.shape[1] + 37), float("nan"), dtype=torch.float32, device=DEV)
        wide[:, 5:5 + x.shape[1]] = x
        spaced = torch.full((6, x.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
        spaced[::2] = x
        need = _metric.lib_value("l3ac_sosfilt_scratch_bytes", 3, x.shape[1], len(sos))
        runs = {
            "ragged": l3ac_amd.sosfilt(x, sos, lengths=lens, dtype=torch.float64),
            "reversed": l3ac_amd.sosfilt(x.flip(0), sos, lengths=lens[::-1], dtype=torch.float64).flip(0),
            "wide rows": l3ac_amd.sosfilt(wide[:, 5:5 + x.shape[1]], sos, lengths=lens, dtype=torch.float64),
            "every other row": l3ac_amd.sosfilt(spaced[::2], sos, lengths=lens, dtype=torch.float64),
            "twice the scratch": l3ac_amd.sosfilt(x, sos, lengths=lens, dtype=torch.float64, extra_scratch=need),
        }
        for what, y in runs.items():
            y = y.cpu().numpy()
            for i, n in enumerate(lens):
                assert same_bits(y[i, :n], want[i]), f"{name} {what}: clip {i}"
                assert not y[i, n:].any(), f"{name} {what}: clip {i} is not zero after its length"
        # a NaN inside clip 1 leaves clips 0 and 2 as they are
        clean = padded(clips)
        for pattern in ("P2", "P3"):
            poison.twin_check(lambda b: l3ac_amd.sosfilt(b, sos, lengths=lens, dtype=torch.float64), clean, [1], pattern, extent=lens, what=name)


# ---- 6. streaming ----------------------------------------------------------------------------------------------------------------------------
STREAM_LENGTHS = (5 * SEG + 3, 2 * SEG, SEG - 1)


def split_a(n):
    """One sample at a time across the first boundary, pieces of SEG - 1 afterwards."""
    pieces = [min(n, SEG - 3)] + [1] * 6
    pieces = pieces if sum(pieces) <= n else [1] * n if n < 8 else [n - 6] + [1] * 6
    while sum(pieces) < n:
        pieces.append(min(SEG - 1, n - sum(pieces)))
    return pieces


def split_b(n):
    """Pieces of SEG + 1 with zero-length pushes between."""
    pieces = []
    while sum(pieces) < n:
        pieces += [min(SEG + 1, n - sum(pieces)), 0]
    return pieces


def split_c(n, seed):
    rng = np.random.default_rng(seed)
    pieces = []
    while sum(pieces) < n:
        pieces.append(int(min(rng.integers(0, 2 * SEG + 40), n - sum(pieces))))
    return pieces


def drive(flt, streams, plans):
    """Push stream i in the pieces plans[i] (a stream out of pieces brings nothing; it ends with its last piece) -> what each emitted.
    Rows are NaN after a stream's own samples of a push."""
    got = [[] for _ in streams]
    pos = [0] * len(streams)
    for p in range(max(len(plan) for plan in plans)):
        take = [plan[p] if p < len(plan) else 0 for plan in plans]
        end = [p == len(plan) - 1 for plan in plans]
        piece = torch.full((len(streams), max(take)), float("nan"), dtype=torch.float32)
        for i, x in enumerate(streams):
            piece[i, :take[i]] = torch.from_numpy(x[pos[i]:pos[i] + take[i]])
        y, n = flt.push(piece.to(DEV), lengths=take, end=end)
        assert y.shape == piece.shape and n.tolist() == take and n.dtype == torch.int32 and not n.is_cuda
        for i in range(len(streams)):
            got[i].append(y[i, :take[i]].cpu().numpy())
            assert not y[i, take[i]:].cpu().numpy().any(), "not zero after a stream's own samples"
            pos[i] += take[i]
    assert pos == [len(x) for x in streams]
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize("name", ["F1", "F5"])
def test_streams_add_up_to_the_one_shot_bits(name):
    sos = library_sos(name)
    streams = [R.clip_signal(n, 16000, seed=51 + i) for i, n in enumerate(STREAM_LENGTHS)]
    want = [alone(x, sos) for x in streams]
    splits = {"a": [split_a(len(x)) for x in streams], "b": [split_b(len(x)) for x in streams],
              "c": [split_c(len(x), 63 + i) for i, x in enumerate(streams)]}
    for what, plans in splits.items():
        assert len({len(plan) for plan in plans}) == 3  # the streams end at different pushes
        flt = l3ac_amd.stream_filter(3, sos, dtype=torch.float64)
        got = drive(flt, streams, plans)
        for i in range(3):
            assert same_bits(got[i], want[i]), f"{name} split {what}: stream {i}"
        assert flt.states == [(0, 0)] * 3
        # the slots are at rest: other streams through the same session, in another order
        again = drive(flt, streams[::-1], plans[::-1])
        for i in range(3):
            assert same_bits(again[i], want[2 - i]), f"{name} split {what}: stream {2 - i} in a reused slot"
    # a stream's bits with the others idle, and with the others absent
    idle = drive(l3ac_amd.stream_filter(3, sos, dtype=torch.float64), [streams[0], streams[1][:0], streams[2][:0]], [splits["c"][0], [0], [0]])
    assert same_bits(idle[0], want[0])
    lone = drive(l3ac_amd.stream_filter(1, sos, dtype=torch.float64), [streams[0]], [splits["a"][0]])
    assert same_bits(lone[0], want[0])
    # the default session emits fp32: the fp64 bits rounded once
    single = drive(l3ac_amd.stream_filter(1, sos), [streams[0]], [splits["b"][0]])
    assert single[0].dtype == np.float32 and same_bits(single[0], want[0].astype(np.float32))


@pytest.mark.parametrize("name", ["F1", "F5"])
def test_a_long_push_onto_a_stream_inside_a_segment(name):
    """A push that spans more than one workgroup of 64 segments onto streams at k = 7, SEG - 1 and 0: group 0 begins before the push
    (a negative first index), and where group 1 begins depends on k."""
    sos = library_sos(name)
    heads = (7, SEG - 1, 2 * SEG)
    n = 64 * SEG + 5
    streams = [R.clip_signal(h + n + 3, 16000, seed=101 + i) for i, h in enumerate(heads)]
    want = [alone(x, sos) for x in streams]
    got = drive(l3ac_amd.stream_filter(3, sos, dtype=torch.float64), streams, [[h, n, 3] for h in heads])
    for i in range(3):
        assert same_bits(got[i], want[i]), f"{name}: stream {i}, a push of {n} at k = {heads[i] % SEG}"


def test_reset_hands_a_slot_to_a_new_stream():
    """reset drops what a stream holds: the slot's next stream starts from rest, whatever the device rows hold (its first push is flagged
    fresh and reads none of them), and the streams that were not reset go on."""
    sos = library_sos("F1")
    old = np.stack([R.clip_signal(3 * SEG + 9, 16000, seed=111 + i) for i in range(3)])
    new = np.stack([R.clip_signal(2 * SEG + 5, 16000, seed=121 + i) for i in range(3)])
    want_new = l3ac_amd.sosfilt(torch.from_numpy(new).to(DEV), sos, dtype=torch.float64)
    flt = l3ac_amd.stream_filter(3, sos, dtype=torch.float64)
    y0, _ = flt.push(torch.from_numpy(old[:, :SEG + 9]).to(DEV))  # past the first boundary: a non-zero start pair, both running states
    assert flt.states == [(9, SEG + 9)] * 3
    flt.reset([0, 2])
    assert flt.states == [(0, 0), (9, SEG + 9), (0, 0)]
    piece = torch.from_numpy(np.stack([new[0, :2 * SEG], old[1, SEG + 9:3 * SEG + 9], new[2, :2 * SEG]])).to(DEV)
    y1, _ = flt.push(piece)
    assert same_bits(y1[0], want_new[0, :2 * SEG]) and same_bits(y1[2], want_new[2, :2 * SEG])
    assert same_bits(torch.cat([y0[1], y1[1]]), alone(old[1], sos))
    flt.reset()  # all of them, stream 1 at k = 9 with SEG of its samples behind it
    y2, _ = flt.push(torch.from_numpy(new).to(DEV), end=True)
    assert same_bits(y2, want_new) and flt.states == [(0, 0)] * 3
    with pytest.raises(ValueError):
        flt.reset(3)


def test_stream_errors_leave_the_session_unchanged():
    sos = library_sos("F1")
    x = np.stack([R.clip_signal(3 * SEG, 16000, seed=81), R.clip_signal(3 * SEG, 16000, seed=82)])
    want = l3ac_amd.sosfilt(torch.from_numpy(x).to(DEV), sos, dtype=torch.float64)
    flt = l3ac_amd.stream_filter(2, sos, dtype=torch.float64)
    piece = torch.from_numpy(x).to(DEV)
    y0, n0 = flt.push(piece[:, :SEG + 9])
    states = flt.states
    assert states == [(9, SEG + 9)] * 2 and n0.tolist() == [SEG + 9] * 2
    rest = piece[:, SEG + 9:]
    for bad in ([-1, 5], [2 * SEG, 5], [5], [1.5, 5], "ab"):
        with pytest.raises(ValueError):
            flt.push(rest, lengths=bad)
    with pytest.raises(ValueError):
        flt.push(rest, end=[True])
    with pytest.raises(ValueError):
        flt.push(rest[:1])
    with pytest.raises(RuntimeError):
        flt.push(rest.cpu())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="captured"):
            flt.push(rest)
        doubled = rest * 2  # (something to capture)
    assert flt.states == states
    y1, n1 = flt.push(rest, end=True)  # ... and goes on with the right bits
    assert same_bits(torch.cat([y0, y1], dim=1), want) and n1.tolist() == [2 * SEG - 9] * 2 and flt.states == [(0, 0)] * 2
    y2, _ = flt.push(torch.zeros(2, 0, device=DEV))  # a push of no samples at all
    assert y2.shape == (2, 0)


# ---- 8. composition --------------------------------------------------------------------------------------------------------------------------
def test_highpass_is_the_two_calls_composed():
    x = padded([R.clip_signal(3 * SEG + 5, 16000, seed=91), R.clip_signal(2 * SEG, 16000, seed=92)])
    lens = [3 * SEG + 5, 2 * SEG]
    assert same_bits(l3ac_amd.highpass(x, lengths=lens), l3ac_amd.sosfilt(x, l3ac_amd.butter_sos(4, 50.0, 16000, "highpass"), lengths=lens))
    assert same_bits(l3ac_amd.highpass(x, 300.0, 16000, 5), l3ac_amd.sosfilt(x, library_sos("F4")))
    assert l3ac_amd.highpass(x).dtype == torch.float32


def test_k_weighted_audio_carries_loudness_own_step_energies():
    """sosfilt(x, k_weighting_sos(fs)) squared and summed per 100 ms step on the host, in the order of the samples, against loudness' own
    step energies read back through the momentary row as its tests do (z_j = 10^((l_j + 0.691) / 10) = (e_j + .. + e_j+3) / (4 step)):
    within 4 E of the case, E = tests/loudness_ref.py's yardstick.  Not bit for bit: loudness segments by steps, this filter by SEG."""
    fs, step = 16000, 1600
    x = R.clip_signal(2 * fs, fs, seed=95)
    y = alone(x, l3ac_amd.k_weighting_sos(fs))
    e = L.step_energies(y, step)
    blocks = l3ac_amd.loudness_blocks(len(x), fs)
    mine = np.array([(((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / (4.0 * step) for j in range(blocks)]).astype(np.longdouble)
    momentary = l3ac_amd.loudness(torch.from_numpy(x)[None].to(DEV), fs, return_momentary=True)["momentary"][0].cpu().numpy()
    theirs = np.power(10.0, (momentary.astype(np.longdouble) + np.longdouble("0.691")) / 10)
    yard = L.yardstick(x, fs)
    err = float(np.max(np.abs(mine - theirs) / theirs))
    print(f"K-weighted z_j: E = {yard:.3g}, sosfilt against loudness {err:.3g} = {err / yard:.2f} E")
    assert blocks == 17 and yard > 0 and err <= 4 * yard
