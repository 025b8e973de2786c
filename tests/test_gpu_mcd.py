"""Mel-cepstral distortion with DTW alignment on the MI355X (kernels/mcd.hip) against the fp64 oracle (tests/mcd_ref.py, DESIGN.md section
3.17): the cepstra bit for bit the specified fmaf chain on `log_mel`'s own cells and within the derived bound of the fp64 value, the DTW
exact on integer features, on Gaussian features its frame distances within (dim + 3) 2^-53 of the oracle's and its cost, path length
and path bit for bit the oracle's dynamic programme RUN ON THE LIBRARY'S OWN distance matrix, bit invariance over batch / row / strides /
scratch size / what lies after a pair's counts, `mcd` against the composed calls and on pairs whose answer is known, codec.evaluate
(mcd=True), and graph capture as the first DTW call of the process.

The dynamic programme is exact given the distance matrix — one fp64 addition per cell, a minimum with a stated tie order — so no case
needs a margin and none is filtered.  The figures measured on an MI355X are in the docstrings of the tests that print them."""
import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import mcd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 16000


def bits(t):
    """A device tensor as integers: NaN entries compare like any other."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def dev(*arrays):
    return torch.from_numpy(np.stack(arrays)).to(DEV)


def run(a, b, **kw):
    """The library on one pair alone -> numpy values: cost, path_length, path (P, 2), cost_matrix."""
    out = l3ac_amd.dtw(dev(a), dev(b), return_path=True, return_cost_matrix=True, **kw)
    fa, fb = len(a), len(b)
    assert set(out) == {"cost", "path_length", "path", "cost_matrix"} and all(v.is_cuda for v in out.values())
    assert out["cost"].dtype == out["cost_matrix"].dtype == torch.float64 and out["path_length"].dtype == out["path"].dtype == torch.int32
    assert out["cost"].shape == out["path_length"].shape == (1,) and out["path"].shape == (1, fa + fb - 1, 2) and out["cost_matrix"].shape == (1, fa, fb)
    steps = int(out["path_length"][0])
    path = out["path"][0].cpu().numpy()
    assert (path[steps:] == -1).all()
    return dict(cost=out["cost"][0].cpu().numpy(), path_length=steps, path=path[:steps].astype(np.int64), cost_matrix=out["cost_matrix"][0].cpu().numpy())


def check_against_own_matrix(g, fa, fb, name):
    """cost, path length and path are the oracle's dynamic programme on the library's own distance matrix, bit for bit."""
    want = R.dtw(g["cost_matrix"][:fa, :fb])
    assert g["path_length"] == want["path_length"] and np.array_equal(g["path"], want["path"]), name
    assert np.float64(want["cost"]).view(np.int64) == g["cost"].view(np.int64), (name, want["cost"], float(g["cost"]))
    assert max(fa, fb) <= g["path_length"] <= fa + fb - 1, name


# ---- 6. graph capture: FIRST in this file, no other file of the suite calls dtw -------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits_as_the_first_dtw_call():
    """There is no table to upload and the frame counts are kernel arguments: the very first call may be the captured one."""
    (a0, b0), (a1, b1) = R.float_pair(65, 64, 13), R.float_pair(63, 64, 13)
    a = torch.zeros(2, 65, 13, device=DEV)
    b = torch.zeros(2, 64, 13, device=DEV)
    a[0], b[0], a[1, :63], b[1] = (torch.from_numpy(np.array(v)).to(DEV) for v in (a0, b0, a1, b1))
    other = b.flip(1).contiguous()
    kw = dict(lengths_a=[65, 63], lengths_b=[64, 50], return_path=True, return_cost_matrix=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = l3ac_amd.dtw(a, b, **kw)
    graph.replay()
    torch.cuda.synchronize()
    eager = l3ac_amd.dtw(a, b, **kw)
    for k in eager:
        assert same(out[k], eager[k]), k
    want = R.dtw(R.delta(a1[:63], b1[:50]))
    assert int(eager["path_length"][1]) == want["path_length"] and abs(float(eager["cost"][1]) - want["cost"]) <= 1e-12 * want["cost"]
    b.copy_(other)  # the replay reads the tensors' current contents
    graph.replay()
    torch.cuda.synchronize()
    again = l3ac_amd.dtw(a, other, **kw)
    for k in again:
        assert same(out[k], again[k]), k
    assert not same(again["cost"], eager["cost"])


# ---- 1. cepstra -----------------------------------------------------------------------------------------------------------------------------------
def signal(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


CEPSTRA = {
    "one sample": (16, 4, 4, 3, [1]),
    "nine samples": (16, 4, 4, 3, [9]),
    "the defaults, half a second": (512, 160, 40, 13, [8000]),
    "255 filters, 64 coefficients": (512, 160, 255, 64, [2000]),
    "256 filters, 64 coefficients": (512, 160, 256, 64, [2000]),
    "ragged: 127, 128 and 129 frames": (512, 160, 40, 13, [126 * 160, 127 * 160 + 159, 128 * 160]),
}


@pytest.mark.parametrize("name", list(CEPSTRA))
def test_cepstra_are_the_specified_chain_on_log_mels_own_cells(name):
    """`mfcc` equals `chain_form` of `log_mel`'s output bit for bit and lies within (M + 2) 2^-24 sum_m |D| |L| of the fp64 cepstra of the
    same cells.  Measured on an MI355X, worst error / bound: 0.081 one sample, 0.185 nine samples, 0.125 the defaults and the ragged batch,
    0.053 and 0.040 at 255 and 256 filters with 64 coefficients."""
    n_fft, hop, n_mels, k, lens = CEPSTRA[name]
    t = max(lens) + (100 if len(lens) > 1 else 0)
    x = np.stack([signal(t, 70 + i) for i in range(len(lens))])
    ragged = len(lens) > 1
    if ragged:
        for i, n in enumerate(lens):
            x[i, n:] = 1e30  # what lies after a clip's length is not read
    kw = dict(sample_rate=SR, n_fft=n_fft, hop=hop, n_mels=n_mels)
    audio = torch.from_numpy(x).to(DEV)
    if ragged:
        got, frames = l3ac_amd.mfcc(audio, n_coeffs=k, lengths=lens, **kw)
        cells, frames_mel = l3ac_amd.log_mel(audio, lengths=lens, **kw)
        assert frames.tolist() == frames_mel.tolist() == [127, 128, 129]
    else:
        got, cells = l3ac_amd.mfcc(audio, n_coeffs=k, **kw), l3ac_amd.log_mel(audio, **kw)
        frames = torch.tensor([1 + lens[0] // hop])
    assert got.shape == (len(lens), 1 + t // hop, k + 1) and got.dtype == torch.float32 and got.is_cuda
    table = l3ac_amd.dct_table(n_mels, k).numpy()
    got, cells = got.cpu().numpy(), cells.cpu().numpy()
    worst = 0.0
    for i, f in enumerate(frames.tolist()):
        want = R.chain_form(cells[i, :f], table)
        assert np.array_equal(got[i, :f].view(np.int32), want.view(np.int32)), (name, i, np.argwhere(got[i, :f] != want)[:4].tolist())
        assert not got[i, f:].view(np.int32).any(), (name, i)  # exact zeros after the clip's own frames
        c, a = R.cepstra64(cells[i, :f], table)
        err = np.abs(got[i, :f].astype(np.float64) - c)
        assert (err <= R.cepstra_bound(n_mels) * a).all(), (name, i, float((err[a > 0] / (R.cepstra_bound(n_mels) * a[a > 0])).max()))
        worst = max(worst, float((err[a > 0] / (R.cepstra_bound(n_mels) * a[a > 0])).max()))
    print(f"\n[mcd] cepstra, {name}: worst |c - c_fp64| = {worst:.4f} of (M + 2) u sum |D| |L|")


def test_a_ragged_clip_of_the_cepstra_equals_the_clip_alone():
    n_fft, hop, n_mels, k, lens = CEPSTRA["ragged: 127, 128 and 129 frames"]
    x = np.stack([signal(max(lens) + 100, 70 + i) for i in range(3)])
    batch = x.copy()
    for i, n in enumerate(lens):
        batch[i, n:] = np.nan
    got, frames = l3ac_amd.mfcc(torch.from_numpy(batch).to(DEV), n_coeffs=k, lengths=lens, extra_scratch=0)
    for i, n in enumerate(lens):
        alone = l3ac_amd.mfcc(torch.from_numpy(x[i:i + 1, :n]).to(DEV), n_coeffs=k)
        assert same(got[i, :int(frames[i])], alone[0]), i


# ---- 2. exact DTW on integer-valued features ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3])
def test_exact_dtw_on_integer_features(dim):
    """Every delta^2 is a small integer: delta, cost, path length and path equal the oracle's exactly, ties included."""
    for fa, fb in ((1, 1), (1, 7), (7, 1), (64, 65)):
        a, b = R.integers(fa, dim, 10 * fa + dim), R.integers(fb, dim, 20 * fb + dim)
        g = run(a, b)
        want = R.dtw(R.delta(a, b))
        assert np.array_equal(g["cost_matrix"], R.delta(a, b)) and float(g["cost"]) == want["cost"], (fa, fb)
        assert g["path_length"] == want["path_length"] and np.array_equal(g["path"], want["path"]), (fa, fb)
    x = R.distinct_steps(33, dim)  # a sequence against itself with every frame repeated twice: zero cost along a staircase of ties
    g = run(x, np.repeat(x, 2, axis=0))
    assert float(g["cost"]) == 0.0 and g["path_length"] == 66 and np.array_equal(g["path"], R.staircase(33))
    g = run(np.repeat(x, 2, axis=0), x)
    assert float(g["cost"]) == 0.0 and np.array_equal(g["path"], R.staircase(33)[:, ::-1])
    for fa, fb in ((64, 65), (7, 1), (5, 5)):  # a constant sequence: every cell a tie
        g = run(np.full((fa, dim), 2.0, dtype=np.float32), np.full((fb, dim), 2.0, dtype=np.float32))
        want = R.dtw(np.zeros((fa, fb)))
        assert float(g["cost"]) == 0.0 and np.array_equal(g["path"], want["path"]) and not g["cost_matrix"].any(), (fa, fb)


# ---- 3. DTW on Gaussian features ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.FLOAT_DIMS)
@pytest.mark.parametrize("fa,fb", R.FLOAT_SHAPES)
def test_float_dtw(fa, fb, dim):
    """delta within (dim + 3) 2^-53 relative of the oracle's (loose enough for a square root one ulp off; measured on an MI355X: equal
    bit for bit in every case); cost, path length and path those of the oracle's programme on the library's own matrix."""
    a, b = R.float_pair(fa, fb, dim)
    name = (fa, fb, dim)
    g = run(a, b)
    dl = R.delta(a, b)
    err = np.abs(g["cost_matrix"] - dl)
    assert (err <= (dim + 3) * R.U64 * dl).all(), (name, float((err / dl).max() / R.U64))
    check_against_own_matrix(g, fa, fb, name)
    assert float(g["cost"]) == R.path_sum(g["cost_matrix"], g["path"])
    # frame f against frame f on the common prefix, and the warped cost never above it
    n = min(fa, fb)
    plain = run(a, b, lengths_a=[n], lengths_b=[n], diagonal_only=True)
    diag = plain["cost_matrix"][np.arange(n), np.arange(n)]
    assert (np.abs(diag - dl[np.arange(n), np.arange(n)]) <= (dim + 3) * R.U64 * diag).all(), name
    assert np.float64(R.diagonal(plain["cost_matrix"][:n, :n])).view(np.int64) == plain["cost"].view(np.int64), name
    assert plain["path_length"] == n and np.array_equal(plain["path"], np.stack([np.arange(n)] * 2, axis=1)), name
    warped = run(a, b, lengths_a=[n], lengths_b=[n])
    check_against_own_matrix(warped, n, n, name)
    assert float(warped["cost"]) <= float(plain["cost"]), name
    print(f"\n[mcd] dtw {fa} x {fb}, dim {dim}: worst |delta - delta_oracle| = {float((err / dl).max() / R.U64):.2f} x 2^-53 relative, "
          f"P = {g['path_length']}, cost {float(g['cost']):.6g} (diagonal on {n}: {float(plain['cost']):.6g}, warped {float(warped['cost']):.6g})")


# ---- 4. invariance --------------------------------------------------------------------------------------------------------------------------------
COUNTS = ((300, 280), (64, 200), (5, 1))
OUT = ("cost", "path_length", "path", "cost_matrix")


def ragged_batch():
    pairs = [R.float_pair(fa, fb, 14) for fa, fb in COUNTS]
    a = np.empty((3, 300, 14), dtype=np.float32)
    b = np.empty((3, 280, 14), dtype=np.float32)
    for i, ((fa, fb), (x, y)) in enumerate(zip(COUNTS, pairs)):
        for rows, v, f in ((a, x, fa), (b, y, fb)):
            rows[i, :f] = v
            rows[i, f:, 0::2] = np.nan  # what lies after a pair's counts is not read
            rows[i, f:, 1::2] = 1e30
    return pairs, torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)


def same_pair(out, row, alone, fa, fb):
    steps = int(alone["path_length"][0])
    assert same(out["cost"][row], alone["cost"][0]) and same(out["path_length"][row], alone["path_length"][0])
    assert same(out["path"][row, :steps], alone["path"][0, :steps]) and bool((out["path"][row, steps:] == -1).all())
    assert same(out["cost_matrix"][row, :fa, :fb], alone["cost_matrix"][0])
    assert not out["cost_matrix"][row, fa:].any() and not out["cost_matrix"][row, :, fb:].any()


def test_a_pair_does_not_depend_on_its_batch_row_strides_scratch_or_what_follows_it():
    pairs, a, b = ragged_batch()
    kw = dict(return_path=True, return_cost_matrix=True)
    # each pair alone, on the contiguous copy of its [..., 1:] view
    alone = [l3ac_amd.dtw(dev(np.ascontiguousarray(x[:, 1:])), dev(np.ascontiguousarray(y[:, 1:])), **kw) for x, y in pairs]
    for (fa, fb), (x, y), res in zip(COUNTS, pairs, alone):
        g = dict(cost=res["cost"][0].cpu().numpy(), path_length=int(res["path_length"][0]), cost_matrix=res["cost_matrix"][0].cpu().numpy())
        g["path"] = res["path"][0, :g["path_length"]].cpu().numpy().astype(np.int64)
        check_against_own_matrix(g, fa, fb, (fa, fb))
    need = _capi.load_library().l3ac_dtw_scratch_bytes(3, 300, 280)
    for order in ([0, 1, 2], [2, 1, 0]):
        va, vb = a[order][..., 1:], b[order][..., 1:]  # strided views: a frame stride of 14 under 13 features
        assert not va.is_contiguous() and va.stride(1) == 14
        for extra in (None, 0, need):  # the minimum scratch (twice: the default is the minimum) and twice the minimum
            out = l3ac_amd.dtw(va, vb, lengths_a=[COUNTS[i][0] for i in order], lengths_b=[COUNTS[i][1] for i in order], extra_scratch=extra, **kw)
            for row, i in enumerate(order):
                same_pair(out, row, alone[i], *COUNTS[i])
    # the view against its contiguous copy, whole batch
    lens = dict(lengths_a=[c[0] for c in COUNTS], lengths_b=[c[1] for c in COUNTS])
    view, copy = l3ac_amd.dtw(a[..., 1:], b[..., 1:], **lens, **kw), l3ac_amd.dtw(a[..., 1:].contiguous(), b[..., 1:].contiguous(), **lens, **kw)
    for k in OUT:
        assert same(view[k], copy[k]), k
    # NaN inside one pair leaves the others bit for bit, and its own path inside its matrix
    a[1, 10, 3] = np.nan
    out = l3ac_amd.dtw(a[..., 1:], b[..., 1:], **lens, **kw)
    for i in (0, 2):
        same_pair(out, i, alone[i], *COUNTS[i])
    steps = int(out["path_length"][1])
    path = out["path"][1].cpu().numpy()
    assert max(COUNTS[1]) <= steps <= sum(COUNTS[1]) - 1 and (path[steps:] == -1).all()
    assert (path[:steps] >= 0).all() and (path[:steps, 0] < COUNTS[1][0]).all() and (path[:steps, 1] < COUNTS[1][1]).all()
    assert path[0].tolist() == [0, 0] and path[steps - 1].tolist() == [COUNTS[1][0] - 1, COUNTS[1][1] - 1]
    assert set(map(tuple, np.diff(path[:steps], axis=0).tolist())) <= {(1, 1), (1, 0), (0, 1)}


# ---- 5. mcd ---------------------------------------------------------------------------------------------------------------------------------------
def stretched(x, factor):
    """x played `factor` times slower, by linear interpolation."""
    n = int(round(len(x) * factor))
    return np.interp(np.arange(n) / factor, np.arange(len(x)), x).astype(np.float32)


def test_mcd_of_a_clip_against_itself_is_zero_along_the_diagonal():
    x = dev(R.speech_like(8000, 1), R.speech_like(8000, 2))
    out = l3ac_amd.mcd(x, x, lengths=[8000, 5000], return_path=True)
    assert set(out) == {"mcd_db", "cost", "path_length", "frames_ref", "frames_est", "path"}
    assert out["mcd_db"].tolist() == [0.0, 0.0] and out["cost"].tolist() == [0.0, 0.0] and out["mcd_db"].dtype == torch.float64 and out["mcd_db"].is_cuda
    assert out["frames_ref"].tolist() == out["frames_est"].tolist() == out["path_length"].tolist() == [51, 32] and not out["frames_ref"].is_cuda
    path = out["path"].cpu().numpy()
    for i, f in enumerate((51, 32)):
        assert np.array_equal(path[i, :f], np.stack([np.arange(f)] * 2, axis=1)) and (path[i, f:] == -1).all()


def test_mcd_equals_the_composed_calls():
    ref = dev(R.speech_like(9000, 3), R.speech_like(9000, 4))
    est = dev(stretched(R.speech_like(9000, 3), 1.02)[:9100], R.speech_like(9100, 5))
    lens, est_lens = [9000, 7000], [9100, 6500]
    for kw in (dict(), dict(n_fft=256, hop=64, n_mels=20, n_coeffs=19)):
        out = l3ac_amd.mcd(ref, est, lengths=lens, estimate_lengths=est_lens, return_path=True, **kw)
        c_ref, f_ref = l3ac_amd.mfcc(ref, lengths=lens, **kw)
        c_est, f_est = l3ac_amd.mfcc(est, lengths=est_lens, **kw)
        d = l3ac_amd.dtw(c_ref[..., 1:], c_est[..., 1:], lengths_a=f_ref, lengths_b=f_est, return_path=True)
        assert same(out["cost"], d["cost"]) and same(out["path_length"], d["path_length"]) and same(out["path"], d["path"])
        assert same(out["mcd_db"], (d["cost"] * (5.0 * np.sqrt(2.0))) / d["path_length"].to(torch.float64))
        assert out["frames_ref"].tolist() == f_ref.tolist() and out["frames_est"].tolist() == f_est.tolist()
        assert (out["mcd_db"] > 0).all()
    plain = l3ac_amd.mcd(ref, est[:, :9000], lengths=lens, dtw=False)
    c_est, _ = l3ac_amd.mfcc(est[:, :9000], lengths=lens)
    c_ref, f_ref = l3ac_amd.mfcc(ref, lengths=lens)
    d = l3ac_amd.dtw(c_ref[..., 1:], c_est[..., 1:], lengths_a=f_ref, lengths_b=f_ref, diagonal_only=True)
    assert same(plain["cost"], d["cost"]) and plain["path_length"].tolist() == f_ref.tolist() and "path" not in plain
    assert same(plain["mcd_db"], (d["cost"] * (5.0 * np.sqrt(2.0))) / d["path_length"].to(torch.float64))


def test_dtw_absorbs_a_delay_and_a_drift_that_the_plain_value_pays_for():
    """The estimate is the reference 2 % slower and 3 hops late: along the DTW path the distortion is strictly below the frame-by-frame
    value on the common prefix."""
    hop, n = 160, 16000
    x = R.speech_like(n, 6)
    est = np.concatenate([np.zeros(3 * hop, dtype=np.float32), stretched(x, 1.02)])
    assert len(est) == 3 * hop + 16320
    warped = l3ac_amd.mcd(dev(x), dev(est))
    plain = l3ac_amd.mcd(dev(x), dev(est[:n]), dtw=False)
    assert warped["frames_ref"].tolist() == [101] and warped["frames_est"].tolist() == [1 + len(est) // hop] and plain["path_length"].tolist() == [101]
    print(f"\n[mcd] delayed and stretched: {float(warped['mcd_db'][0]):.3f} dB along the path, {float(plain['mcd_db'][0]):.3f} dB frame by frame")
    assert 0.0 < float(warped["mcd_db"][0]) < float(plain["mcd_db"][0])


def test_a_gain_of_two_costs_nothing_beyond_the_derived_bound():
    """estimate = 2 reference: every mel power is exactly 4 times the reference's, so every cell moves by log10 4 up to log10f's error, and
    the cepstra q >= 1 of a constant are zero up to the table's rounding.  Per frame and coefficient
        |c_est - c_ref| <= ((M + 2) u + 4 u) (A + A') + log10(4) |sum_m D[q][m]|,   A = sum_m |D||L|, A' the same on the estimate,
    ((M + 2) u: the two chains, bound of check 1; 4 u: log10f within 2 ulp on each side), delta(f, f) <= the root of the sum of squares over
    q, the DTW cost is at most the diagonal's and P at least F: mcd_db <= 5 sqrt(2) (1 + 2^-40) mean_f of that root.  Measured on an MI355X:
    4.2e-6 dB against a bound of 4.1e-4 dB."""
    n_mels, k, u = 40, 13, R.U32
    x = dev(R.speech_like(8000, 7))
    cells, cells2 = l3ac_amd.log_mel(x, SR, 512, 160, n_mels).cpu().numpy()[0], l3ac_amd.log_mel(2 * x, SR, 512, 160, n_mels).cpu().numpy()[0]
    assert (cells > -10.0).all() and (cells2 > -10.0).all()  # every cell above the clamp
    table = l3ac_amd.dct_table(n_mels, k).numpy().astype(np.float64)[1:]
    a, a2 = np.abs(cells.astype(np.float64)) @ np.abs(table).T, np.abs(cells2.astype(np.float64)) @ np.abs(table).T
    per_q = ((n_mels + 2) * u + 4 * u) * (a + a2) + np.log10(4.0) * np.abs(table.sum(axis=1))[None, :]
    bound = 5.0 * np.sqrt(2.0) * (1 + 2.0 ** -40) * float(np.sqrt((per_q ** 2).sum(axis=1)).mean())
    out = l3ac_amd.mcd(x, 2 * x)
    print(f"\n[mcd] a gain of two: {float(out['mcd_db'][0]):.3e} dB, bound {bound:.3e} dB")
    assert 0.0 <= float(out["mcd_db"][0]) <= bound and bound < 1e-3
    assert 0.0 <= float(l3ac_amd.mcd(x, 2 * x, dtw=False)["mcd_db"][0]) <= bound


@pytest.fixture(scope="module")
def codec():
    c = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    c.network.to(device=DEV).eval()
    return c


def test_codec_evaluate_with_mcd_equals_the_composed_calls(codec):
    lens = [16000, 14400]
    audio = torch.zeros(2, 16000)
    for i, n in enumerate(lens):
        audio[i, :n] = torch.from_numpy(R.speech_like(n, 600 + i))
    audio = audio.to(DEV)
    kw = dict(process_window=5400, prefix_tokens=3)  # several chunks each
    result = codec.evaluate(audio, lengths=lens, mcd=True, **kw)
    _, info = codec.encode_long(audio, lengths=lens, **kw)
    decoded = codec.decode_long(indices=info["indices"], lengths=info["lengths"], **kw)[:, :16000]
    warped = l3ac_amd.mcd(audio, decoded, sample_rate=codec.config.sample_rate, lengths=lens)
    plain = l3ac_amd.mcd(audio, decoded, sample_rate=codec.config.sample_rate, lengths=lens, dtw=False)
    assert same(result["mcd_db"], warped["mcd_db"]) and same(result["mcd_plain_db"], plain["mcd_db"]) and result["mcd_db"].is_cuda
    assert (result["mcd_db"] <= result["mcd_plain_db"]).all() and (result["mcd_db"] > 0).all()
    today = {"mel_distance", "per_scale", "mse", "snr_db", "si_sdr_db", "tokens", "bps"}
    assert set(result) == today | {"mcd_db", "mcd_plain_db"}
    assert set(codec.evaluate(audio, lengths=lens, **kw)) == today
    with pytest.raises(ValueError, match="4096 frames"):
        codec.evaluate(torch.zeros(1, 4096 * 160, device=DEV), mcd=True)


# ---- 6. capture of mcd, and the tables ----------------------------------------------------------------------------------------------------------------
def test_mcd_graph_capture_after_one_warm_up_call():
    ref = dev(R.speech_like(6000, 8), R.speech_like(6000, 9))
    est = dev(R.speech_like(6400, 10), stretched(R.speech_like(6000, 9), 1.1)[:6400])
    kw = dict(lengths=[6000, 4000], estimate_lengths=[6400, 4300], return_path=True)
    eager = l3ac_amd.mcd(ref, est, **kw)  # (the warm-up: uploads the tables)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = l3ac_amd.mcd(ref, est, **kw)
    est.mul_(0.5)  # the replay reads the tensors' current contents ...
    graph.replay()
    torch.cuda.synchronize()
    assert not same(out["cost"], eager["cost"])
    est.mul_(2.0)  # ... (a power of two: exactly undone)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("mcd_db", "cost", "path_length", "path"):
        assert same(out[k], eager[k]), k


def test_the_dct_table_refuses_to_upload_under_capture():
    x = torch.zeros(1, 800, device=DEV)
    l3ac_amd.mfcc(x)  # the default tables are warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside stream capture"):
        with torch.cuda.graph(graph):
            l3ac_amd.mfcc(x)
            l3ac_amd.mfcc(x, n_coeffs=7)  # an n_coeffs no other test uses: its table is not on the device, raises inside the capture
    torch.cuda.synchronize()
    assert l3ac_amd.mfcc(x, n_coeffs=7).shape == (1, 6, 8)  # eager, it works (and is warm from now on)
