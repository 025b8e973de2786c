"""Mel-cepstral distortion with DTW alignment without a GPU: the DCT table against its fp64 design, the oracle (tests/mcd_ref.py) against
brute force and on sequences whose path is known, every bad argument refused — through the ABI with pointers that are never dereferenced
and through Python on CPU tensors — before any device work, the exports and the header, and the scratch sizes at their edges."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import mcd_ref as R

C = _capi.C
EINVAL = -1


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,n_coeffs", [(4, 3), (40, 13), (80, 24), (255, 64), (256, 64), (2, 1)])
def test_dct_table_is_its_fp64_design_rounded_once(n_mels, n_coeffs):
    table = l3ac_amd.dct_table(n_mels, n_coeffs).numpy()
    design = R.dct_design(n_mels, n_coeffs)
    assert table.shape == (n_coeffs + 1, n_mels) and table.dtype == np.float32
    assert (np.abs(table.astype(np.float64) - design) <= np.spacing(np.abs(design).astype(np.float32)).astype(np.float64)).all()  # 1 fp32 ulp
    assert (table[0] == np.float32(np.sqrt(1.0 / n_mels))).all()
    gram = table.astype(np.float64) @ table.astype(np.float64).T
    assert np.abs(gram - np.eye(n_coeffs + 1)).max() <= 1e-6
    lib = _capi.load_library()
    assert lib.l3ac_dct_table(n_mels, n_coeffs, None, 0) == (n_coeffs + 1) * n_mels
    guard = np.full(8, 7.0, dtype=np.float32)
    assert lib.l3ac_dct_table(n_mels, n_coeffs, guard.ctypes.data, (n_coeffs + 1) * n_mels - 1) == (n_coeffs + 1) * n_mels and (guard == 7.0).all()  # too small: untouched


def test_dct_table_refuses_unsupported_parameters():
    lib = _capi.load_library()
    for n_mels, n_coeffs, word in ((40, 0, b"n_coeffs"), (40, 40, b"n_coeffs"), (40, -1, b"n_coeffs"), (256, 65, b"n_coeffs"), (1, 1, b"n_coeffs"),
                                   (0, 1, b"n_mels"), (257, 13, b"n_mels")):
        assert lib.l3ac_dct_table(n_mels, n_coeffs, None, 0) < 0 and word in lib.l3ac_last_error(), (n_mels, n_coeffs)
        with pytest.raises(ValueError):
            l3ac_amd.dct_table(n_mels, n_coeffs)


def test_chain_form_is_within_the_bound_of_the_fp64_cepstra():
    rng = np.random.default_rng(5)
    for n_mels, n_coeffs in ((4, 3), (40, 13), (255, 64)):
        cells = (-4.0 + 3.0 * rng.standard_normal((9, n_mels))).astype(np.float32)
        table = l3ac_amd.dct_table(n_mels, n_coeffs).numpy()
        c, a = R.cepstra64(cells, table)
        got = R.chain_form(cells, table)
        assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - c) <= R.cepstra_bound(n_mels) * a).all()
    assert np.array_equal(R.chain_form(np.zeros((3, 8), dtype=np.float32), l3ac_amd.dct_table(8, 3).numpy()), np.zeros((3, 4), dtype=np.float32))


# ---- the oracle's dynamic programme -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 5), (5, 4), (1, 6), (6, 1)])
def test_dp_is_the_brute_force_minimum_on_random_matrices(shape):
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    for _ in range(8):
        dl = np.abs(rng.standard_normal(shape))
        got = R.dtw(dl)
        cost, path = R.brute_force(dl)
        assert got["cost"] == cost and np.array_equal(got["path"], path)
        assert got["cost"] == R.path_sum(dl, got["path"])  # exactly the sequential sum along the returned path


@pytest.mark.parametrize("shape", [(4, 5), (5, 4), (1, 6), (6, 1), (3, 3)])
def test_tie_order_on_integer_matrices(shape):
    rng = np.random.default_rng(100 + shape[0] * 10 + shape[1])
    for hi in (1, 2, 3):  # 0/1 matrices are almost all ties
        for _ in range(6):
            dl = rng.integers(0, hi + 1, shape).astype(np.float64)
            got = R.dtw(dl)
            cost, path = R.brute_force(dl)
            assert got["cost"] == cost and np.array_equal(got["path"], path), dl
    got = R.dtw(np.zeros(shape))  # every cell a tie: the diagonal while both indices last, then along the edge
    i, j = shape[0] - 1, shape[1] - 1
    want = [(i, j)]
    while i > 0 or j > 0:
        i, j = (i - 1, j - 1) if i > 0 and j > 0 else (i - 1, j) if i > 0 else (i, j - 1)
        want.append((i, j))
    assert got["cost"] == 0.0 and got["path"].tolist() == [list(p) for p in want[::-1]]


def test_path_length_bounds_and_the_sequential_sum():
    for fa, fb, dim in ((7, 19, 3), (64, 65, 1), (33, 12, 13)):
        a, b = R.float_pair(fa, fb, dim)
        dl = R.delta(a, b)
        got = R.dtw(dl)
        assert max(fa, fb) <= got["path_length"] <= fa + fb - 1
        assert got["path"][0].tolist() == [0, 0] and got["path"][-1].tolist() == [fa - 1, fb - 1]
        steps = np.diff(got["path"], axis=0)
        assert set(map(tuple, steps.tolist())) <= {(1, 1), (1, 0), (0, 1)}
        assert got["cost"] == R.path_sum(dl, got["path"])
        if fa == fb:
            assert got["cost"] <= R.diagonal(dl)


def test_a_sequence_against_itself_with_every_frame_repeated_twice():
    for frames, dim in ((1, 1), (5, 1), (9, 3)):
        x = R.distinct_steps(frames, dim)
        got = R.dtw(R.delta(x, np.repeat(x, 2, axis=0)))
        assert got["cost"] == 0.0 and got["path_length"] == 2 * frames and np.array_equal(got["path"], R.staircase(frames))
        got = R.dtw(R.delta(np.repeat(x, 2, axis=0), x))  # the mirror: the first tie goes to (i - 1, j)
        assert got["cost"] == 0.0 and np.array_equal(got["path"], R.staircase(frames)[:, ::-1])


def test_delta_is_the_ordered_fp64_form():
    a, b = R.float_pair(6, 5, 13)
    dl = R.delta(a, b)
    for i, j in ((0, 0), (5, 4), (3, 1)):
        s = np.float64(0.0)
        for q in range(13):
            d = np.float64(a[i, q]) - np.float64(b[j, q])
            s = s + d * d
        assert dl[i, j] == np.sqrt(s)
    assert R.mcd_db(3.0, 2) == (3.0 * (5.0 * np.sqrt(2.0))) / 2.0


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def dtw_scratch(batch, fa, fb):
    return _capi.load_library().l3ac_dtw_scratch_bytes(batch, fa, fb)


def test_scratch_sizes_at_their_edges():
    lens = lambda b: 256 * -(-4 * b // 256)
    up = lambda v: 256 * -(-v // 256)
    for b, fa, fb in ((1, 1, 1), (1, 16, 16), (1, 16, 17), (64, 1, 1), (65, 3, 5), (3, 4096, 4096), (65535, 4096, 4096), (2, 4096, 1), (2, 1, 4096)):
        assert dtw_scratch(b, fa, fb) == 2 * lens(b) + up(b * fa * fb), (b, fa, fb)
    assert dtw_scratch(1, 1, 1) == 768 and dtw_scratch(1, 16, 16) == 768 and dtw_scratch(1, 16, 17) == 1024 and dtw_scratch(65, 1, 1) == 1280
    lib = _capi.load_library()
    for bad, word in (((0, 5, 5), b"batch"), ((65536, 5, 5), b"batch"), ((-1, 5, 5), b"batch"), ((2, 0, 5), b"max_frames_a"), ((2, 4097, 5), b"max_frames_a"),
                      ((2, 5, 0), b"max_frames_b"), ((2, 5, 4097), b"max_frames_b"), ((2, -3, 5), b"max_frames_a")):
        assert dtw_scratch(*bad) < 0 and word in lib.l3ac_last_error(), bad
    mel = lambda b, t, n_fft, hop, m: lib.l3ac_mel_scratch_bytes(b, t, n_fft, hop, m)
    for b, t, n_fft, hop, m, k in ((1, 1, 16, 4, 4, 3), (1, 8000, 512, 160, 40, 13), (3, 20000, 512, 160, 255, 64), (65, 9, 16, 4, 4, 1)):
        want = lens(b) + up(4 * b * (1 + t // hop) * m) + mel(b, t, n_fft, hop, m)
        assert lib.l3ac_mfcc_scratch_bytes(b, t, n_fft, hop, m, k) == want, (b, t, n_fft, hop, m, k)
    for bad, word in (((1, 100, 512, 160, 40, 40), b"n_coeffs"), ((1, 100, 512, 160, 40, 0), b"n_coeffs"), ((1, 100, 512, 160, 256, 65), b"n_coeffs"),
                      ((1, 100, 500, 160, 40, 13), b"n_fft"), ((1, 100, 512, 162, 40, 13), b"hop"), ((0, 100, 512, 160, 40, 13), b"batch"),
                      ((1, 0, 512, 160, 40, 13), b"samples"), ((1, 100, 512, 160, 257, 13), b"n_mels")):
        assert lib.l3ac_mfcc_scratch_bytes(*bad) < 0 and word in lib.l3ac_last_error(), bad


def test_bad_arguments_are_refused_by_the_abi():
    lib = _capi.load_library()
    fake, fa, fb, dim = 4096, 300, 280, 13
    need = dtw_scratch(2, fa, fb)
    ok_a, ok_b = (C.c_int32 * 2)(300, 5), (C.c_int32 * 2)(280, 1)

    def dtw(a=fake, afs=dim + 1, ars=fa * (dim + 1), b=fake, bfs=dim, brs=fb * dim, batch=2, dim=dim, fa=fa, fb=fb, la=ok_a, lb=ok_b, diagonal=0,
            cost=fake, steps=fake, path=None, delta=None, scratch=fake, nbytes=need):
        return lib.l3ac_dtw(a, afs, ars, b, bfs, brs, batch, dim, fa, fb, la, lb, diagonal, cost, steps, path, delta, scratch, nbytes, None)

    # refused on the arguments alone, whatever the pointers: nothing is launched or dereferenced
    for kw in (dict(batch=0), dict(batch=65536), dict(dim=0), dict(dim=65), dict(fa=0), dict(fa=4097), dict(fb=0), dict(fb=4097),
               dict(la=(C.c_int32 * 2)(0, 5)), dict(la=(C.c_int32 * 2)(301, 5)), dict(lb=(C.c_int32 * 2)(280, 0)), dict(lb=(C.c_int32 * 2)(281, 1)),
               dict(la=(C.c_int32 * 2)(-4, 5)), dict(afs=dim - 1), dict(bfs=dim - 1), dict(afs=-1), dict(ars=(fa - 1) * (dim + 1) + dim - 1),
               dict(brs=(fb - 1) * dim + dim - 1), dict(ars=-5), dict(a=None), dict(b=None), dict(cost=None), dict(steps=None), dict(scratch=None),
               dict(scratch=fake + 128), dict(nbytes=need - 1), dict(nbytes=0), dict(diagonal=1), dict(diagonal=1, la=None, lb=None),
               dict(diagonal=1, fb=fa, la=(C.c_int32 * 2)(300, 5), lb=(C.c_int32 * 2)(300, 4))):
        assert dtw(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert dtw(fa=4097) == EINVAL and b"max_frames_a" in lib.l3ac_last_error()
    assert dtw(dim=65) == EINVAL and b"dim" in lib.l3ac_last_error()
    assert dtw(nbytes=need - 1) == EINVAL and b"scratch" in lib.l3ac_last_error()
    assert dtw(bfs=dim - 1) == EINVAL and b"stride" in lib.l3ac_last_error()
    assert dtw(lb=(C.c_int32 * 2)(280, -1)) == EINVAL and b"frames_b[1]" in lib.l3ac_last_error()
    assert dtw(diagonal=1) == EINVAL and b"diagonal_only" in lib.l3ac_last_error()
    assert dtw(nbytes=dtw_scratch(2, fa, fb - 1)) == EINVAL  # the scratch of another shape

    t, n_fft, hop, m, k = 8000, 512, 160, 40, 13
    need = lib.l3ac_mfcc_scratch_bytes(2, t, n_fft, hop, m, k)
    ok = (C.c_int32 * 2)(300, t)

    def mfcc(audio=fake, batch=2, t=t, stride=t, lens=ok, n_fft=n_fft, hop=hop, basis=fake, weights=fake, m=m, dct=fake, k=k, out=fake, scratch=fake,
             nbytes=need):
        return lib.l3ac_mfcc(audio, batch, t, stride, lens, n_fft, hop, basis, weights, m, dct, k, out, scratch, nbytes, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(t=0), dict(stride=t - 1), dict(lens=(C.c_int32 * 2)(0, t)), dict(lens=(C.c_int32 * 2)(300, t + 1)),
               dict(n_fft=500), dict(n_fft=8), dict(hop=0), dict(hop=162), dict(hop=516), dict(m=0), dict(m=257), dict(k=0), dict(k=m), dict(k=65, m=256),
               dict(audio=None), dict(basis=None), dict(weights=None), dict(dct=None), dict(out=None), dict(scratch=None), dict(scratch=fake + 128),
               dict(nbytes=need - 1), dict(nbytes=0)):
        assert mfcc(**kw) == EINVAL and lib.l3ac_last_error(), kw
    assert mfcc(k=m) == EINVAL and b"n_coeffs" in lib.l3ac_last_error()
    assert mfcc(nbytes=need - 1) == EINVAL and b"scratch" in lib.l3ac_last_error()
    assert mfcc(lens=(C.c_int32 * 2)(300, 0)) == EINVAL and b"samples[1]" in lib.l3ac_last_error()


def test_bad_arguments_raise_in_python_before_any_device_work():
    x, y = torch.zeros(2, 5000), torch.zeros(2, 6000)
    for kw in (dict(n_coeffs=40), dict(n_coeffs=0), dict(n_coeffs=65, n_mels=256), dict(n_mels=0), dict(n_mels=257), dict(n_fft=500), dict(hop=162),
               dict(sample_rate=0)):
        with pytest.raises(ValueError):  # the parameter first, on CPU tensors
            l3ac_amd.mfcc(x, **kw)
        with pytest.raises(ValueError):
            l3ac_amd.mcd(x, x, **kw)
    with pytest.raises(ValueError, match="n_coeffs"):
        l3ac_amd.mfcc(x, n_mels=24, n_coeffs=24)
    with pytest.raises(ValueError, match="dtw=False"):
        l3ac_amd.mcd(x, y, dtw=False)
    with pytest.raises(ValueError, match="dtw=False"):
        l3ac_amd.mcd(x, x, lengths=[5000, 400], estimate_lengths=[5000, 700], dtw=False)
    for kw in (dict(lengths=[0, 5]), dict(lengths=[5001, 5]), dict(lengths=[5]), dict(estimate_lengths=[6001, 5]), dict(estimate_lengths=[1, 2, 3])):
        with pytest.raises(ValueError, match="lengths"):
            l3ac_amd.mcd(x, y, **kw)
    with pytest.raises(ValueError, match="batch"):
        l3ac_amd.mcd(x, torch.zeros(3, 5000))
    with pytest.raises(ValueError, match="frames"):
        l3ac_amd.mcd(torch.zeros(1, 4096 * 160), torch.zeros(1, 100))  # 4097 frames
    a, b = torch.zeros(2, 30, 13), torch.zeros(2, 20, 13)
    for bad_a, bad_b, word in ((torch.zeros(1, 4097, 3), torch.zeros(1, 5, 3), "4097 frames"), (torch.zeros(1, 5, 3), torch.zeros(1, 4097, 3), "4097 frames"),
                               (torch.zeros(1, 5, 65), torch.zeros(1, 5, 65), "dim 65"), (a, torch.zeros(2, 20, 12), "differ"),
                               (a, torch.zeros(3, 20, 13), "differ"), (torch.zeros(30, 13), b, "tensor"), (a, None, "tensor"),
                               (torch.zeros(2, 0, 13), b, "frames"), (torch.zeros(2, 5, 0), torch.zeros(2, 5, 0), "dim")):
        with pytest.raises(ValueError, match=word):
            l3ac_amd.dtw(bad_a, bad_b)
    for kw in (dict(lengths_a=[0, 5]), dict(lengths_a=[31, 5]), dict(lengths_b=[21, 5]), dict(lengths_b=[5]), dict(lengths_a=[2.5, 5])):
        with pytest.raises(ValueError, match="lengths_"):
            l3ac_amd.dtw(a, b, **kw)
    with pytest.raises(ValueError, match="diagonal_only"):
        l3ac_amd.dtw(a, b, diagonal_only=True)
    with pytest.raises(ValueError, match="diagonal_only"):
        l3ac_amd.dtw(a, a, lengths_a=[30, 7], lengths_b=[30, 8], diagonal_only=True)
    for call in (lambda: l3ac_amd.mfcc(x), lambda: l3ac_amd.mfcc(x.numpy()), lambda: l3ac_amd.mfcc(x, lengths=[1, 5000]), lambda: l3ac_amd.dtw(a, b),
                 lambda: l3ac_amd.dtw(a, a, diagonal_only=True), lambda: l3ac_amd.dtw(a, b, lengths_a=[30, 1], lengths_b=[1, 20], return_path=True),
                 lambda: l3ac_amd.mcd(x, y), lambda: l3ac_amd.mcd(x, x, dtw=False), lambda: l3ac_amd.mcd(x, y, lengths=[1, 5000], return_path=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_exports_and_abi_version():
    for name in ("mfcc", "dtw", "mcd", "dct_table"):
        assert name in l3ac_amd.__all__ and callable(getattr(l3ac_amd, name))
    header = (Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h").read_text()
    assert re.search(r"#define\s+L3AC_ABI_VERSION\s+5\b", header) and _capi.ABI_VERSION == 5  # additive: the version stays
    lib = _capi.load_library()
    assert lib.l3ac_abi_version() == 5
    assert "DESIGN.md section 3.17" in header
    assert "256 ceil(batch max_frames_a max_frames_b /" in header  # the closed form of the DTW scratch is stated
    import inspect
    assert "mcd" in inspect.signature(l3ac_amd.L3AC.evaluate).parameters
