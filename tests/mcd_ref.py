"""The fp64 oracle of the mel-cepstral distortion with DTW alignment, in NumPy, written from the specification
alone: the DCT design, the cepstra as the specification's fp32 fmaf chain (`chain_form`) and in fp64 with the sum of absolute products
beside them, the frame distance, the dynamic programme walked by anti-diagonals, the backtrace with the specification's tie order, a
brute-force minimum over all monotone paths for tiny matrices, and the suite's inputs."""
import functools
import math

import numpy as np

from tests.align_ref import fma32

U32 = 2.0 ** -24  # fp32 unit roundoff
U64 = 2.0 ** -53
MAX_FRAMES, MAX_DIM, MAX_COEFFS = 4096, 64, 64
MCD_SCALE = 5.0 * math.sqrt(2.0)


# ---- cepstra ------------------------------------------------------------------------------------------------------------------------------------
def dct_design(n_mels, n_coeffs):
    """D [n_coeffs + 1][n_mels] in fp64: D[0][m] = sqrt(1 / M), D[q][m] = sqrt(2 / M) cos(pi q (2m + 1) / (2M)), the phase q (2m + 1)
    reduced mod 4M in integers."""
    m = np.arange(n_mels)
    d = np.empty((n_coeffs + 1, n_mels))
    d[0] = math.sqrt(1.0 / n_mels)
    for q in range(1, n_coeffs + 1):
        r = (q * (2 * m + 1)) % (4 * n_mels)
        d[q] = math.sqrt(2.0 / n_mels) * np.cos(math.pi * r.astype(np.float64) / (2.0 * n_mels))
    return d


def chain_form(cells, table):
    """The specification's arithmetic itself: c[f][q] as one fp32 fmaf chain over m = 0 .. M - 1 in increasing m from +0, on fp32 cells
    [F][M] and the fp32 table [K + 1][M] -> fp32 [F][K + 1].  The library's cepstra equal this bit for bit."""
    cells, table = np.asarray(cells, dtype=np.float32), np.asarray(table, dtype=np.float32)
    acc = np.zeros((cells.shape[0], table.shape[0]), dtype=np.float32)
    for m in range(cells.shape[1]):
        acc = fma32(np.broadcast_to(table[None, :, m], acc.shape), np.broadcast_to(cells[:, m, None], acc.shape), acc).astype(np.float32)
    return acc


def cepstra64(cells, table):
    """-> (c, A), each fp64 [F][K + 1]: c = sum_m D L and A = sum_m |D| |L| on the fp32 values."""
    cells, table = np.asarray(cells, dtype=np.float64), np.asarray(table, dtype=np.float64)
    return cells @ table.T, np.abs(cells) @ np.abs(table).T


def cepstra_bound(n_mels):
    """|c_library - c_fp64| <= this times A: an fp32 fmaf chain of M terms (M roundings, first order M u, with the second-order terms and
    the fp64 value's own rounding inside the + 2)."""
    return (n_mels + 2) * U32


# ---- frame distance and the dynamic programme -----------------------------------------------------------------------------------------------------
def delta(a, b):
    """delta(i, j) = sqrt(sum_q (a[i][q] - b[j][q])^2) in fp64 from the fp32 values: difference, square, sum in the order of q."""
    a, b = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    s = np.zeros((a.shape[0], b.shape[0]))
    for q in range(a.shape[1]):
        d = a[:, q, None] - b[None, :, q]
        s = s + d * d
    return np.sqrt(s)


def dp(dl):
    """The accumulation on a given delta matrix, walked by anti-diagonals -> (Dacc, choice): one fp64 addition per cell, the minimum over
    the predecessors inside the matrix, ties to the diagonal (0), then to (i - 1, j) (1), then to (i, j - 1) (2)."""
    dl = np.asarray(dl, dtype=np.float64)
    fa, fb = dl.shape
    acc = np.full((fa + 1, fb + 1), np.inf)  # acc[i + 1][j + 1] = Dacc[i][j]; the border stands for "outside"
    choice = np.zeros((fa, fb), dtype=np.uint8)
    for d in range(fa + fb - 1):
        i = np.arange(max(0, d - fb + 1), min(d, fa - 1) + 1)
        j = d - i
        best, c = acc[i, j].copy(), np.zeros(len(i), dtype=np.uint8)
        up, left = acc[i, j + 1], acc[i + 1, j]
        take = up < best
        best[take], c[take] = up[take], 1
        take = left < best
        best[take], c[take] = left[take], 2
        if d == 0:
            best[:] = 0.0  # Dacc[0][0] = delta(0, 0): 0 + x is x
        acc[i + 1, j + 1] = dl[i, j] + best
        choice[i, j] = c
    return acc[1:, 1:], choice


def backtrace(choice):
    """The path from (0, 0) forward, (P, 2) int: the stored choices followed from (Fa - 1, Fb - 1)."""
    i, j = choice.shape[0] - 1, choice.shape[1] - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        c = choice[i, j]
        if c == 0:
            i, j = i - 1, j - 1
        elif c == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return np.array(path[::-1], dtype=np.int64)


def dtw(dl):
    """-> dict(cost, path, path_length) on a given delta matrix."""
    acc, choice = dp(dl)
    path = backtrace(choice)
    return dict(cost=float(acc[-1, -1]), path=path, path_length=len(path), acc=acc)


def path_sum(dl, path):
    """The sequential fp64 sum of delta along a path, from (0, 0)."""
    s = np.float64(dl[path[0][0], path[0][1]])
    for i, j in path[1:]:
        s = s + dl[i, j]
    return float(s)


def diagonal(dl):
    """dtw=False: sum_f delta(f, f) in the order of f."""
    n = min(dl.shape)
    return path_sum(dl, [(f, f) for f in range(n)])


def brute_force(dl):
    """Every monotone path of a tiny matrix -> (cost, path) of the best one: the smallest sequential sum; among equals the path whose
    steps, read from the END, prefer the diagonal, then (i - 1, j), then (i, j - 1) — the order in which the backtrace meets them."""
    fa, fb = dl.shape
    best = None

    def walk(i, j, steps, cells):
        nonlocal best
        if i == 0 and j == 0:
            path = cells[::-1]
            key = (path_sum(dl, path), tuple(steps))
            if best is None or key < best[0]:
                best = (key, path)
            return
        if i > 0 and j > 0:
            walk(i - 1, j - 1, steps + [0], cells + [(i - 1, j - 1)])
        if i > 0:
            walk(i - 1, j, steps + [1], cells + [(i - 1, j)])
        if j > 0:
            walk(i, j - 1, steps + [2], cells + [(i, j - 1)])

    walk(fa - 1, fb - 1, [], [(fa - 1, fb - 1)])
    return best[0][0], np.array(best[1], dtype=np.int64)


def mcd_db(cost, steps):
    return (np.float64(cost) * MCD_SCALE) / np.float64(steps)


def padded_path(path, rows):
    out = np.full((rows, 2), -1, dtype=np.int32)
    out[:len(path)] = path
    return out


# ---- the suite's inputs ---------------------------------------------------------------------------------------------------------------------------
def gaussian(frames, dim, seed):
    return np.random.default_rng(seed).standard_normal((frames, dim)).astype(np.float32)


def integers(frames, dim, seed):
    """Integer-valued features in [-3, 3]: every delta^2 is an exact integer, and ties abound."""
    return np.random.default_rng(seed).integers(-3, 4, (frames, dim)).astype(np.float32)


def distinct_steps(frames, dim):
    """Integer-valued frames of which no two neighbours are equal: frame f is f in every coordinate."""
    return np.repeat(np.arange(frames, dtype=np.float32)[:, None], dim, axis=1)


def staircase(frames):
    """The path of a sequence against itself with every frame repeated twice: (f, 2f), (f, 2f + 1)."""
    return np.array([(f, 2 * f + k) for f in range(frames) for k in (0, 1)], dtype=np.int64)


FLOAT_SHAPES = ((2, 3), (63, 64), (65, 64), (257, 255), (1025, 300), (4096, 33), (33, 4096))
FLOAT_DIMS = (1, 13, 64)


@functools.lru_cache(maxsize=None)
def float_pair(fa, fb, dim):
    """Gaussian features, the second side a noisy resampling of the first so that the best path wanders.  Shared and never written to."""
    a = gaussian(fa, dim, 1000 + fa + dim)
    src = np.minimum((np.arange(fb) * fa) // fb, fa - 1)
    b = (a[src] + np.float32(0.5) * gaussian(fb, dim, 2000 + fb + dim)).astype(np.float32)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def speech_like(n, seed, fs=16000):
    """Harmonics of a gliding pitch under a slow envelope plus a little noise: every mel cell of a frame is well above the clamp."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t)
    phase = 2 * np.pi * np.cumsum(f0) / fs
    x = sum(np.sin(k * phase + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 40))
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 2.3 * t + 1.0)
    return (0.05 * env * x + 0.01 * rng.standard_normal(n)).astype(np.float32)
