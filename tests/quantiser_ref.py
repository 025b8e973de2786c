"""Plain CPU references for the quantiser kernels (kernels/fsq.hip): the FSQ forward pass in fp64 with the error the fp32 kernel is
entitled to, activations that sit on the rounding halves, and integer-grid data for the explicit-codebook search on which every
distance is exact, so the defined result is an integer argmin.  Shared by tests/test_quantiser_host.py (no GPU) and
tests/test_gpu_quantiser.py; nothing here touches a GPU or the library.

Error model of the forward pass (u = 2^-24, gamma_n = n u / (1 - n u), Higham's constant for n roundings in any order):
* latent d of a token is an fmaf chain over the lane's channels, at most six lane-sum additions and one bias addition: at most
  feat + 8 roundings whatever their order, so |lat_gpu - lat| <= e_lat = gamma_{feat+8} (|x| . |W_in|^T + |b_in|).
* s = (tanh(lat) + 1) / 2 (L - 1) is what gets rounded.  |tanh'| <= 1 and the halving give 0.5 e_lat; tanhf is documented at 2 ulp,
  2^-22 at values below 1; the "+ 1" and the "x 0.5" round once each at values below 2 (4 u covers both); the product with L - 1
  rounds once more at a value below L - 1 (u (L - 1)).  Hence
      tau = (L - 1) (0.5 e_lat + 2^-22 + 4 u) + u (L - 1):
  a level index may differ from round_half_even(s) only where s lies within tau of a half, and then by one step.
* everything after the rounding is exact IEEE arithmetic up to the output projection, an fmaf chain of D terms onto the bias:
  |q_feature - (q . W_out^T + b_out)| <= gamma_{D+1} (|b_out| + |q| . |W_out|^T) with q the kernel's own dequantised levels.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
LEVELS8 = (9, 7, 5, 3, 2, 4, 6, 8)  # levels[:D] for D = 1 .. 8: the largest codebook is 362 880 < 2^24
FEATS = (8, 16, 32, 64, 128, 256, 512)
AMBIGUOUS_CAP = 0.03  # share of tokens with any dimension inside its tau: a property of the inputs (worst 2.1 % at feat 512, D 8)


def gamma(n):
    return n * U / (1.0 - n * U)


def fsq_geometry(feat):
    """launch_fsq_t's rule: (channel quads per lane, lanes per token, tokens per 256-thread block)."""
    nv = 4 if feat >= 128 else 2
    lpt = feat // (4 * nv)
    return nv, lpt, 256 // lpt


def fsq_levels(d):
    return list(LEVELS8[:d])


def fsq_basis(levels):
    return torch.cumprod(torch.tensor([1] + list(levels)[:-1], dtype=torch.int64), 0)


def fsq_case(feat, d, n=4096):
    """The inputs of one forward case, drawn from one generator in a fixed order: w_in, b_in, x, then w_out, b_out."""
    g = torch.Generator().manual_seed(1000 * feat + d)
    bi, bo = 1.0 / math.sqrt(feat), 1.0 / math.sqrt(d)
    w_in = (torch.rand(d, feat, generator=g) * 2 - 1) * bi
    b_in = (torch.rand(d, generator=g) * 2 - 1) * bi
    x = torch.randn(n, feat, generator=g) * 2
    w_out = (torch.rand(feat, d, generator=g) * 2 - 1) * bo
    b_out = (torch.rand(feat, generator=g) * 2 - 1) * bo
    return {"feat": feat, "d": d, "n": n, "levels": fsq_levels(d), "w_in": w_in, "b_in": b_in, "x": x, "w_out": w_out, "b_out": b_out}


def fsq_forward_ref(x, w_in, b_in, levels):
    """fp64 forward pass up to the rounding, with the margins above.  Returns a dict of fp64 tensors: lat, e_lat [n][D], s (the value
    that is rounded), li (round_half_even(s)), tau, ambiguous (bool [n][D]: s within tau of a half)."""
    feat = x.shape[1]
    lat = x.double() @ w_in.double().T + b_in.double()
    e_lat = gamma(feat + 8) * (x.abs().double() @ w_in.abs().double().T + b_in.abs().double())
    lm1 = torch.tensor(list(levels), dtype=torch.float64) - 1
    s = (torch.tanh(lat) + 1) / 2 * lm1
    tau = lm1 * (0.5 * e_lat + 2.0 ** -22 + 4 * U) + U * lm1
    ambiguous = ((s - s.floor()) - 0.5).abs() <= tau
    return {"lat": lat, "e_lat": e_lat, "s": s, "li": torch.round(s), "tau": tau, "ambiguous": ambiguous}


def check_level_indices(li, ref, levels):
    """The rule of the margin: integers in [0, L - 1]; equal to round_half_even(s) outside tau, within one step inside.
    Returns (number of differing entries, ambiguous share of tokens); raises AssertionError otherwise."""
    li = li.double()
    lm1 = torch.tensor(list(levels), dtype=torch.float64) - 1
    assert torch.equal(li, li.round()) and (li >= 0).all() and (li <= lm1).all(), "level index outside [0, L - 1] or not an integer"
    diff = li - ref["li"]
    clear = ~ref["ambiguous"]
    assert (diff[clear] == 0).all(), (f"{int((diff[clear] != 0).sum())} level indices differ from round_half_even(s) outside the margin; "
                                      f"first at {torch.nonzero((diff != 0) & clear)[0].tolist()}")
    assert (diff.abs() <= 1).all(), "a level index inside the margin is off by more than one step"
    return int((diff != 0).sum()), ref["ambiguous"].any(1).double().mean().item()


def dequantise(li, levels):
    """q = li / (L - 1) * 2 - 1 in fp32, operation for operation what the kernel and the reference do (exact IEEE: the same bits)."""
    lm1 = torch.tensor(list(levels), dtype=torch.float32) - 1
    return (li.float() / lm1) * 2 - 1


def project_out_ref(q, w_out, b_out):
    """fp64 output projection of dequantised levels q [n][D] and its rounding bound gamma_{D+1} (|b_out| + |q| . |W_out|^T)."""
    out = q.double() @ w_out.double().T + b_out.double()
    bound = gamma(q.shape[1] + 1) * (q.abs().double() @ w_out.abs().double().T + b_out.abs().double())
    return out, bound


# ---- the rounding half ------------------------------------------------------------------------------------------------------------
def half_activations(levels):
    """Per dimension, fp32 activation values a with fl(a (L - 1)) exactly k + 0.5 for every k in [0, L - 2] (every fp32 value within
    8 ulp of (k + 0.5) / (L - 1) whose product lands on the half: for L - 1 not a power of two several do, or the nearest may not),
    the +-1 and +-2 ulp neighbours of the lowest and the highest of them, and 0, 1, 2^-30.  Returns (act [rows][D] fp32 — column d
    cycles through dimension d's values at a stride coprime to their number, so the dimensions meet in changing combinations —,
    ties [D] = how many k of dimension d have an exact half)."""
    cols, ties = [], []
    for L in levels:
        vals = [np.float32(0.0), np.float32(1.0), np.float32(2.0 ** -30)]
        n_tie = 0
        for k in range(L - 1):
            c = np.float32((k + 0.5) / (L - 1))
            cand = [c]
            lo = hi = c
            for _ in range(8):
                lo = np.nextafter(lo, np.float32(-1.0), dtype=np.float32)
                hi = np.nextafter(hi, np.float32(2.0), dtype=np.float32)
                cand += [lo, hi]
            on = sorted(a for a in cand if np.float32(a * np.float32(L - 1)) == np.float32(k + 0.5))
            n_tie += bool(on)
            ends = [on[0], on[-1]] if on else [c, c]
            vals += on
            for a, toward in ((ends[0], np.float32(-1.0)), (ends[1], np.float32(2.0))):
                for _ in range(2):
                    a = np.nextafter(a, toward, dtype=np.float32)
                    vals.append(a)
        cols.append(np.array(sorted(set(vals)), dtype=np.float32))
        ties.append(n_tie)
    rows = 3 * 257  # more than two token groups at feat = 8 (256 tokens per block)
    act = np.empty((rows, len(levels)), dtype=np.float32)
    for d, v in enumerate(cols):
        step = next(s for s in range(d + 1, d + 1 + len(v) + 1) if math.gcd(s, len(v)) == 1)
        act[:, d] = v[(np.arange(rows) * step + d) % len(v)]
    return torch.from_numpy(act), ties


# ---- explicit-codebook search on the integer grid ----------------------------------------------------------------------------------
VQ_KS = (1, 31, 32, 33, 63, 65, 511, 513, 1025, 2049)
VQ_NS_WAVE = (1, 3, 4, 5, 255, 5119)       # wavefront form
VQ_NS_MANY = (5120, 5121, 6200)            # screened form, and the direct-form scan with form = 1
VQ_WAVE_MAX_N = 5120                       # fsq.hip: the form switch
_ISO_FIRST = (-6, 0, 5)                    # first coordinates of the isolated codes
_REST_FIRST = (-8, -4, -3, -2, 2, 3, 7, 8)  # ... of all other codes: at least 2 away from every isolated one


def vq_cases(dim):
    """(k, n) pairs of one dimension: every k and every n at least once.  The pairing is rotated by the dimension so that over the
    eight dimensions every k meets most n; k = 1 (nothing to tie with) always meets a wavefront-form n; and every dimension gets
    the largest codebook with a screened-form n (65 tiles: several codebook slices in the screen and in the listed search)."""
    ns = list(VQ_NS_WAVE) + list(VQ_NS_MANY)
    ks = list(VQ_KS[1:])
    pairs = [(ks[i], ns[(i + dim) % len(ns)]) for i in range(len(ks))]
    pairs = [(1, VQ_NS_WAVE[dim % len(VQ_NS_WAVE)])] + pairs
    return pairs if (2049, 5121) in pairs else pairs + [(2049, 5121)]


def vq_block_of(c):
    """Which 16-code block of the screened form holds code c: accumulator register r of lane (col, h) of tile t is code
    32 t + 8 (r / 4) + 4 h + r % 4, and a lane's 16 registers are one block."""
    c = np.asarray(c)
    return 2 * (c // 32) + ((c % 32) // 4) % 2


def vq_grid_case(dim, k, n, seed):
    """Mixed data: integer codes in [-8, 8], queries on multiples of 0.5 in [-9, 9].  From k = 31 on, three codes are isolated (first
    coordinate -6 / 0 / 5, every other code's at least 2 away) and an eighth of the others are exact copies of codes elsewhere in the
    codebook, the last code a copy of the first.  Queries in turn: at or half a step beside an isolated code (one clear winner); on a
    code (copies tie); on the midpoint of two codes (bisector ties); anywhere on the grid."""
    g = np.random.default_rng(seed)
    cb = g.integers(-8, 9, size=(k, dim)).astype(np.float32)
    q = g.integers(-18, 19, size=(n, dim)).astype(np.float32) * 0.5
    if k >= 31:
        iso = np.array([k // 3, (2 * k) // 3, k - 3])
        rest = np.setdiff1d(np.arange(k), iso)
        cb[rest, 0] = g.choice(_REST_FIRST, size=rest.size)
        cb[iso, 0] = _ISO_FIRST
        inner = rest[(rest > 0) & (rest < k - 1)]
        dst = g.choice(inner, size=max(1, k // 8), replace=False)
        cb[dst] = cb[g.choice(np.setdiff1d(rest, dst), size=dst.size)]
        cb[k - 1] = cb[0]
        r = np.arange(n)
        t0, t1, t2 = r[r % 4 == 0], r[r % 4 == 1], r[r % 4 == 2]
        q[t0] = cb[iso[g.integers(0, 3, size=t0.size)]]
        q[t0, 0] += g.integers(-1, 2, size=t0.size) * 0.5
        q[t1] = cb[g.integers(0, k, size=t1.size)]
        q[t2] = 0.5 * (cb[g.integers(0, k, size=t2.size)] + cb[g.integers(0, k, size=t2.size)])
    return torch.from_numpy(q), torch.from_numpy(cb)


def vq_bisector_case(dim, k, n, seed):
    """Every query on a bisector of two codes that are not each other's copies, the pair in different blocks: codes on even
    coordinates, code i + k / 2 = code i + 2 e_0, the odd last code a copy of code 1; query = code i + e_0 — at distance 1 from
    exactly the codes equal to code i or to code i + 2 e_0 and further from every other code of the even lattice."""
    assert k // 2 >= 32
    g = np.random.default_rng(seed)
    half = k // 2
    a = g.integers(-4, 5, size=(half, dim)) * 2
    a[:, 0] = g.integers(-4, 4, size=half) * 2  # -8 .. 6: room for + 2
    b = a.copy()
    b[:, 0] += 2
    cb = np.concatenate([a, b] + ([a[1:2]] if k % 2 else [])).astype(np.float32)
    q = a[g.integers(0, half, size=n)].astype(np.float32)
    q[:, 0] += 1
    return torch.from_numpy(q), torch.from_numpy(cb)


def vq_exactness(q, cb):
    """The conditions under which every form of the search is exact in fp32 in any order, as a dict of booleans."""
    q2, c = q.double().numpy() * 2, cb.double().numpy()
    dim = q.shape[1]
    qd = dim * (np.abs(q.numpy()).max() + np.abs(cb.numpy()).max()) ** 2
    return {
        "codes are integers in [-8, 8]": bool((c == np.round(c)).all() and np.abs(c).max() <= 8),
        "queries are multiples of 0.5 in [-9, 9]": bool((q2 == np.round(q2)).all() and np.abs(q2).max() <= 18),
        "running sums stay below 2400 (multiples of 0.25 below 2^22: exact)": bool(dim * 17.0 ** 2 < 2400),
        "norms and scores are integers below 2^24": bool(dim * 64 + 2 * dim * 9 * 8 < 2 ** 24),
        "tol = 2^-17 Qd lies below the smallest non-zero gap 0.25": bool(2.0 ** -17 * qd + 1e-35 < 0.25),
    }


def vq_argmin_ref(q, cb, chunk=512):
    """The defined result on grid data: argmin_k of the int64 value sum_d (2 q_d - 2 c_d)^2, first occurrence = lowest index.
    Returns (idx int32 [n], across bool [n]: the minimum is attained in more than one 16-code block of the screened form — exactly
    the queries that form sends to the full direct-form search, the scores being exact too)."""
    q2 = np.round(q.double().numpy() * 2).astype(np.int64)
    c2 = np.round(cb.double().numpy() * 2).astype(np.int64)
    blk = vq_block_of(np.arange(c2.shape[0]))
    idx = np.empty(q2.shape[0], dtype=np.int32)
    across = np.empty(q2.shape[0], dtype=bool)
    for i in range(0, q2.shape[0], chunk):
        d = ((q2[i:i + chunk, None, :] - c2[None, :, :]) ** 2).sum(-1)
        idx[i:i + chunk] = np.argmin(d, axis=1)
        at_min = d == d.min(axis=1, keepdims=True)
        across[i:i + chunk] = np.where(at_min, blk, blk.max() + 1).min(1) != np.where(at_min, blk, -1).max(1)
    return torch.from_numpy(idx), torch.from_numpy(across)
