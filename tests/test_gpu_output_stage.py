"""The decoder's output stage on the MI355X (kernels/last_block.hip) against an fp64 restatement of the oracle, per element within an
a-priori error bound: each LegacyUnit (l3ac_op_legacy_unit) and the head (l3ac_op_head) on their own, at the kernels' tile, halo, clip
and grid edges, on both routes (bf16x3: legacy_unit_split_kernel; exact fp32: legacy_unit_kernel), plus bit-exact clip isolation,
run-to-run and composition properties.

The bound.  u = 2^-24, gamma_n = n u / (1 - n u); every quantity below is evaluated in fp64 from the fp64 intermediates of the
reference (the folded fp32 weights and the fp32 input, widened).

* snake(v) = v + ia sin^2(alpha v), ia = 1 / (alpha + 1e-8).  The kernels evaluate fma(ia32, sin2(fl(alpha v)), v) with
  ia32 = 1.0f / (alpha + 1e-8f) (two fp32 roundings, network.hip) and the device sin^2, whose absolute error against fp64 at the fp32
  argument is eps_sin = 2e-7 (test_sin_squared_range asserts it for the scalar and the packed form).  Error terms: the product
  alpha v rounds (u |alpha v|, and |d sin^2 / du| <= 1, so <= u |alpha ia| |v| after the factor ia); sin^2 itself (|ia| eps_sin); ia32
  (2u |ia| sin^2); the fma (u (|v| + |ia| sin^2)).  With |alpha ia| <= 1 (asserted on the weights) the sum is
      e_snake(v) <= c1 u (|v| + |ia| sin^2(alpha v)) + |ia| eps_sin (1 + 4u),   c1 = 3,
  (the coefficient of |v| needs 2, that of |ia| sin^2 needs 3; the (1 + 4u) covers the product of the ia32 and sin^2 errors).
  Both routes evaluate snake in fp32 alike, so c1 is the same for both.  An error e already in v adds L e, L = 1 + max |alpha ia|
  (|d snake / dv| <= L <= 2).
* hidden h = b1 + W1 (*)_dil s:  e_h <= g_h (|b1| + |W1| (*) |s|) + |W1| (*) e_snake(x).
  Exact route: fp32 MFMA (v_mfma_f32_32x32x2_f32) accumulation of 7C products onto the bias: the classical dot-product bound
  gamma_n with n = 7C + 1 (k = 1: the bias is the first term; zero-padded products add exactly).
  bf16x3 route: every product a w is six plane products a_i w_j, each exact in fp32, and the three dropped cross
  products are <= 2^-24 |a w| together; sum_{i+j<=2} |a_i w_j| <= (1 + 2^-7)^2 |a| |w|.  Nothing is assumed about how a bf16 MFMA
  adds its 32 products: at most one fp32 rounding per plane product added (a sequential chain is the worst case), so 42C roundings
  plus the dropped terms: g_h = (1 + 2^-5) gamma_{42C + 2} (k = 35C + 2 in the gamma_{7C+k} form).
* s2 = snake(h):  e_s2 <= L e_h + e_snake(h).
* y = x + b2 + W2 s2:  e_y <= g_y (|x| + |b2| + |W2| |s2|) + |W2| e_s2 (+ e_x, the error already in x).
  Exact route: C products onto the bias, then the residual add: g_y = gamma_{C + 2}.  bf16x3: g_y = (1 + 2^-5) gamma_{6C + 3}.
* head (pre-tanh) = b + w (*) snake(x): one fp32 fma chain of 7C products from the bias (head_fused_kernel, either route):
  bound <= gamma_{7C + 1} (|b| + |w| (*) |s|) + |w| (*) e_snake(x).

No slack factor is applied: the assertion is |gpu - ref64| <= bound for every element, and the worst err / bound of every case is
printed.  The second yardstick is the project's usual one: pooled over a group of cases, the GPU's rms error against fp64 may not
exceed 1.5 x the fp32 CPU oracle's.

The fp64 references run on the CPU and dominate the wall time: the cases with hundreds of thousands of frames (grid and tile-counter
edges) are compared in windows of whole tiles around the clip edges and the grid's pass boundaries (a unit's output frame depends
on input frames t - 3 dil .. t + 3 dil only, so a window with that much context is exact).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import l3ac_amd
from l3ac_amd import _capi, weights as W
from oracle import l3ac_oracle as O
from tests import gpu_ops as G
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS_SIN = 2e-7   # test_sin_squared_range: the device sin^2 against fp64, scalar and packed forms
C1 = 3.0
TILE = 256       # frames per tile of the unit kernels and the head kernel
DILS = (1, 3, 9)
TANH_ULP = 2.0   # HIP's documented maximum error of tanhf (the same 2 ulp as CUDA's math library documents)
CONFIGS = {  # name -> (config, synthetic seed, weight profile)
    "tiny": (GOLDEN / "tiny.toml", 3, "mild"),
    "1kbps": ("1kbps", 0, "mild"),
    "1kbps-stress": ("1kbps", 0, "stress"),
    "refdefault": (GOLDEN / "refdefault.toml", 0, "mild"),
}
WANT = {True: "legacy_unit_split_kernel", False: "legacy_unit_kernel"}


def gamma(n):
    return n * U / (1.0 - n * U)


def unit_gammas(c, split):
    if split:
        return (1 + 2.0 ** -5) * gamma(42 * c + 2), (1 + 2.0 ** -5) * gamma(6 * c + 3)
    return gamma(7 * c + 1), gamma(c + 2)


class Stage:
    """One config's output stage: the context, the fp32 folded weights and their fp64 copies."""

    def __init__(self, name):
        cfg, seed, profile = CONFIGS[name]
        self.name = name
        self.codec = l3ac_amd.get_model(cfg, synthetic_seed=seed, synthetic_profile=profile)
        self.codec.network.to(device="cuda").eval()
        self.ctx = self.codec.network.context()
        mc = self.codec.network.mc
        self.c = mc.decoder_dims[-1]
        self.lp = f"decoder.blocks.{1 + 3 * len(mc.decode_rates)}.block"
        w = W.folded_weights(self.codec.network.state_dicts())
        self.w32 = {k: v for k, v in w.items() if k.startswith(self.lp)}
        self.w64 = {k: v.double() for k, v in self.w32.items()}
        alphas = [self.w64[f"{self.unit(u)}.block.{i}.alpha"] for u in range(3) for i in (0, 2)] + [self.w64[f"{self.lp}.1.alpha"]]
        ratio = max(float((a * (a + O.EPS).reciprocal()).abs().max()) for a in alphas)
        assert ratio <= 1.001, f"{name}: |alpha / (alpha + 1e-8)| = {ratio}: the snake bound's derivation does not hold"
        self.lip = 1.0 + ratio  # |d snake / dv| <= 1 + |alpha ia|

    def unit(self, u):
        return f"{self.lp}.0.{u}.module"


_STAGES = {}


def stage(name):
    if name not in _STAGES:
        _STAGES[name] = Stage(name)
    return _STAGES[name]


def _x(b, c, t, seed, loud=1):
    """seeded noise at scale 1; clip `loud` (if the batch has it) at scale 8, so that snake's sin^2 covers several periods."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, c, t), generator=g)
    if b > loud:
        x[loud] *= 8.0
    return x


def snake64(v, alpha, e_in, lip):
    ia = (alpha + O.EPS).reciprocal()
    sq = torch.sin(alpha * v).pow(2)
    s = v + ia * sq
    e = C1 * U * (v.abs() + ia.abs() * sq) + ia.abs() * (EPS_SIN * (1 + 4 * U))
    if e_in is not None:
        e = e + lip * e_in
    return s, e


def unit64(st, u, x, e_x, split):
    """fp64 LegacyUnit u on x (B, C, T) and the bound on the kernel's error (e_x: the error already in x, or None)."""
    p, d, w = st.unit(u), DILS[u], st.w64
    g_h, g_y = unit_gammas(st.c, split)
    w1, b1, w2, b2 = w[f"{p}.block.1.weight"], w[f"{p}.block.1.bias"], w[f"{p}.block.3.weight"], w[f"{p}.block.3.bias"]
    s, e_s = snake64(x, w[f"{p}.block.0.alpha"], e_x, st.lip)
    h = F.conv1d(s, w1, b1, dilation=d, padding=3 * d)
    e_h = g_h * F.conv1d(s.abs(), w1.abs(), b1.abs(), dilation=d, padding=3 * d) + F.conv1d(e_s, w1.abs(), None, dilation=d, padding=3 * d)
    s2, e_s2 = snake64(h, w[f"{p}.block.2.alpha"], e_h, st.lip)
    y = x + F.conv1d(s2, w2, b2)
    e_y = g_y * (x.abs() + F.conv1d(s2.abs(), w2.abs(), b2.abs())) + F.conv1d(e_s2, w2.abs(), None)
    if e_x is not None:
        e_y = e_y + e_x
    return y, e_y


def head64(st, x, e_x):
    """fp64 pre-tanh head on x (B, C, T) -> (B, T) and its bound."""
    w = st.w64
    hw, hb = w[f"{st.lp}.2.weight"], w[f"{st.lp}.2.bias"]
    s, e_s = snake64(x, w[f"{st.lp}.1.alpha"], e_x, st.lip)
    y = F.conv1d(s, hw, hb, padding=3).squeeze(1)
    e = gamma(7 * st.c + 1) * F.conv1d(s.abs(), hw.abs(), hb.abs(), padding=3).squeeze(1) + F.conv1d(e_s, hw.abs(), None, padding=3).squeeze(1)
    return y, e


def unit32(st, u, x):
    return O.legacy_unit(st.w32, st.unit(u), x, DILS[u])


def head32(st, x):
    s = O.snake(x, st.w32[f"{st.lp}.1.alpha"])
    return F.conv1d(s, st.w32[f"{st.lp}.2.weight"], st.w32[f"{st.lp}.2.bias"], padding=3).squeeze(1)


def ratio_of(got, ref, bound):
    err = (got.double() - ref).abs()
    ok = bool((err <= bound).all()) and bool(torch.isfinite(got).all())
    worst = float((err / bound.clamp(min=1e-300)).max())
    return ok, worst, float(err.max())


def run_unit(st, u, xf, split):
    with _capi.profile() as prof:
        y = G.legacy_unit(st.ctx, u, xf)
    names = [e["name"] for e in prof.entries]
    assert WANT[split] in names and WANT[not split] not in names, f"{st.name} unit {u}: expected {WANT[split]}, ran {names}"
    return y


def run_head(st, xf):
    with _capi.profile() as prof:
        y = G.head(st.ctx, xf)
    names = [e["name"] for e in prof.entries]
    assert "head_fused_kernel" in names and not any(n.startswith("legacy_unit") for n in names), f"{st.name} head: ran {names}"
    return y


class Route:
    """network.set_gemm_split(split) for the duration of a block; the default route (bf16x3) afterwards."""

    def __init__(self, st, split):
        self.st, self.split = st, split

    def __enter__(self):
        self.st.codec.network.set_gemm_split(self.split)
        assert self.st.ctx.get_gemm_split() == self.split

    def __exit__(self, *exc):
        self.st.codec.network.set_gemm_split(True)
        return False


class Rms:
    """pooled squared errors of the GPU and of the fp32 oracle against fp64"""

    def __init__(self):
        self.gpu, self.cpu = {}, {}

    def add(self, key, got, got32, ref):
        for acc, v in ((self.gpu, got), (self.cpu, got32)):
            s, n = acc.get(key, (0.0, 0))
            acc[key] = (s + float((v.double() - ref).pow(2).sum()), n + ref.numel())

    def check(self, label):
        for key in self.gpu:
            g = math.sqrt(self.gpu[key][0] / self.gpu[key][1])
            c = math.sqrt(self.cpu[key][0] / self.cpu[key][1])
            print(f"[{label} {key}] rms err vs fp64: gpu {g:.3e}, fp32 oracle {c:.3e}")
            assert g <= 1.5 * c + 1e-30, f"{label} {key}: GPU rms error {g:.3e} > 1.5 x the fp32 oracle's {c:.3e}"


def unit_ts(d):
    return sorted({1, 2, 3 * d - 1, 3 * d, 3 * d + 1, 6 * d + 1, 255, 256, 257, 256 + 3 * d, 511, 513 + 3 * d, 1500} - {0})


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_legacy_units_within_fp64_bound(cfg):
    """Every LegacyUnit alone on both routes at T around the halo (3 dil) and the tile (256) edges, B = 1 and 3."""
    st = stage(cfg)
    rms = Rms()
    for u, d in enumerate(DILS):
        for t in unit_ts(d):
            for b in (1, 3):
                x = _x(b, st.c, t, seed=1000 * u + 7 * t + b)
                ref, bound = unit64(st, u, x.double(), None, True)
                ref_e, bound_e = unit64(st, u, x.double(), None, False)
                ref32 = unit32(st, u, x)
                xf = G.to_frames(x)
                for split in (True, False):
                    with Route(st, split):
                        got = G.from_frames(run_unit(st, u, xf, split))
                    bd = bound if split else bound_e
                    ok, worst, err = ratio_of(got, ref, bd)
                    route = "bf16x3" if split else "fp32"
                    print(f"[{cfg} unit {u} dil {d} {route} B={b} T={t}] max err {err:.3e}, worst err/bound {worst:.3f}")
                    assert ok, f"{cfg} unit {u} (dil {d}) {route} B={b} T={t}: max err {err:.3e}, worst err/bound {worst:.3f}"
                    rms.add(f"unit {u} {route}", got, ref32, ref)
    rms.check(cfg)


def _windows(b, t, d, extra_tiles=()):
    """(clip, lo, hi) frame windows: whole tiles (plus 8 frames either side) at the clip edges, mid-clip, and the given global tiles."""
    tpc = -(-t // TILE)
    pick = set()
    for clip in range(b):
        for k in (0, 1, tpc // 2, tpc - 2, tpc - 1):
            if 0 <= k < tpc:
                pick.add((clip, k))
    for g in extra_tiles:
        if g < b * tpc:
            pick.add((g // tpc, g % tpc))
    return [(clip, max(0, TILE * k - 8), min(t, TILE * (k + 1) + 8)) for clip, k in sorted(pick)]


def _check_windows(st, u, x, got, split, label):
    """got (B, C, T) against the fp64 reference in the windows; returns the worst err / bound."""
    d = DILS[u]
    worst = 0.0
    b, _, t = x.shape
    for clip, lo, hi in _windows(b, t, d, extra_tiles=(511, 512, 1023, 1024)):
        elo, ehi = max(0, lo - 3 * d), min(t, hi + 3 * d)
        ref, bound = unit64(st, u, x[clip:clip + 1, :, elo:ehi].double(), None, split)
        ok, w, err = ratio_of(got[clip:clip + 1, :, lo:hi], ref[..., lo - elo:hi - elo], bound[..., lo - elo:hi - elo])
        assert ok, f"{label} clip {clip} frames [{lo}, {hi}): max err {err:.3e}, worst err/bound {w:.3f}"
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_legacy_units_grid_and_counter_edges(cfg):
    """Total tiles 512 (the full persistent grid, one pass), 513 (a second pass of one tile), 1024 (two full passes: still static
    shares) and 1025 (tiles by counter, unit_counter 1 / 3, against static shares 0: the same bits, and all within the bound)."""
    st = stage(cfg)
    cases = ((2, 65536), (1, 131328), (4, 65536), (5, 52225))
    for ci, (b, t) in enumerate(cases):
        tiles = b * -(-t // TILE)
        x = _x(b, st.c, t, seed=77 + ci)
        xf = G.to_frames(x)
        for u, d in enumerate(DILS):
            for split in (True, False):
                route = "bf16x3" if split else "fp32"
                outs = {}
                for mode in ((0, 1, 3) if tiles > 1024 else (1,)):
                    st.ctx.set_option("unit_counter", mode)
                    try:
                        with Route(st, split):
                            outs[mode] = G.from_frames(run_unit(st, u, xf, split))
                    finally:
                        st.ctx.set_option("unit_counter", 1)
                    label = f"{cfg} unit {u} dil {d} {route} B={b} T={t} ({tiles} tiles) unit_counter={mode}"
                    worst = _check_windows(st, u, x, outs[mode], split, label)
                    print(f"[{label}] worst err/bound {worst:.3f}")
                first = next(iter(outs.values()))
                for mode, y in outs.items():
                    assert torch.equal(y, first), f"{cfg} unit {u} {route} B={b} T={t}: unit_counter={mode} changes the bits"


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_output_stage_clip_isolation_and_run_to_run(cfg):
    """A clip's output does not depend on its neighbours (filled ~10^3 larger: a leak across the clip edge cannot hide under a
    tolerance): each unit and the head, in a batch of three, equal the middle clip run alone, and a second call the first, bit for bit."""
    st = stage(cfg)
    for split in (True, False):
        with Route(st, split):
            for u, d in enumerate(DILS):
                for t in (1, 3 * d - 1, 3 * d + 1, 257, 513 + 3 * d):
                    x = _x(3, st.c, t, seed=500 + t, loud=3)
                    x[0] *= 1e3
                    x[2] *= 1e3
                    xf = G.to_frames(x)
                    y = run_unit(st, u, xf, split)
                    assert torch.equal(run_unit(st, u, xf, split), y), f"{cfg} unit {u} T={t}: two calls differ"
                    alone = run_unit(st, u, xf[1:2].contiguous(), split)
                    assert torch.equal(alone[0], y[1]), f"{cfg} unit {u} T={t} split={split}: the neighbours leak into the clip"
            for t in (1, 3, 4, 257):
                x = _x(3, st.c, t, seed=600 + t, loud=3)
                x[0] *= 1e3
                x[2] *= 1e3
                xf = G.to_frames(x)
                for pre in (True, False):
                    st.ctx.set_head_pretanh(pre)
                    try:
                        y = run_head(st, xf)
                        assert torch.equal(run_head(st, xf), y)
                        alone = run_head(st, xf[1:2].contiguous())
                    finally:
                        st.ctx.set_head_pretanh(False)
                    assert torch.equal(alone[0], y[1]), f"{cfg} head T={t} pretanh={pre}: the neighbours leak into the clip"


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_head_within_fp64_bound_and_tanh(cfg):
    """The head's pre-tanh value (head_pretanh on) within the fp64 bound; with it off, the output is tanh of the device's own pre-tanh
    value within tanhf's 2 ulp."""
    st = stage(cfg)
    rms = Rms()
    for t in (1, 2, 3, 4, 255, 256, 257, 259, 1500):
        for b in (1, 3):
            x = _x(b, st.c, t, seed=300 + t + b)
            ref, bound = head64(st, x.double(), None)
            ref32 = head32(st, x)
            xf = G.to_frames(x)
            for split in (True, False):
                with Route(st, split):
                    st.ctx.set_head_pretanh(True)
                    try:
                        pre = run_head(st, xf).cpu()
                    finally:
                        st.ctx.set_head_pretanh(False)
                    out = run_head(st, xf).cpu()
                ok, worst, err = ratio_of(pre, ref, bound)
                print(f"[{cfg} head split={split} B={b} T={t}] pre-tanh max err {err:.3e}, worst err/bound {worst:.3f}")
                assert ok, f"{cfg} head B={b} T={t}: max err {err:.3e}, worst err/bound {worst:.3f}"
                rms.add(f"head split={split}", pre, ref32, ref)
                exact = torch.tanh(pre.double())
                ulp = torch.from_numpy(np.spacing(exact.abs().float().numpy())).double()
                terr = (out.double() - exact).abs()
                assert (terr <= TANH_ULP * ulp).all(), f"{cfg} head B={b} T={t}: tanh off by {float((terr / ulp).max()):.2f} ulp"
    rms.check(cfg)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_last_block_is_the_composition_of_the_parts(cfg):
    """l3ac_op_last_block == op_head(op_legacy_unit(2, op_legacy_unit(1, op_legacy_unit(0, x)))) bit for bit, on both routes, with and
    without tanh, and on a batch whose units hand their tiles out by counter: the parts are what the pipeline runs."""
    st = stage(cfg)
    for b, t in ((1, 1), (3, 257), (2, 1500), (5, 52225)):
        xf = G.to_frames(_x(b, st.c, t, seed=800 + t))
        for split in (True, False):
            with Route(st, split):
                for pre in (True, False):
                    st.ctx.set_head_pretanh(pre)
                    try:
                        whole = G.op_plain(st.ctx, "l3ac_op_last_block", xf, b, t, (b, t))
                        y = xf
                        for u in range(3):
                            y = run_unit(st, u, y, split)
                        parts = run_head(st, y)
                    finally:
                        st.ctx.set_head_pretanh(False)
                    assert torch.equal(whole, parts), f"{cfg} B={b} T={t} split={split} pretanh={pre}: last_block != its parts"


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_last_block_pretanh_within_fp64_bound(cfg):
    """The whole stage (three units and the head, pre-tanh) against the fp64 composition, the units' bounds carried through."""
    st = stage(cfg)
    rms = Rms()
    for t in (1, 27, 28, 257, 1500):
        b = 3
        x = _x(b, st.c, t, seed=900 + t)
        r32 = x
        for u in range(3):
            r32 = unit32(st, u, r32)
        r32 = head32(st, r32)
        xf = G.to_frames(x)
        for split in (True, False):
            r, e = x.double(), None
            for u in range(3):
                r, e = unit64(st, u, r, e, split)
            ref, bound = head64(st, r, e)
            with Route(st, split):
                st.ctx.set_head_pretanh(True)
                try:
                    got = G.op_plain(st.ctx, "l3ac_op_last_block", xf, b, t, (b, t)).cpu()
                finally:
                    st.ctx.set_head_pretanh(False)
            ok, worst, err = ratio_of(got, ref, bound)
            print(f"[{cfg} last_block split={split} B={b} T={t}] pre-tanh max err {err:.3e}, worst err/bound {worst:.3f}")
            assert ok, f"{cfg} last_block split={split} T={t}: max err {err:.3e}, worst err/bound {worst:.3f}"
            rms.add(f"last_block split={split}", got, r32, ref)
    rms.check(cfg)


def test_legacy_unit_entry_refuses_bad_arguments():
    st = stage("tiny")
    x = G.to_frames(_x(1, st.c, 40, seed=1))
    with pytest.raises(_capi.L3acError, match="alias"):
        G.legacy_unit(st.ctx, 0, x, out=x)
    for bad in (-1, 3):
        with pytest.raises(_capi.L3acError, match="unit"):
            G.legacy_unit(st.ctx, bad, x)
