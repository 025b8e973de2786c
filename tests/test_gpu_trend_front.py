"""The two trend front ends on the MI355X against an fp64 restatement of the oracle, per element within an a-priori error bound: the
encoder stem (kernels/first_block.hip: l3ac_op_first_block / l3ac_op_first_block_at, both of its forms, every compiled d0) and the
decoder's EnhanceBlock (kernels/enhance.hip + the gate: l3ac_op_enhance, and l3ac_op_enhance_up for the gate's three evaluators), on
inputs that reach the pad rules, the halos, the tile edges and an InstanceNorm at 1/std up to 316 -- plus bit-exact properties: the two
stem forms, padding folded into the load, a strided input, clip isolation, run to run.

The fp64 references evaluate the oracle's own formulas (O.trend_pool, F.conv1d, F.gelu, the InstanceNorm's mean / biased variance)
on the folded fp32 weights and the fp32 input, widened; they are checked against O.first_block / O.enhance_block run in fp64.

The bounds.  u = 2^-24, gamma_n = n u / (1 - n u).  Every quantity is evaluated in fp64 from the reference's fp64 intermediates; where
a rounding acts on a COMPUTED value, |value| + (its error so far) stands for it, so nothing is dropped as "second order".

Stem (first_block_trends + the two 1x1 convs):
* m = max_pool(|x|, k): fabsf / fmaxf are exact; the zero the kernels start from stands for ATen's -inf pad because |x| >= 0.
* p = avg_pool(m, k): at most k - 1 fp32 additions (left to right) and one division by k: e_p <= gamma_k p.  (k = 1: p = x, e_p = 0.)
* h = b + w (*) p, seven fmas from the bias: e_h <= gamma_7 (|b| + |w| (*) (|p| + e_p)) + |w| (*) e_p.
* s = b1 + W1 h, twenty fmas: e_s <= gamma_20 (|b1| + |W1| (|h| + e_h)) + |W1| e_h.
* g = gelu(s): the kernels' gelu_erf at an fp32 argument is within 0.5 |s| 1.2e-7 + 1.5 ulp(g) of the exact value
  (test_gelu_known_answers asserts exactly this), and |gelu'| <= 1.13 carries e_s: e_g <= 0.5 (|s| + e_s) 1.2e-7 +
  1.5 ulp(|g| + 1.13 e_s) + 1.13 e_s.
* y = b2 + W2 [g; x], 81 fmas: e_y <= gamma_81 (|b2| + |W2| (|[g; x]| + [e_g; 0])) + |W2[:, :80]| e_g.

EnhanceBlock (enhance_branches_kernel, enhance_stats_kernel, the gate).  The bound is the one of an all-fp32 evaluation; where the
kernels do better (marked "now") it holds a fortiori, and it is kept as it is: what it has to catch is logic, not rounding.
* the four branches as above with k in (1, 3, 5, 9), dilation k // 2 + 1: e_yi.  (Now: the seven taps are summed in fp64 and rounded
  once, which is within gamma_7 of seven fp32 fmas.)
* mean: enhance_stats_kernel adds ceil(T / 1024) values per thread, 6 butterfly levels per wave and 16 wave partials: no value passes
  through more than D = ceil(T / 1024) + 6 + 16 additions, then 1 / (float)T and one product:
  e_mean <= gamma_{D+2} mean(|yi| + e_yi) + mean(e_yi).  (gamma_T would be vacuous at T = 16200 and 1/std = 300.  Now: the same
  reduction in fp64.)
* d = yi - mean, one subtraction: e_d <= e_yi + e_mean + u (|d| + e_yi + e_mean).  (Now: taken in fp64 against the fp64 mean and
  rounded once, by enhance_stats_kernel, which writes it over yi; the gate evaluators subtract a stored mean of 0.)
* var = mean(d^2): one product each, the same reduction, 1 / T: e_var <= mean(2 |d| e_d + e_d^2) + gamma_{D+3} mean((|d| + e_d)^2).
* a = var + 1e-5 (1e-5f is within u of 1e-5; one addition): e_a <= e_var + u 1e-5 + u (a + e_var).  rstd = 1 / sqrtf(a), both
  correctly rounded: relative error <= 0.5 e_a / (a - e_a) + 4 u.
* z = d rstd in_w + in_b, three roundings however contracted: with E = |in_w| (rstd e_d + |d| e_rstd + e_d e_rstd),
  e_z <= E + gamma_3 (|d rstd in_w| + |in_b| + E).  rstd |in_w| e_d is the conditioning term: at a near-constant channel 0 rstd is
  144 .. 316 and this is what the DC and silence inputs exercise.
* g = gate_b + gate_w . z, four multiply-adds however contracted (rows.hip, up_fused.hip and the gated GEMM contract them
  differently): e_g <= gamma_5 (|gate_b| + |gate_w| (|z| + e_z)) + |gate_w| e_z.
* out = x + g x: e_out <= |x| e_g + gamma_2 (|x| + (|g| + e_g) |x|).

No slack factor is applied: the assertion is |gpu - ref64| <= bound on every element of every case, everything finite.  The bound is
loose against random rounding (the fp32 CPU oracle sits at 0.003 .. 0.2 of it), so it catches logic errors -- a wrong pad rule or a
frame of shift moves the output by hundreds of bounds -- while the sharp instruments are the second yardstick (pooled per config and
input kind, the GPU's rms error against fp64 may not exceed 1.5 x the fp32 CPU oracle's) and the bit-for-bit properties.

l3ac_op_enhance_up, where the gate is not observable alone, is held on the same inputs to: rms error against fp64 <= 1.5 x the fp32
oracle's, and max error <= 2 x that of the GPU's own two-call route (l3ac_op_enhance, then l3ac_op_up_layer) + 1e-7 (the factors of
test_conv_units_wide_fused), on both routes, with the profile asserting which evaluator of the gate ran.  Only channel 0 -- the only one
the gate reads -- carries the structured signal; the other channels stay noise, so that the up layer's ChannelNorm (eps 1e-8), which
is not this file's subject, stays well conditioned.

F.instance_norm refuses a single frame per channel, so at T = 1 the EnhanceBlock has no fp32 oracle: that length is held to the fp64
restatement and the bound only (its InstanceNorm is z = in_b), and l3ac_op_enhance_up's list starts at 2.

The stem's profile name is the same for both forms: which one ran is asserted from the shape, with launch_first_block's own rule
(few = ceil(frames / 64) * batch <= 1024 -> first_block_split_kernel).

Observed on the MI355X (every test prints its figures; "rms ratio" is the GPU's rms error over the fp32 oracle's, per input kind):
* stem, all six configs (d0 = 8, 16, 24, 32), both forms bit for bit: worst err / bound 0.026 (tiny), 0.032 (1kbps, refdefault), 0.076
  (1kbps-stress), 0.042 (stem16), 0.035 (stem32), each at the 1e-6 input; the fp32 oracle's own worst is 0.02 - 0.08.  Rms error 9e-9
  (silence) .. 1.1e-7 (noise); rms ratio 0.85 .. 1.17, and 1.45 for DC at d0 = 16.  No test of the stem has failed on any build.
* l3ac_op_enhance: worst err / bound 0.114 (tiny), 0.164 (1kbps), 0.145 (1kbps-stress), 0.146 (refdefault), each at the tile impulses
  (the oracle: up to 0.19).  The rms yardstick is what found something, twice, and enhance.hip says what was changed for it:
  - with fp32 statistics (the kernels as they were) the rms ratio was 4.1 - 6.5 for silence, 1.6 - 9.9 for DC, 3.4 - 14 for the square
    wave, 2.9 - 5.8 for the edge impulses, 2.5 - 3.7 for the 1e-6 input (tiny, 1kbps, refdefault; 1kbps-stress alike), and 0.9 - 1.1 for
    noise: the mean's rounding times 1/std = 316.  With fp64 sums and yi centred in place: silence 0.04 - 0.23, DC 0.07 - 0.19, square
    0.09 - 0.22, edge impulses 0.28 - 0.66, x100 loud 0.09 - 0.26, noise and the other kinds 0.58 - 1.15;
  - the 1e-6 input stayed at 1.55 - 1.74 (the branch convs' seven fp32 roundings at the bias's magnitude) until their taps were summed
    in fp64; with that the assertion holds for every kind in every config.  (The per-kind figures of that last build were not kept.)
* l3ac_op_enhance_up: rms ratio 0.44 - 1.10 (tiny), 1.00 elsewhere, on both routes, where both errors against fp64 (5e-5 .. 1e-3) are
  those of F.interpolate's fp32 source coordinate at frame numbers in the thousands, which the kernels reproduce: on long clips the
  sharp check of this entry is the max error against the two-call route (observed 0.5 - 1.7 x it at up_fused_kernel, equal to it elsewhere).
* The whole file (44 tests): 37 s of wall time, 32 s of it inside pytest, 30 s of that in the loops over the cases (fp64 references and
  fp32 oracle included) -- measured before the short edge lengths were given to every decoder stage, which adds a few seconds.
"""
import math
import time

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
CONFIGS = {  # name -> (config, synthetic seed, weight profile)
    "tiny": (GOLDEN / "tiny.toml", 3, "mild"),
    "1kbps": ("1kbps", 0, "mild"),
    "1kbps-stress": ("1kbps", 0, "stress"),
    "refdefault": (GOLDEN / "refdefault.toml", 0, "mild"),
    "stem16": (GOLDEN / "stem16.toml", 3, "mild"),   # tiny with encoder_dims[0] = 16 / 32: the stem's other two instantiations
    "stem32": (GOLDEN / "stem32.toml", 3, "mild"),
}
STEM_CONFIGS = list(CONFIGS)
ENH_CONFIGS = ["tiny", "1kbps", "1kbps-stress", "refdefault"]
STEM = "encoder.blocks.0"
STEM_POOLS = (1, 5, 11, 21, 45)
ENH_POOLS = (1, 3, 5, 9)
STEM_TS = (1, 2, 3, 4, 7, 22, 23, 44, 45, 46, 47, 48, 63, 64, 65, 94, 111, 175, 255, 256, 257, 303, 511, 513, 1000, 4000, 16200)
ENH_TS = (1, 2, 3, 6, 7, 15, 16, 22, 23, 24, 46, 47, 255, 256, 257, 279, 511, 513, 1023, 1024, 1025, 2700, 16200)
TILE_OFFSETS = (-47, -25, -23, -22, -3, -1, 0, 1, 3, 22, 46)
UP_FUSED = ((256, 96), (96, 48), (48, 24))


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp32(v):
    """the fp32 spacing at |v| (fp64 tensor), not smaller than the spacing of any fp32 value of that magnitude"""
    return torch.from_numpy(np.spacing((v.abs() * (1 + 2.0 ** -22)).float().numpy())).double()


class Model:
    """One config: the context, the fp32 folded weights and their fp64 copies."""

    def __init__(self, name):
        cfg, seed, profile = CONFIGS[name]
        self.name = name
        self.codec = l3ac_amd.get_model(cfg, synthetic_seed=seed, synthetic_profile=profile)
        self.codec.network.to(device="cuda").eval()
        self.ctx = self.codec.network.context()
        self.mc = mc = self.codec.network.mc
        self.w32 = W.folded_weights(self.codec.network.state_dicts())
        keep = lambda k: k.startswith(STEM + ".") or any(k.startswith(f"decoder.blocks.{2 + 3 * i}.") or k.startswith(f"decoder.blocks.{3 + 3 * i}.")
                                                         for i in range(len(mc.decode_rates)))
        self.w64 = {k: v.double() for k, v in self.w32.items() if keep(k)}
        self.d0 = mc.encoder_dims[0]
        self.hop = mc.hop_length
        # decoder stage i: (EnhanceBlock, up layer, cin, cout, scale, frames per token)
        self.stages = []
        mult = mc.en_coder_compress_rate
        for i, s in enumerate(mc.decode_rates):
            self.stages.append((f"decoder.blocks.{2 + 3 * i}", f"decoder.blocks.{3 + 3 * i}", mc.decoder_dims[i], mc.decoder_dims[i + 1], s, mult))
            mult *= s


_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = Model(name)
    return _MODELS[name]


class Route:
    """network.set_gemm_split(split) for the duration of a block; the default route (bf16x3) afterwards."""

    def __init__(self, m, split):
        self.m, self.split = m, split

    def __enter__(self):
        self.m.codec.network.set_gemm_split(self.split)
        assert self.m.ctx.get_gemm_split() == self.split

    def __exit__(self, *exc):
        self.m.codec.network.set_gemm_split(True)
        return False


class Rms:
    """pooled squared errors of the GPU and of the fp32 oracle against fp64, and the worst err / bound, per key"""

    def __init__(self):
        self.gpu, self.cpu, self.worst = {}, {}, {}

    def add(self, key, got, got32, ref):
        for acc, v in ((self.gpu, got), (self.cpu, got32)):
            s, n = acc.get(key, (0.0, 0))
            acc[key] = (s + float((v.double() - ref).pow(2).sum()), n + ref.numel())

    def ratio(self, key, w):
        self.worst[key] = max(self.worst.get(key, 0.0), w)

    def check(self, label):
        bad = []
        for key in self.gpu:
            g = math.sqrt(self.gpu[key][0] / self.gpu[key][1])
            c = math.sqrt(self.cpu[key][0] / self.cpu[key][1])
            w = f", worst err/bound {self.worst[key]:.3f}" if key in self.worst else ""
            print(f"[{label} | {key}] rms err vs fp64: gpu {g:.3e}, fp32 oracle {c:.3e}{w}")
            if not g <= 1.5 * c + 1e-30:
                bad.append(f"{key}: GPU rms error {g:.3e} > 1.5 x the fp32 oracle's {c:.3e}")
        assert not bad, f"{label}: " + "; ".join(bad)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def signals(t, seed, gauss=False, loud=False):
    """(kinds, [B][t] fp32): one clip per input kind (several for the tile impulses).  Amplitudes <= 1 unless gauss / loud (the
    EnhanceBlock's channel 0).  An interior impulse is blind to the pad rule, DC is blind to interior shifts, noise sees both but only
    as "some error": hence the mix."""
    g = torch.Generator().manual_seed(seed)
    noise = lambda: torch.randn(t, generator=g) if gauss else torch.rand(t, generator=g) * 2 - 1
    n = torch.arange(t)
    kinds, clips = [], []

    def add(kind, x):
        kinds.append(kind)
        clips.append(x.float())
    add("noise", noise())
    add("silence", torch.zeros(t))
    add("dc", torch.full((t,), 0.3))
    add("dc+1e-3 noise", 0.3 + 1e-3 * noise())
    add("square", 1.0 - 2.0 * ((n // 16) % 2).float())
    add("step", torch.where(n < t // 2, 0.0, 0.8))
    add("negative", -torch.rand(t, generator=g))
    x = torch.zeros(t)
    x[0] = x[-1] = 1.0
    add("edge impulses", x)
    for stride in (64, 256):  # the tile starts of first_block_split_kernel and of the 256-frame kernels
        for off in TILE_OFFSETS:
            pos = torch.arange(0, t + 64, stride) + off
            x = torch.zeros(t)
            x[pos[(pos >= 0) & (pos < t)]] = 1.0
            add("tile impulses", x)
    if loud:
        add("x100 loud", 100.0 * noise())
    add("1e-6 quiet", 1e-6 * noise())
    return kinds, torch.stack(clips)


# ---- stem: fp64 reference, bound, runners -----------------------------------------------------------------------------------------
def branches64(w, prefix, x, pools, rate):
    """trend branches of x (B, 1, T) fp64 -> (h, e_h), (B, len(pools) * each, T)"""
    hs, es = [], []
    for i, k in enumerate(pools):
        dil = k // rate + 1
        p = O.trend_pool(x, k)
        e_p = gamma(k) * p if k > 1 else torch.zeros_like(p)
        cw, cb = w[f"{prefix}.blocks.{i}.1.weight"], w[f"{prefix}.blocks.{i}.1.bias"]
        hs.append(F.conv1d(p, cw, cb, dilation=dil, padding=3 * dil))
        es.append(gamma(7) * F.conv1d(p.abs() + e_p, cw.abs(), cb.abs(), dilation=dil, padding=3 * dil)
                  + F.conv1d(e_p, cw.abs(), None, dilation=dil, padding=3 * dil))
    return torch.cat(hs, 1), torch.cat(es, 1)


def stem64(w, x):
    """fp64 stem on x (B, T) -> (y, bound), (B, d0, T)"""
    x = x.unsqueeze(1)
    h, e_h = branches64(w, STEM, x, STEM_POOLS, 99)
    w1, b1 = w[f"{STEM}.conv_1.weight"], w[f"{STEM}.conv_1.bias"]
    s = F.conv1d(h, w1, b1)
    e_s = gamma(20) * F.conv1d(h.abs() + e_h, w1.abs(), b1.abs()) + F.conv1d(e_h, w1.abs())
    g = F.gelu(s)
    e_g = 0.5 * (s.abs() + e_s).clamp(max=10.0) * 1.2e-7 + 1.5 * ulp32(g.abs() + 1.13 * e_s) + 1e-38 + 1.13 * e_s
    w2, b2 = w[f"{STEM}.conv_2.weight"], w[f"{STEM}.conv_2.bias"]
    cat, e_cat = torch.cat([g, x], 1), torch.cat([e_g, torch.zeros_like(x)], 1)
    y = F.conv1d(cat, w2, b2)
    return y, gamma(81) * F.conv1d(cat.abs() + e_cat, w2.abs(), b2.abs()) + F.conv1d(e_cat, w2.abs())


def few(batch, frames):
    """launch_first_block's rule: first_block_split_kernel (64-frame workgroups) up to 1024 of them, first_block_kernel beyond"""
    return -(-frames // 64) * batch <= 1024


def stem_call(m, audio, samples=None, frames=None, want_few=None):
    """the stem on audio [B][S] (GPU) through l3ac_op_first_block_at -> (B, d0, frames) on the CPU, the form asserted from the shape"""
    b = audio.shape[0]
    f = (audio.shape[1] if samples is None else samples) if frames is None else frames
    if want_few is not None:
        assert few(b, f) == want_few, f"{m.name}: B={b} frames={f} does not take the {'split' if want_few else 'batch'} form"
    with _capi.profile() as prof:
        y = G.first_block_at(m.ctx, audio, samples, frames)
    names = [e["name"] for e in prof.entries]
    assert names == ["first_block_kernel"], f"{m.name}: the stem ran {names}"
    return G.from_frames(y)


def stem_form(m, audio, form, samples=None, frames=None):
    """every clip of audio [B][S] (GPU) through the wanted form of the stem: the split form in calls of as many clips as it takes, the
    batch form with the batch repeated until launch_first_block picks it (the repeats must agree bit for bit)."""
    b = audio.shape[0]
    f = (audio.shape[1] if samples is None else samples) if frames is None else frames
    wgs = -(-f // 64)
    if form == "split":
        n = 1024 // wgs
        assert n >= 1, f"frames={f}: no batch takes the split form"
        return torch.cat([stem_call(m, audio[i:i + n].contiguous(), samples, frames, want_few=True) for i in range(0, b, n)])
    reps = 1024 // (wgs * b) + 1
    y = stem_call(m, audio.repeat(reps, 1), samples, frames, want_few=False)
    assert torch.equal(y[(reps - 1) * b:], y[:b]), f"{m.name} frames={f}: the batch form's clips depend on their place in the batch"
    return y[:b]


def ratio_of(got, ref, bound):
    """-> (all within the bound and finite, worst err / bound per clip, max err)"""
    err = (got.double() - ref).abs()
    ok = bool((err <= bound).all()) and bool(torch.isfinite(got).all())
    per_clip = (err / bound.clamp(min=1e-300)).flatten(1).max(1).values
    return ok, per_clip, float(err.max())


def check_stem64_is_the_oracle(m):
    x = signals(300, 5)[1][:4].double()
    ref = O.first_block(m.w64, STEM, x.unsqueeze(1))
    assert torch.allclose(stem64(m.w64, x)[0], ref, rtol=1e-13, atol=1e-15), f"{m.name}: stem64 is not O.first_block in fp64"


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", STEM_CONFIGS)
def test_stem_within_fp64_bound_in_both_forms(cfg):
    """Every input kind at every length, through BOTH forms of the stem (bit for bit the same), within the bound of the fp64
    reference on every element; pooled per input kind, the rms error at most 1.5 x the fp32 oracle's."""
    m = model(cfg)
    check_stem64_is_the_oracle(m)
    rms = Rms()
    t_start = time.time()
    for t in sorted(set(STEM_TS) | {2 * m.hop, 60 * m.hop}):
        kinds, x = signals(t, seed=1000 + t)
        assert float(x.abs().max()) <= 1.0
        ref, bound = stem64(m.w64, x.double())
        ref32 = O.first_block(m.w32, STEM, x.unsqueeze(1))
        xg = x.cuda()
        got = stem_form(m, xg, "split")
        assert torch.equal(stem_form(m, xg, "batch"), got), f"{cfg} T={t}: first_block_kernel and first_block_split_kernel differ"
        ok, per_clip, err = ratio_of(got, ref, bound)
        w32 = float(ratio_of(ref32, ref, bound)[1].max())
        print(f"[{cfg} stem d0={m.d0} T={t}] max err {err:.3e}, worst err/bound {float(per_clip.max()):.3f} ({kinds[int(per_clip.argmax())]}); fp32 oracle {w32:.3f}")
        assert ok, f"{cfg} stem T={t}: max err {err:.3e}, worst err/bound {float(per_clip.max()):.3f} at input '{kinds[int(per_clip.argmax())]}'"
        for i, kind in enumerate(kinds):
            rms.add(kind, got[i], ref32[i], ref[i])
            rms.ratio(kind, float(per_clip[i]))
    print(f"[{cfg} stem] {time.time() - t_start:.1f} s")
    rms.check(f"{cfg} stem")


def test_stem_instantiations_all_run():
    """every L3AC_FB_CASE of launch_first_block has a config here"""
    assert sorted({model(c).d0 for c in STEM_CONFIGS}) == [8, 16, 24, 32]


@pytest.mark.parametrize("cfg", STEM_CONFIGS)
def test_stem_forms_return_the_same_bits(cfg):
    """Clips 0, 1 and the last of a batch large enough for first_block_kernel against the same clips run alone
    (first_block_split_kernel): "the same bits" (first_block.hip).  The form is asserted from the shape (one profile name for both)."""
    m = model(cfg)
    for t in (1, 65, 255, 256, 257, 303, 4000):
        b = 1024 // -(-t // 64) + 1
        g = torch.Generator().manual_seed(40 + t)
        x = (torch.rand((b, t), generator=g) * 2 - 1).cuda()
        big = stem_call(m, x, want_few=False)
        for clip in (0, 1, b - 1):
            alone = stem_call(m, x[clip:clip + 1].contiguous(), want_few=True)
            assert torch.equal(alone[0], big[clip]), f"{cfg} T={t}: clip {clip} of {b} (batch form) differs from the clip alone (split form)"


@pytest.mark.parametrize("cfg", STEM_CONFIGS)
def test_stem_padding_folded_into_the_load(cfg):
    """first_block_at(samples = s, frames = f) is first_block on the audio zero-padded to f, bit for bit, in both forms, and within
    the fp64 bound on the padded audio: f - s around the halo (47) and the hop round-up of l3ac_encode."""
    m = model(cfg)
    hop = 270
    cases = [(s, s + pad) for pad in (1, 3, 46, 47, 48, 269) for s in (1, 40, 257)] + [(s, -(-s // hop) * hop) for s in (1, 269, 271, 8191)]
    cases += [(s, -(-s // m.hop) * m.hop) for s in (1, 271)]  # the config's own hop
    for s, f in cases:
        g = torch.Generator().manual_seed(7 * s + f)
        x = torch.rand((3, s), generator=g) * 2 - 1
        x[1] = 0.3  # a DC clip: its pooled signals see the padding over the whole halo
        padded = F.pad(x, (0, f - s))
        ref, bound = stem64(m.w64, padded.double())
        xg, pg = x.cuda(), padded.cuda()
        for form in ("split", "batch"):
            got = stem_form(m, xg, form, samples=s, frames=f)
            want = stem_form(m, pg, form)
            assert torch.equal(got, want), f"{cfg} samples={s} frames={f} {form} form: the folded padding differs from explicit zeros"
            ok, per_clip, err = ratio_of(got, ref, bound)
            assert ok, f"{cfg} samples={s} frames={f} {form} form: max err {err:.3e}, worst err/bound {float(per_clip.max()):.3f}"
        print(f"[{cfg} stem samples={s} frames={f}] worst err/bound {float(per_clip.max()):.3f}")


@pytest.mark.parametrize("cfg", STEM_CONFIGS)
def test_stem_strided_input(cfg):
    """audio_stride > samples, NaN between the rows: the bits of the contiguous call, in both forms, with and without padding."""
    m = model(cfg)
    for s, f, stride in ((1, 1, 2), (257, 257, 258), (300, 540, 1000), (4000, 4050, 4001)):
        for b in (3, 1024 // -(-f // 64) + 1):
            g = torch.Generator().manual_seed(s + b)
            buf = torch.full((b, stride), float("nan"))
            buf[:, :s] = torch.rand((b, s), generator=g) * 2 - 1
            bg = buf.cuda()
            view = bg[:, :s]
            assert view.stride(0) == stride
            got = stem_call(m, view, s, f, want_few=b == 3)
            want = stem_call(m, view.contiguous(), s, f, want_few=b == 3)
            assert torch.isfinite(got).all() and torch.equal(got, want), f"{cfg} B={b} samples={s} frames={f} stride={stride}: differs from the contiguous call"


@pytest.mark.parametrize("cfg", STEM_CONFIGS)
def test_stem_clip_isolation_and_run_to_run(cfg):
    """A clip inside a batch is the clip alone (neighbours at full scale against a quiet clip: a leak cannot hide), a second call is
    the first, and a small shape after a large one and back returns the same bits."""
    m = model(cfg)
    for t in (1, 46, 47, 64, 65, 257, 1000):
        g = torch.Generator().manual_seed(90 + t)
        x = torch.rand((3, t), generator=g) * 2 - 1
        x[1] *= 1e-3
        xg = x.cuda()
        y = stem_call(m, xg, want_few=True)
        assert torch.equal(stem_call(m, xg, want_few=True), y), f"{cfg} T={t}: two calls differ"
        assert torch.equal(stem_call(m, xg[1:2].contiguous(), want_few=True)[0], y[1]), f"{cfg} T={t}: the neighbours leak into the clip"
    g = torch.Generator().manual_seed(99)
    small, large = (torch.rand((1, 7), generator=g) * 2 - 1).cuda(), (torch.rand((40, 4000), generator=g) * 2 - 1).cuda()
    ys, yl = stem_call(m, small, want_few=True), stem_call(m, large, want_few=False)
    assert torch.equal(stem_call(m, small, want_few=True), ys) and torch.equal(stem_call(m, large, want_few=False), yl)


def test_first_block_at_refuses_bad_arguments():
    m = model("tiny")
    x = torch.zeros((2, 64)).cuda()
    y = torch.empty((2, 64, m.d0)).cuda()
    call = lambda samples, stride, frames: _capi.check(m.ctx.lib.l3ac_op_first_block_at(
        m.ctx.handle, x.data_ptr(), 2, samples, stride, frames, y.data_ptr(), torch.cuda.current_stream().cuda_stream))
    with pytest.raises(_capi.L3acError, match="frames"):
        call(40, 64, 39)
    with pytest.raises(_capi.L3acError, match="stride"):
        call(40, 39, 64)
    for bad in (0, -1):
        with pytest.raises(_capi.L3acError, match="samples"):
            call(bad, 64, 64)
    call(40, 64, 64)
    torch.cuda.synchronize()


# ---- EnhanceBlock: fp64 reference, bound, runners ---------------------------------------------------------------------------------
def enhance64(w, p, x):
    """fp64 EnhanceBlock p on x (B, C, T) -> (out, bound)"""
    t = x.shape[-1]
    yi, e_yi = branches64(w, p, x[:, :1], ENH_POOLS, 2)
    depth = -(-t // 1024) + 6 + 16
    mean = yi.mean(-1, keepdim=True)
    e_mean = gamma(depth + 2) * (yi.abs() + e_yi).mean(-1, keepdim=True) + e_yi.mean(-1, keepdim=True)
    d = yi - mean
    e_d = e_yi + e_mean
    e_d = e_d + U * (d.abs() + e_d)
    var = d.pow(2).mean(-1, keepdim=True)
    e_var = (2 * d.abs() * e_d + e_d.pow(2)).mean(-1, keepdim=True) + gamma(depth + 3) * (d.abs() + e_d).pow(2).mean(-1, keepdim=True)
    a = var + 1e-5
    e_a = e_var + U * 1e-5 + U * (a + e_var)
    assert bool((e_a < a).all())
    rstd = a.rsqrt()
    e_rstd = rstd * (0.5 * e_a / (a - e_a) + 4 * U)
    in_w, in_b = w[f"{p}.merge_layer.0.weight"].view(1, -1, 1), w[f"{p}.merge_layer.0.bias"].view(1, -1, 1)
    prod = d * rstd * in_w
    e_cond = in_w.abs() * (rstd * e_d + d.abs() * e_rstd + e_d * e_rstd)  # rstd |in_w| e_d: the conditioning term
    z = prod + in_b
    e_z = e_cond + gamma(3) * (prod.abs() + in_b.abs() + e_cond)
    gw, gb = w[f"{p}.merge_layer.1.weight"], w[f"{p}.merge_layer.1.bias"]
    g = F.conv1d(z, gw, gb)
    e_g = gamma(5) * F.conv1d(z.abs() + e_z, gw.abs(), gb.abs()) + F.conv1d(e_z, gw.abs())
    out = x + g * x
    return out, x.abs() * e_g + gamma(2) * (x.abs() + (g.abs() + e_g) * x.abs()), float(rstd.max())


def up_ref(w, ub, scale, e):
    """the up layer on the gated rows (the three lines of test_enhance_and_up_layers), in e's precision"""
    r = F.conv1d(e, w[f"{ub}.0.weight"], w[f"{ub}.0.bias"])
    r = F.interpolate(r, scale_factor=scale, mode="linear", align_corners=False)
    return O.channel_norm_first(r, w[f"{ub}.2.weight"], w[f"{ub}.2.bias"])


def enh_input(c, t, seed, lo=0, hi=None):
    """(kinds, x (B, c, t)): channel 0 carries the input kinds, the other channels noise"""
    kinds, x0 = signals(t, seed, gauss=True, loud=True)
    hi = len(kinds) if hi is None else hi
    x = torch.stack([torch.randn((c, t), generator=torch.Generator().manual_seed(64 * seed + j)) for j in range(lo, hi)])
    x[:, 0] = x0[lo:hi]
    return kinds[lo:hi], x


def names_of(prof):
    return [e["name"] for e in prof.entries]


def run_enhance(m, eb, xf):
    with _capi.profile() as prof:
        y = G.op_block(m.ctx, "l3ac_op_enhance", eb, xf, tuple(xf.shape))
    names = names_of(prof)
    assert sorted(names) == ["enhance_branches_kernel", "enhance_stats_kernel", "gate_flat_kernel"], f"{m.name} {eb}: l3ac_op_enhance ran {names}"
    return y


def gate_evaluator_expected(cin, cout, split):
    """run_enhance_up's choice, from the weight's shape and the route only"""
    if split and (cin, cout) in UP_FUSED:
        return f"up_fused_kernel<{cin},{cout}>"
    if split and cout >= 192 and cin >= 32 and cin % 8 == 0:  # a 1x1 conv wide enough for the bf16x3 GEMM: gate row pass, then the GEMM
        return "gate_flat_kernel"
    return "gemm_f32_kernel<gated>"


def run_enhance_up(m, eb, ub, xf, cin, cout, scale, split):
    with _capi.profile() as prof:
        y = G.op_block2(m.ctx, "l3ac_op_enhance_up", eb, ub, xf, (xf.shape[0], xf.shape[1] * scale, cout))
    names = names_of(prof)
    ran = {n for n in names if n.startswith("up_fused_kernel")} | {"gate_flat_kernel" for n in names if n == "gate_flat_kernel"} \
        | {"gemm_f32_kernel<gated>" for n in names if n.startswith("gemm_f32_kernel<") and ",gated>" in n}
    want = gate_evaluator_expected(cin, cout, split)
    assert ran == {want}, f"{m.name} {eb}+{ub} split={split}: expected the gate in {want}, ran {names}"
    if want == "gate_flat_kernel":
        assert any(n.startswith("gemm_split_kernel") for n in names), f"{m.name} {eb}+{ub}: expected the bf16x3 GEMM after the gate pass, ran {names}"
    return y, want


def stage_ts(m, i):
    """the lengths of stage i: its real frame counts for a 2-token and a 60-token clip, and the short edge lengths (the halo of 23,
    up_fused_kernel's 14-frame tiles, the 256-frame tile of enhance_branches_kernel), so that every gate evaluator sees them; the last
    (narrowest, longest) stage takes the whole list, up to enhance_stats_kernel's 1024 and 16200 frames"""
    mult = m.stages[i][5]
    ts = {2 * mult, 60 * mult} | {t for t in ENH_TS if t <= 279}
    if i == len(m.stages) - 1:
        ts |= set(ENH_TS)
    return sorted(ts)


def chunks(c, t, n):
    """clip ranges that keep a call's tensors (B, c, t) below 4 M elements"""
    step = max(1, (4 << 20) // (c * t))
    return [(lo, min(n, lo + step)) for lo in range(0, n, step)]


@pytest.mark.parametrize("cfg", ENH_CONFIGS)
def test_enhance_within_fp64_bound(cfg):
    """l3ac_op_enhance, every stage, every input kind in channel 0, within the bound of the fp64 reference on every element; pooled
    per input kind, the rms error at most 1.5 x the fp32 oracle's (T = 1: the bound only, F.instance_norm refuses one frame)."""
    m = model(cfg)
    x = enh_input(m.stages[0][2], 50, 3)[1][:4].double()
    ref = O.enhance_block(m.w64, m.stages[0][0], x)
    assert torch.allclose(enhance64(m.w64, m.stages[0][0], x)[0], ref, rtol=1e-12, atol=1e-14), f"{cfg}: enhance64 is not O.enhance_block in fp64"
    rms = Rms()
    t_start = time.time()
    for i, (eb, ub, cin, cout, scale, mult) in enumerate(m.stages):
        for t in stage_ts(m, i):
            n_kinds = len(signals(1, 0, loud=True)[0])
            worst, worst_kind, worst32, err_max, rstd_max = 0.0, "", 0.0, 0.0, 0.0
            for lo, hi in chunks(cin, t, n_kinds):
                kinds, x = enh_input(cin, t, 2000 + 31 * i + t, lo, hi)
                ref, bound, rstd = enhance64(m.w64, eb, x.double())
                got = G.from_frames(run_enhance(m, eb, G.to_frames(x)))
                ok, per_clip, err = ratio_of(got, ref, bound)
                if float(per_clip.max()) >= worst:
                    worst, worst_kind = float(per_clip.max()), kinds[int(per_clip.argmax())]
                err_max, rstd_max = max(err_max, err), max(rstd_max, rstd)
                assert ok, (f"{cfg} {eb} C={cin} T={t}: max err {err:.3e}, worst err/bound {float(per_clip.max()):.3f} at input "
                            f"'{kinds[int(per_clip.argmax())]}'")
                ref32 = O.enhance_block(m.w32, eb, x) if t > 1 else None
                if ref32 is not None:
                    worst32 = max(worst32, float(ratio_of(ref32, ref, bound)[1].max()))
                for j, kind in enumerate(kinds):
                    rms.ratio(kind, float(per_clip[j]))
                    if ref32 is not None:
                        rms.add(kind, got[j], ref32[j], ref[j])
            print(f"[{cfg} {eb} C={cin} T={t}] max err {err_max:.3e}, worst err/bound {worst:.3f} ({worst_kind}); fp32 oracle {worst32:.3f}; max 1/std {rstd_max:.1f}")
    print(f"[{cfg} enhance] {time.time() - t_start:.1f} s")
    rms.check(f"{cfg} enhance")


@pytest.mark.parametrize("cfg", ENH_CONFIGS)
def test_enhance_up_gate_evaluators(cfg):
    """l3ac_op_enhance_up on the same inputs, both routes: the rms error against fp64 at most 1.5 x the fp32 oracle's (pooled per route
    and input kind), the max error at most 2 x that of the two-call route (l3ac_op_enhance, l3ac_op_up_layer) + 1e-7 per case, and the
    profile says which evaluator of the gate ran.  Channel 0 alone is structured (see the file's docstring)."""
    m = model(cfg)
    rms = Rms()
    seen = set()
    t_start = time.time()
    for i, (eb, ub, cin, cout, scale, mult) in enumerate(m.stages):
        for t in stage_ts(m, i):
            if t < 2:  # no fp32 oracle at one frame
                continue
            n_kinds = len(signals(1, 0, loud=True)[0])
            for lo, hi in chunks(max(cin, cout * scale), t, n_kinds):
                kinds, x = enh_input(cin, t, 2000 + 31 * i + t, lo, hi)
                ref = up_ref(m.w64, ub, scale, O.enhance_block(m.w64, eb, x.double()))
                ref32 = up_ref(m.w32, ub, scale, O.enhance_block(m.w32, eb, x))
                xf = G.to_frames(x)
                for split in (True, False):
                    with Route(m, split):
                        y, how = run_enhance_up(m, eb, ub, xf, cin, cout, scale, split)
                        two = G.op_block(m.ctx, "l3ac_op_up_layer", ub, run_enhance(m, eb, xf), (xf.shape[0], t * scale, cout))
                    seen.add(how)
                    got, two = G.from_frames(y), G.from_frames(two)
                    assert torch.isfinite(got).all()
                    e_got, e_two = float((got.double() - ref).abs().max()), float((two.double() - ref).abs().max())
                    route = "bf16x3" if split else "fp32"
                    print(f"[{cfg} {eb}+{ub} {cin}->{cout} T={t} clips {lo}..{hi - 1} {route}: {how}] max err {e_got:.3e}, two calls {e_two:.3e}")
                    assert e_got <= 2.0 * e_two + 1e-7, (f"{cfg} {eb}+{ub} T={t} clips {lo}..{hi - 1} {route} ({how}): max err {e_got:.3e} > 2 x "
                                                         f"the two-call route's {e_two:.3e} + 1e-7")
                    for j, kind in enumerate(kinds):
                        rms.add(f"{route} {kind}", got[j], ref32[j], ref[j])
    print(f"[{cfg} enhance_up] {time.time() - t_start:.1f} s, gate evaluators: {sorted(seen)}")
    if cfg.startswith("1kbps"):
        assert seen == {"gate_flat_kernel", "gemm_f32_kernel<gated>"} | {f"up_fused_kernel<{a},{b}>" for a, b in UP_FUSED}, seen
    else:
        assert seen == {"gemm_f32_kernel<gated>"}, seen
    rms.check(f"{cfg} enhance_up")


@pytest.mark.parametrize("cfg", ENH_CONFIGS)
def test_enhance_statistics_are_per_clip_and_run_to_run(cfg):
    """A silent, a DC and a x100 loud clip next to noise clips: every clip of the batch is the clip alone, bit for bit
    (l3ac_op_enhance, and l3ac_op_enhance_up on both routes); a second call is the first; a small shape after a large one and back."""
    m = model(cfg)
    for i, (eb, ub, cin, cout, scale, mult) in enumerate(m.stages):
        for t in (2, 23, 257, 1025):
            g = torch.Generator().manual_seed(300 + t + i)
            x = torch.randn((5, cin, t), generator=g)
            x[1, 0], x[2, 0], x[3, 0] = 0.0, 0.3, 100.0 * x[3, 0]
            xf = G.to_frames(x)
            y = run_enhance(m, eb, xf)
            assert torch.equal(run_enhance(m, eb, xf), y), f"{cfg} {eb} T={t}: two calls differ"
            for clip in range(5):
                assert torch.equal(run_enhance(m, eb, xf[clip:clip + 1].contiguous())[0], y[clip]), f"{cfg} {eb} T={t}: clip {clip} depends on its batch"
            for split in (True, False):
                with Route(m, split):
                    y = run_enhance_up(m, eb, ub, xf, cin, cout, scale, split)[0]
                    assert torch.equal(run_enhance_up(m, eb, ub, xf, cin, cout, scale, split)[0], y), f"{cfg} {eb}+{ub} T={t} split={split}: two calls differ"
                    for clip in range(5):
                        alone = run_enhance_up(m, eb, ub, xf[clip:clip + 1].contiguous(), cin, cout, scale, split)[0]
                        assert torch.equal(alone[0], y[clip]), f"{cfg} {eb}+{ub} T={t} split={split}: clip {clip} depends on its batch"
    eb, ub, cin, cout, scale, mult = m.stages[-1]
    g = torch.Generator().manual_seed(77)
    small, large = G.to_frames(torch.randn((1, cin, 7), generator=g)), G.to_frames(torch.randn((8, cin, 4000), generator=g))
    ys, yl = run_enhance(m, eb, small), run_enhance(m, eb, large)
    assert torch.equal(run_enhance(m, eb, small), ys) and torch.equal(run_enhance(m, eb, large), yl)
    us, ul = run_enhance_up(m, eb, ub, small, cin, cout, scale, True)[0], run_enhance_up(m, eb, ub, large, cin, cout, scale, True)[0]
    assert torch.equal(run_enhance_up(m, eb, ub, small, cin, cout, scale, True)[0], us)
    assert torch.equal(run_enhance_up(m, eb, ub, large, cin, cout, scale, True)[0], ul)
