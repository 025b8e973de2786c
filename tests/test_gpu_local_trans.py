"""The LocalTrans stacks on the MI355X against an fp64 evaluation of the oracle, at window, tile and softmax edges: trans_stack_kernel
(kernels/trans_stack.hip: its three wave-count instantiations, each in the one-workgroup and the cooperative form), the layered route
with attention_mfma_kernel<64 / 128 / 192> or the scalar attention_kernel<DH> (kernels/attention.hip) between the LayerNorm rows
(kernels/rows.hip) and the GEMMs, and the distance-bias table (network.hip).  Everything goes through l3ac_op_local_trans.

Method.  No absolute tolerance anywhere: the yardstick is the fp32 CPU oracle's OWN error against the same fp64 reference.
* Reference: O.local_trans on the folded fp32 weights and the fp32 input, both widened to fp64; on every multi-window length it is
  cross-checked against O.local_trans_dense in fp64 (max difference <= 1e-12).  Clips inside one window are evaluated with the
  window set to the clip's length (O.local_trans pads to whole windows: 750 x 1500 scores per head for a clip of one frame), which is
  cross-checked against the stack's own window in the same way; the fp32 oracle is evaluated like the reference.
* Models: 1kbps (W = 250 / 750), 3kbps (W = 400) and tests/golden/win40.toml (W = 40 / 120: many windows inside a clip, window
  boundaries inside one key tile and inside one staged chunk, whole key tiles in front of a wave's first visible key) run the stack
  kernel and the matrix-core attention (dim_head 32); refdefault (dim_head 64, W = 500) and tiny (dim_head 4, W = 8 / 16) run the
  scalar kernel.  Each 128-wide model also runs PEAKY: the q and k rows of every to_qkv.weight x 5, which takes the std of q.k from
  ~0.33 to ~8 -- online rescaling with alpha << 1 and exponentials at arguments of -30 .. -90, where the synthetic weights as they
  come leave the softmax to the distance bias alone.
* Input kinds (two different clips of each, all in one batch of 14): noise N(0,1); loud (x 100); quiet (x 1e-3: the variance, 1e-6,
  is below the LayerNorm's eps); flat (3 + 1e-2 noise across channels: 1/std ~ 100); silence (every key equal: the softmax is the
  distance bias alone); repeat (one random frame repeated); impulses (0.1 noise with frames x 30 at tile and window edges).
* Routes, each asserted from the launch profile: "coop" (trans_stack_kernel<coop>, the batch being <= 32), "single"
  (trans_stack_kernel, option trans_coop = 0), "layered" (attention_kernel present, no trans_stack_kernel: frames > window or > 192,
  or a model the stack kernel does not take), and "fp32" (set_gemm_split(False): the layered route on the exact fp32 GEMM, at every
  length of the en_decoder stacks, as a third instrument).  Both attention kernels carry the profile name attention_kernel: which one
  ran follows from the shape by launch_attention's own rule (dim_head 32: the matrix-core kernel with KC = 64 up to 64 frames, 192
  for 129 .. 192 frames, else 128; any other dim_head: the scalar kernel), restated here as kc_of() and held by
  test_every_kernel_form_is_reached.
* Yardstick (test_error_against_fp64_within_the_oracles_own): per (model, weights, stack, route, input kind), pooled over the
  lengths, the GPU's rms error against fp64 may not exceed 2 x the fp32 oracle's (the factor of test_local_trans_stack_kernel), and
  for the well-conditioned kinds (noise, loud, silence, repeat, impulses) its maximum error may not exceed 4 x the oracle's maximum
  (not derived: twice the rms factor, because a maximum over differently ordered sums scatters more).  flat and quiet get the rms
  check only: their errors are the LayerNorm's conditioning times a rounding, with a heavy tail.
* Bit-for-bit properties: causality at cut points around the tiles and the window (frames after the cut replaced: the frames up to
  it keep their bits, some later frame changes); the look-back reach of a stack of depth d (window 0 replaced: every frame from
  (d + 1) W on keeps its bits, window 1 changes); cooperative == one-workgroup form, a clip alone == the clip in a batch of 40, the
  batch reversed gives the outputs reversed, two launches agree -- on every input kind, peaky weights where the model has them.

Observed on the MI355X (every pool prints its figures: "ratio" = the GPU's error over the fp32 oracle's; ranges are over the stacks of
a model and the seven input kinds, rms error | max error of the well-conditioned kinds).  No pool came near its factor and no bit-for-bit
property failed on the first build it ran on: the kernels are unchanged.
* stack kernel (coop and single give the same bits, so the same figures): 1kbps 0.52 .. 1.07 | 0.48 .. 1.21; 1kbps-peaky 0.52 .. 1.00 |
  0.47 .. 1.00; 3kbps 0.61 .. 1.08 | 0.51 .. 1.30; 3kbps-peaky 0.60 .. 1.00 | 0.54 .. 1.00; win40 0.44 .. 1.08 | 0.44 .. 1.21; win40-peaky
  0.44 .. 1.03 | 0.46 .. 1.00.  (Mostly BELOW the oracle: partial tiles accumulated from zero and added once.)
* layered, bf16x3: 1kbps 0.78 .. 1.34 | 0.90 .. 1.92 (repeat, down_trans); 1kbps-peaky 0.77 .. 1.35 | 0.58 .. 1.92; 3kbps 0.84 .. 1.26 |
  0.97 .. 1.42; 3kbps-peaky 0.76 .. 1.26 | 0.94 .. 1.45; win40 0.63 .. 1.41 (quiet, down_trans) | 0.87 .. 1.50; win40-peaky 0.76 .. 1.37 |
  0.60 .. 1.20; refdefault 0.59 .. 1.46 (silence) | 0.97 .. 1.68; tiny 0.59 .. 1.06 | 0.73 .. 1.48.
* layered, exact fp32 (en_decoder stacks): 1kbps 0.81 .. 1.24 | 0.88 .. 1.71; 1kbps-peaky 0.78 .. 1.24 | 0.61 .. 1.42; 3kbps 1.00 .. 1.26 |
  1.03 .. 1.43; 3kbps-peaky 0.81 .. 1.27 | 0.95 .. 1.49; win40 0.62 .. 1.32 | 1.00 .. 1.42; win40-peaky 0.76 .. 1.34 | 0.68 .. 1.43;
  refdefault 0.67 .. 1.38 | 0.97 .. 1.58; tiny 0.59 .. 1.02 | 0.89 .. 1.38.
* per kind over everything: noise 0.70 .. 1.34 | 0.44 .. 1.67; loud 1.00 | 0.94 .. 1.07 (both errors are the residual's rounding at
  |x| ~ 100: this kind watches for overflow and a lost scale, not for rounding); quiet 0.59 .. 1.41; flat 0.59 .. 1.07; silence
  0.44 .. 1.46 | 0.46 .. 1.66; repeat 0.61 .. 1.38 | 0.51 .. 1.92; impulses 0.65 .. 1.41 | 0.52 .. 1.71.
* absolute errors: mild weights, GPU rms 4.5e-8 (silence) .. 8e-6 (loud, flat), max 7.7e-5; the oracle rms 6.5e-8 .. 9e-6, max 8.6e-5.
  Peaky weights on flat: GPU rms up to 1.4e-4, max 2.4e-3; the oracle up to 1.8e-4, max 4.1e-3 (1/std ~ 100 into a softmax at score
  std ~ 8).
* pool sizes: 3.3e5 .. 8.3e5 elements for 1kbps, 9.2e4 .. 5.8e5 for 3kbps, 4.5e5 for refdefault; the shortest are the stack-kernel lengths
  of win40's W = 40 stacks (5.8e4) and tiny (1.4e4, dim 16) -- their max ratios stayed at or below 1.5 all the same.
* wall time of the file (42 tests): 94 s inside pytest, of which the 1kbps W = 750 stacks take 8 .. 17 s each and the 3kbps depth-3 stack
  6 s -- almost all of it the CPU oracle in fp64 and fp32 at 751, 900 and 1600 frames (padded to 1500, 1200 and 2250), which the list of
  lengths asks for; every other case is 0.1 .. 3 s, and all GPU work of the file is a few seconds.
"""
import gc
import math
import time

import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi, weights as W
from oracle import l3ac_oracle as O
from tests import gpu_ops as G
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

CONFIGS = {  # name -> (config, synthetic seed)
    "1kbps": ("1kbps", 0),
    "3kbps": ("3kbps", 0),
    "win40": (GOLDEN / "win40.toml", 3),
    "refdefault": (GOLDEN / "refdefault.toml", 0),
    "tiny": (GOLDEN / "tiny.toml", 3),
}
WIDE = ("1kbps", "3kbps", "win40")  # feature_dim 128, dim_head 32: the stack kernel and the matrix-core attention; each also runs peaky
VARIANTS = [(name, peaky) for name in CONFIGS for peaky in ((False, True) if name in WIDE else (False,))]
PEAKY_GAIN = 5.0
KINDS = ("noise", "loud", "quiet", "flat", "silence", "repeat", "impulses")
WELL_CONDITIONED = ("noise", "loud", "silence", "repeat", "impulses")
CLIPS = 2  # clips per input kind
RMS_FACTOR, MAX_FACTOR = 2.0, 4.0
COOP_BATCH = 8  # clips per cooperative launch of this file
STACK_MAX_FRAMES = 192  # trans_stack_supported: frames <= 192 and <= window, dim 128, dim_head 32

# lengths per (model, window): where the kernels change form
LENGTHS = {
    ("win40", 40): (1, 2, 15, 16, 17, 31, 32, 33, 39, 40,                      # stack kernel, 4-wave form
                    41, 47, 48, 63, 64,                                         # layered: <64>, two windows
                    65, 79, 80, 81, 96, 97, 119, 120, 121, 127, 128,            # <128>; from query 96 on the tile skip is live
                    129, 159, 160, 161, 191, 192,                               # <192>
                    193, 200, 255, 256, 257, 300),                              # several workgroups, jlo > 0
    ("win40", 120): (1, 16, 17, 63, 64, 65, 119, 120,                           # stack kernel, 4- and 8-wave forms
                     121, 128, 129, 191, 192, 193, 239, 240, 241, 360, 361, 400),
    ("1kbps", 250): (1, 63, 64, 65, 127, 128, 129, 177, 180, 191, 192, 193, 250, 251, 600),
    ("1kbps", 750): (1, 63, 64, 65, 127, 128, 129, 177, 180, 191, 192, 193, 250, 251, 600, 751, 1600),
    ("3kbps", 400): (167, 192, 193, 400, 401, 900),
    ("tiny", 8): (5, 8, 9, 16, 17, 63, 64, 65, 70, 130),
    ("tiny", 16): (5, 8, 9, 16, 17, 63, 64, 65, 70, 130),
    ("refdefault", 500): (1, 63, 64, 65, 180, 501),
}
# lengths of the bit-for-bit tests: one per wave-count form of the stack kernel, one per KC of the layered route, several workgroups
EXACT_LENGTHS = {
    ("win40", 40): (33, 40, 64, 97, 128, 192, 300),
    ("win40", 120): (17, 65, 120, 192, 241, 400),
    ("1kbps", 250): (63, 128, 177, 251, 600),
    ("1kbps", 750): (64, 100, 192, 600, 1600),
    ("3kbps", 400): (167, 401, 900),
    ("tiny", 8): (9, 17, 70),
    ("tiny", 16): (16, 65, 130),
    ("refdefault", 500): (65, 180, 501),
}
LOOK_BACK = (  # (model, stack, window, depth, frames): window 0 replaced, frames >= (depth + 1) * window keep their bits
    ("win40", "en_decoder.local_trans", 40, 3, 250),
    ("win40", "en_encoder.local_trans", 40, 2, 200),
    ("win40", "en_encoder.down_trans.trans", 120, 1, 300),
    ("win40", "en_decoder.up_trans.trans", 120, 2, 400),
    ("1kbps", "en_decoder.local_trans", 250, 3, 1100),
)


def stacks_of(mc):
    """(name, window, depth) of every LocalTrans stack, as oracle.en_encoder / en_decoder wire them"""
    if mc.compressed:
        win, r = mc.en_coder_window_size + mc.en_coder_cache_size, mc.en_coder_compress_rate
        return [("en_encoder.down_trans.trans", win * r, 1), ("en_encoder.local_trans", win, 2),
                ("en_decoder.local_trans", win, mc.en_coder_depth - 2), ("en_decoder.up_trans.trans", win * r, 2)]
    return [("en_encoder.local_trans", mc.en_coder_window_size, 1), ("en_decoder.local_trans", mc.en_coder_window_size, mc.en_coder_depth)]


class Model:
    """One config and weight variant: the codec, the fp32 folded transformer weights and their fp64 copies; the context on demand."""

    def __init__(self, name, peaky):
        cfg, seed = CONFIGS[name]
        self.name, self.peaky = name, peaky
        self.label = f"{name}{'-peaky' if peaky else ''}"
        self.codec = l3ac_amd.get_model(cfg, synthetic_seed=seed)
        if peaky:
            sds = self.codec.network.state_dicts()
            n = 0
            for sd in sds.values():
                for k in sd:
                    if ".layers." in k and k.endswith(".0.to_qkv.weight"):
                        inner = sd[k].shape[0] // 3
                        sd[k] = sd[k].clone()
                        sd[k][:2 * inner] *= PEAKY_GAIN  # rows [0, 2 inner): q and k
                        n += 1
            assert n > 0
            self.codec.network.load_state_dicts(sds)
        self.mc = mc = self.codec.network.mc
        self.dim = mc.feature_dim
        self.stacks = stacks_of(mc)
        folded = W.folded_weights(self.codec.network.state_dicts())
        self.w32 = {k: v for k, v in folded.items() if any(k.startswith(s + ".") for s, _, _ in self.stacks)}
        self.w64 = {k: v.double() for k, v in self.w32.items()}
        self.dh = self.w32[f"{self.stacks[0][0]}.layers.0.0.to_qkv.weight"].shape[0] // 3 // O.HEADS
        self._ctx = None

    @property
    def ctx(self):
        if self._ctx is None:
            self.codec.network.to(device="cuda").eval()
            self._ctx = self.codec.network.context()
        return self._ctx

    def release(self):
        if self._ctx is not None:
            self._ctx = None
            self.codec.network.cpu()  # closes the context

    def stack(self, name):
        return next(s for s in self.stacks if s[0] == name)

    def takes_stack_kernel(self, window, frames):
        """use_trans_stack's rule on the split route"""
        return self.dim == 128 and self.dh == 32 and frames <= min(window, STACK_MAX_FRAMES)


_MODELS = {}


def model(name, peaky=False):
    """The Model, its context being the only live one of this file: a context keeps the CUs its cooperative launches claimed (six per
    clip of its largest batch) until it is closed, and a launch whose claim no longer fits the device quietly takes the one-workgroup
    form -- which run() would report as the wrong route."""
    for key, other in _MODELS.items():
        if key != (name, peaky):
            other.release()
    if (name, peaky) not in _MODELS:
        _MODELS[(name, peaky)] = Model(name, peaky)
    return _MODELS[(name, peaky)]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the contexts (and the CUs their cooperative launches claimed) go when this file is done"""
    yield
    for m in _MODELS.values():
        m.release()
    _MODELS.clear()
    gc.collect()


def kc_of(frames):
    """launch_attention's rule for dim_head 32: keys per staged chunk = queries per workgroup of attention_mfma_kernel<KC>"""
    return 64 if frames <= 64 else (192 if 128 < frames <= 192 else 128)


def stack_form(frames):
    """launch_trans_stack's rule: computing waves (two per 32 frames, at least 4) -> the instantiation for at most 4 / 8 / 12"""
    waves = max(4, 2 * -(-frames // 32))
    return 4 if waves <= 4 else (8 if waves <= 8 else 12)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def impulse_frames(t, window):
    return sorted({p for p in (0, 15, 16, 31, 32, 63, 64, window - 1, window, 2 * window - 1, 2 * window, t - 1) if 0 <= p < t})


def inputs(t, dim, window, seed):
    """(len(KINDS) * CLIPS, t, dim) fp32: clips CLIPS k .. CLIPS k + CLIPS - 1 are of kind KINDS[k], each from noise of its own"""
    g = torch.Generator().manual_seed(seed)
    noise = lambda: torch.randn((CLIPS, t, dim), generator=g)
    x = {"noise": noise(), "loud": 100.0 * noise(), "quiet": 1e-3 * noise(), "flat": 3.0 + 1e-2 * noise(),
         "silence": torch.zeros((CLIPS, t, dim)), "repeat": noise()[:, :1].expand(CLIPS, t, dim).clone()}
    imp = 0.1 * noise()
    imp[:, impulse_frames(t, window)] *= 30.0
    x["impulses"] = imp
    return torch.cat([x[k] for k in KINDS]).float().contiguous()


def kind_slice(kind):
    k = KINDS.index(kind)
    return slice(CLIPS * k, CLIPS * (k + 1))


def replaced(x, lo, hi, seed):
    """x with frames [lo, hi) replaced by other finite values of the same magnitude (noise at the rms of the clip's replaced part,
    never exactly the old values)"""
    g = torch.Generator().manual_seed(seed)
    y = x.clone()
    part = x[:, lo:hi]
    scale = part.pow(2).mean(dim=(1, 2), keepdim=True).sqrt().clamp(min=1e-3)
    y[:, lo:hi] = scale * torch.randn(part.shape, generator=g)
    return y


# ---- runners -----------------------------------------------------------------------------------------------------------------
def run(m, stack, x_gpu, route):
    """l3ac_op_local_trans on x (B, T, dim) on the GPU through `route`, which the launch profile must confirm; every option back in
    `finally`.  The cooperative form gets the batch in calls of at most COOP_BATCH clips (clips are independent, which
    test_forms_and_isolation_bit_for_bit holds): the context's claim stays at 6 * COOP_BATCH CUs.  -> (B, T, dim) on the CPU"""
    ctx = m.ctx
    b, t, dim = x_gpu.shape
    if route == "coop" and b > COOP_BATCH:
        return torch.cat([run(m, stack, x_gpu[i:i + COOP_BATCH].contiguous(), route) for i in range(0, b, COOP_BATCH)])
    try:
        if route == "single":
            ctx.set_option("trans_coop", 0)
        if route == "fp32":
            ctx.set_gemm_split(False)
        with _capi.profile() as prof:
            y = G.op_block(ctx, "l3ac_op_local_trans", stack, x_gpu, (b, t, dim))
    finally:
        ctx.set_option("trans_coop", 1)
        ctx.set_gemm_split(True)
    names = [e["name"] for e in prof.entries]
    fused = [n for n in names if n.startswith("trans_stack_kernel")]
    what = f"{m.label} {stack} B={b} T={t} route {route}: ran {names}"
    if route == "coop":
        assert len(fused) == 1 and fused[0].startswith("trans_stack_kernel<coop> ") and "attention_kernel" not in names, what
    elif route == "single":
        assert len(fused) == 1 and fused[0].startswith("trans_stack_kernel ") and "attention_kernel" not in names, what
    else:
        assert not fused and "attention_kernel" in names, what
        if route == "fp32":
            assert not any(n.startswith("gemm_split") for n in names), what
    return y.cpu()


def routes_for(m, stack, window, t):
    """the routes a length is run on: both forms of the stack kernel where the split route takes it, else the layered route; and the
    exact-fp32 layered route for the en_decoder stacks"""
    r = ["coop", "single"] if m.takes_stack_kernel(window, t) else ["layered"]
    return r + (["fp32"] if stack.startswith("en_decoder.") else [])


class Pools:
    """per key: squared-error sums and maxima of the GPU and of the fp32 oracle against fp64"""

    def __init__(self):
        self.acc = {}

    def add(self, key, got, got32, ref):
        a = self.acc.setdefault(key, [0.0, 0.0, 0.0, 0.0, 0])
        eg, ec = (got.double() - ref).abs(), (got32.double() - ref).abs()
        a[0] += float(eg.pow(2).sum())
        a[1] += float(ec.pow(2).sum())
        a[2] = max(a[2], float(eg.max()))
        a[3] = max(a[3], float(ec.max()))
        a[4] += ref.numel()

    def check(self, label):
        bad = []
        for (route, kind), (sg, sc, mg, mc_, n) in self.acc.items():
            rg, rc = math.sqrt(sg / n), math.sqrt(sc / n)
            print(f"[{label} | {route} | {kind}] n={n}: rms gpu {rg:.3e} oracle {rc:.3e} ratio {rg / rc if rc else float('nan'):.2f}; "
                  f"max gpu {mg:.3e} oracle {mc_:.3e} ratio {mg / mc_ if mc_ else float('nan'):.2f}")
            if not rg <= RMS_FACTOR * rc:
                bad.append(f"{route} {kind}: rms error {rg:.3e} > {RMS_FACTOR} x the fp32 oracle's {rc:.3e}")
            if kind in WELL_CONDITIONED and not mg <= MAX_FACTOR * mc_:
                bad.append(f"{route} {kind}: max error {mg:.3e} > {MAX_FACTOR} x the fp32 oracle's {mc_:.3e}")
        assert not bad, f"{label}: " + "; ".join(bad)


def references(m, stack, window, depth, t):
    """-> x (14, t, dim) fp32, the fp64 reference, the fp32 oracle.  O.local_trans pads every clip to whole windows, so a clip of one
    frame under W = 750 costs 750 x 1500 scores per head: a clip inside ONE window (t <= W) is evaluated with the window set to its
    own length instead -- the same keys are visible at the same distances, only padding goes -- and that is checked against the stack's
    own window on the first noise clip (fp64, <= 1e-12).  A clip of several windows is evaluated as it is, and cross-checked against
    the dense restatement on a noise and an impulse clip (the dense score matrix is frames x frames)."""
    x = inputs(t, m.dim, window, seed=1000 * window + t)
    w_eval = min(window, t)
    ref = O.local_trans(m.w64, stack, x.double(), w_eval, depth)
    ref32 = O.local_trans(m.w32, stack, x, w_eval, depth)
    if t > window:
        pick = [kind_slice("noise").start, kind_slice("impulses").start]
        other = O.local_trans_dense(m.w64, stack, x[pick].double(), window, depth)
    else:
        pick = [kind_slice("noise").start]
        other = O.local_trans(m.w64, stack, x[pick].double(), window, depth)
    diff = float((other - ref[pick]).abs().max())
    assert diff <= 1e-12, f"{m.label} {stack} T={t}: two fp64 evaluations of the oracle differ by {diff:.3e}"
    return x, ref, ref32


# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_form_is_reached():
    """From the tables and the launchers' own rules (every run() asserts its route from the profile): the three instantiations of
    the stack kernel, attention_mfma_kernel with KC = 64, 128 and 192 each on more than one window, the tile skip, several
    workgroups with jlo > 0, and the scalar kernel at dim_head 4 and 64."""
    forms, kcs = set(), set()
    for (name, window), ts in LENGTHS.items():
        for t in ts:
            if name in WIDE and t <= min(window, STACK_MAX_FRAMES):
                forms.add(stack_form(t))
            elif name in WIDE and t > window:
                kcs.add(kc_of(t))
    assert forms == {4, 8, 12} and kcs == {64, 128, 192}
    assert set(EXACT_LENGTHS) == set(LENGTHS)
    w40 = LENGTHS[("win40", 40)]
    assert any(t >= 97 for t in w40)        # a wave whose first visible key (window of query 96 less one: 40) leaves tile 0 .. 31 unseen
    assert any(t > 2 * 128 for t in w40)    # a third workgroup of <128>: jlo = (256 // 40 - 1) * 40 > 0
    assert model("tiny").dh == 4 and model("refdefault").dh == 64 and all(model(n).dh == 32 and model(n).dim == 128 for n in WIDE)
    assert [s[1:] for s in model("win40").stacks] == [(120, 1), (40, 2), (40, 3), (120, 2)]


@pytest.mark.parametrize("name,peaky,stack_no", [(n, p, i) for n, p in VARIANTS for i in range(4 if n in ("1kbps", "win40", "tiny") else 2)],
                         ids=lambda v: str(v))
def test_error_against_fp64_within_the_oracles_own(name, peaky, stack_no):
    m = model(name, peaky)
    stack, window, depth = m.stacks[stack_no]
    pools = Pools()
    t_start = time.time()
    for t in LENGTHS[(name, window)]:
        x, ref, ref32 = references(m, stack, window, depth, t)
        assert torch.isfinite(ref32).all()
        xg = x.cuda()
        for route in routes_for(m, stack, window, t):
            got = run(m, stack, xg, route)
            assert torch.isfinite(got).all(), f"{m.label} {stack} T={t} route {route}: not finite"
            for kind in KINDS:
                s = kind_slice(kind)
                pools.add((route, kind), got[s], ref32[s], ref[s])
    print(f"[{m.label} {stack} W={window} depth={depth}] {time.time() - t_start:.1f} s")
    pools.check(f"{m.label} {stack} W={window}")


@pytest.mark.parametrize("name,peaky", [(n, n in WIDE) for n in CONFIGS], ids=lambda v: str(v))
def test_causality_bit_for_bit(name, peaky):
    """Frames after a cut replaced (finite, same magnitude, same length): every output frame up to the cut keeps its bits and some
    later frame changes -- at cuts around the 16- and 32-frame tiles, the 64-query workgroups and the window, on every route."""
    m = model(name, peaky)
    for stack, window, depth in m.stacks:
        for t in EXACT_LENGTHS[(name, window)]:
            x = torch.cat([inputs(t, m.dim, window, seed=7 * t + window)[kind_slice(k)][:1] for k in ("noise", "impulses", "flat")])
            cuts = sorted({c for c in (15, 16, 31, 32, 63, 64, window - 1, window, t - 2) if 0 <= c <= t - 2})
            if not cuts:
                continue
            for route in routes_for(m, stack, window, t):
                for c in cuts:
                    y = run(m, stack, torch.cat([x, replaced(x, c + 1, t, seed=c)]).cuda(), route)
                    base, yc = y[:3], y[3:]
                    what = f"{m.label} {stack} W={window} T={t} route {route} cut {c}"
                    assert torch.isfinite(y).all(), what
                    assert torch.equal(yc[:, :c + 1], base[:, :c + 1]), f"{what}: frames up to the cut depend on later frames"
                    assert not torch.equal(yc[:, c + 1:], base[:, c + 1:]), f"{what}: nothing changed after the cut (vacuous)"


@pytest.mark.parametrize("name,stack,window,depth,t", LOOK_BACK, ids=lambda v: str(v))
def test_look_back_reach_bit_for_bit(name, stack, window, depth, t):
    """Window 0 replaced (finite, O(1)): a stack of `depth` layers, each looking one window back, leaves every frame from
    (depth + 1) * window on with its bits; window 1 changes.  The layered route, bf16x3 and exact fp32, mild and peaky weights."""
    assert t > (depth + 1) * window
    for peaky in (False, True):
        m = model(name, peaky)
        assert m.stack(stack) == (stack, window, depth) and not m.takes_stack_kernel(window, t)
        x = torch.cat([inputs(t, m.dim, window, seed=t)[kind_slice(k)][:1] for k in ("noise", "impulses")])
        batch = torch.cat([x, replaced(x, 0, window, seed=window)]).cuda()
        for route in ("layered", "fp32"):
            y = run(m, stack, batch, route)
            a, b = y[:2], y[2:]
            what = f"{m.label} {stack} W={window} T={t} route {route}"
            assert torch.isfinite(y).all(), what
            assert torch.equal(a[:, (depth + 1) * window:], b[:, (depth + 1) * window:]), f"{what}: window 0 reaches past {depth + 1} windows"
            assert not torch.equal(a[:, window:2 * window], b[:, window:2 * window]), f"{what}: window 1 does not see window 0"


@pytest.mark.parametrize("name,peaky", [(n, n in WIDE) for n in CONFIGS], ids=lambda v: str(v))
def test_forms_and_isolation_bit_for_bit(name, peaky):
    """On every input kind (peaky weights where the model has them): the cooperative form is the one-workgroup form; a second launch
    is the first; the batch reversed gives the outputs reversed; a clip alone is the clip inside a batch of 40 (which the cooperative
    form does not take)."""
    m = model(name, peaky)
    for stack, window, depth in m.stacks:
        for t in EXACT_LENGTHS[(name, window)]:
            x = inputs(t, m.dim, window, seed=31 * t + window)  # every kind: 14 clips
            xg = x.cuda()
            what = f"{m.label} {stack} W={window} T={t}"
            fused = m.takes_stack_kernel(window, t)
            y = run(m, stack, xg, "coop" if fused else "layered")
            assert torch.isfinite(y).all(), what
            if fused:
                assert torch.equal(run(m, stack, xg, "single"), y), f"{what}: the cooperative and the one-workgroup form differ"
            assert torch.equal(run(m, stack, xg, "coop" if fused else "layered"), y), f"{what}: two launches differ"
            flipped = run(m, stack, xg.flip(0).contiguous(), "coop" if fused else "layered")
            assert torch.equal(flipped.flip(0), y), f"{what}: a clip's output depends on its place in the batch"
            if t > 700:  # (a batch of 40 of the longest clips adds nothing the shorter ones do not show)
                continue
            g = torch.Generator().manual_seed(t)
            big = torch.cat([x, torch.randn((40 - x.shape[0], t, m.dim), generator=g)]).cuda()
            yb = run(m, stack, big, "single" if fused else "layered")  # (40 clips: the one-workgroup form whatever trans_coop says)
            assert torch.equal(yb[:x.shape[0]], y), f"{what}: clips inside a batch of 40 differ from the batch of 14"
            for kind in KINDS:
                i = kind_slice(kind).start + 1
                alone = run(m, stack, xg[i:i + 1].contiguous(), "coop" if fused else "layered")
                assert torch.equal(alone[0], yb[i]), f"{what}: the {kind} clip alone differs from itself in a batch of 40"
