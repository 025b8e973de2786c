"""Clip isolation against NON-FINITE neighbours: a NaN, an Inf or an overflowing sample inside one clip of a
batch leaves every other clip, every other stream and every later call bit for bit as it was, through every block of the codec (C ABI),
the public entry points, the resamplers and the metric families (needs an MI355X: `pytest -m gpu`).

Every case is tests/poison.py's twin check: the same call on the clean batch, on the batch with some rows poisoned, and on the clean
batch again.  The reference is the call itself, so there is no tolerance; the launch profile must name the same kernels in all three
runs, and the kernel form a case is meant for.  Nothing is asserted about the poisoned rows' own values except shapes and that indices
stay inside the codebook.  The stride-4 layers of the 3kbps model, which no other block test reaches, are also compared with the oracle.

What was read in the sources before these cases first ran (none of them computes an address, a loop bound, a wait or a launch size from
an activation value): the FSQ index cast (fsq.hip: `(int32_t)idx_f` is stored, never used as an address; decode clamps what it reads);
sin_squared's range reduction (device_math.hpp: v_med3 clamp, `(int)n & 1` selects a value); STOI's keep list (stoi.hip: `v[f] >
threshold` is false for NaN, fmax drops NaN, the list holds frame numbers below the clip's frame count); the loudness gates
(loudness.hip: comparisons select summands, the counts are counts); the LPC pair sort (lpc.hip: a fixed bitonic network, `keep` is
computed from a count); the DTW walk (mcd.hip: every step lowers i or j whatever the choice bytes hold); the persistent kernels' unit
counters and tickets count tiles, not values.

Measured on an MI355X: no leak, every poisoned index in range; 53 tests, 8.3 s for the file alone, the slowest case 0.4 s.  Against a
build whose wide front end (conv_unit_wide.hip, the clip-boundary branch) read the neighbour's row and multiplied it by a 0 / 1 mask,
test_conv_unit_small[96] failed at T = 1, P1 ("clean row 1 beside poisoned rows [0, 2] differs ... and is not finite").
Kernels the launch profile named, per family (`pytest -s` prints them per case):
* stem: first_block_kernel, both forms (by batch size), strided and padded; ragged entry points: first_block_kernel<RAGGED>.
* ConvUnit: C = 24 conv_unit_split_kernel / conv_unit_ring_kernel (narrow_ring 0 / 2), fp32 route conv_unit_fused_kernel; C = 48 the same
  three; C = 96 conv_unit_wide_kernel<96> / wide_sliced_hidden + wide_sliced_out (wide_sliced 0 / 2), fp32 route conv_unit_fused_kernel<96>;
  C = 128 / 192 / 256 dwconv_ln_split_kernel + conv_unit_wide_kernel or the sliced pair; C = 8 / 32 / 512, every in-place call and the wide
  widths' fp32 route: dwconv_ln_kernel + two GEMMs (gemm_split_kernel or gemm_f32_kernel).  Large grids: C = 256 and 192 the fused kernel
  plus the sliced tail, C = 96 conv_unit_wide_kernel<96> with unit_counter 0 and 1, C = 48 both narrow kernels.
* down layers: down_exact_kernel<144,48>, <240,96> (1kbps), <192,96> (3kbps) with down_fused = 2 on both routes; GEMM + row_kernel with
  down_fused = 0 and for 96 -> 192 (gemm_split_kernel or gemm_f32_kernel).  conv_k3: gemm_f32_kernel, gemm_split_conv_kernel (128 -> 512).
* enhance: enhance_branches / enhance_stats / gate_flat kernels; up: GEMM + row_kernel<LERP,CN>; enhance_up: up_fused_kernel<256,96>,
  <96,48>, <48,24> on the bf16x3 route at scale 4, 3 and 2, the unfused chain at 512 -> 256 and on the fp32 route.
* output stage: legacy_unit_split_kernel / legacy_unit_kernel by route, head_fused_kernel.  LocalTrans: the stack kernel as cooperative
  and one-workgroup form and the layered route (1kbps, 3kbps, win40, peaky weights), layered only for refdefault and tiny.
* quantiser: fsq_kernel's profile name covers both fsq_forward128_kernel (hot) and fsq_kernel (generic): chosen by want_latents.
* entry points: the above plus trans_stack_kernel, attention_kernel (ragged), ragged_*, chunk_cut / chunk_merge, pack_stream /
  unpack_stream, stream_gather / carry / append / emit, resample_poly_kernel, resample_stream_kernel; metrics: metrics_stage / scatter /
  mel / mean, mfcc_dct, signal_metrics, the six stoi_* kernels, the loudness_* kernels with loudness_gain and apply_gain, lpc_frame and
  lpc_pair, and through evaluate also dtw_kernel and the pitch kernels."""
import gc
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import l3ac_amd
from l3ac_amd import _capi, weights as W
from oracle import l3ac_oracle as O
from tests import gpu_ops as G
from tests import poison as P
from tests import test_gpu_blocks as TB
from tests import test_gpu_local_trans as LT
from tests import test_gpu_loudness as TL
from tests import test_gpu_output_stage as TO
from tests import test_gpu_ragged as TR
from tests import test_gpu_stoi as TS
from tests import test_gpu_trend_front as TF
from tests import lpc_ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = P.PATTERNS
FORMS = {}  # case family -> kernel names the launch profile saw (printed per test: `pytest -s`)
_CODECS = {}


def codec_of(cfg, seed=0):
    """(codec, mc, folded weights, context) of a config, built once for this file."""
    key = (str(cfg), seed)
    if key not in _CODECS:
        codec = l3ac_amd.get_model(cfg, synthetic_seed=seed)
        codec.network.to(device=DEV).eval()
        _CODECS[key] = (codec, codec.network.mc, W.folded_weights(codec.network.state_dicts()))
    codec, mc, w = _CODECS[key]
    return codec, mc, w, codec.network.context()


@pytest.fixture(scope="module", autouse=True)
def _release():
    """the contexts of this file (and the CUs their cooperative launches claimed) go when it is done"""
    yield
    for m in LT._MODELS.values():
        m.release()
    LT._MODELS.clear()
    for codec, _, _ in _CODECS.values():
        codec.network.cpu()
    _CODECS.clear()
    gc.collect()


class Run:
    """A call under the launch profile: the three runs of a twin check must name the same kernels, every prefix in `want` and none in
    `never`."""

    def __init__(self, family, fn, want=(), never=()):
        self.family, self.fn, self.want, self.never, self.calls = family, fn, tuple(want), tuple(never), []

    def __call__(self, batch):
        lib = _capi.load_library()
        _capi.check(lib.l3ac_profile_begin())
        try:
            out = self.fn(batch)
            torch.cuda.synchronize()
        finally:  # (as _capi.profile, with room for every kernel name of a whole encode + decode)
            buf, n = (_capi.ProfileEntry * 512)(), _capi.C.c_int32(0)
            _capi.check(lib.l3ac_profile_end(buf, 512, _capi.C.byref(n)))
        self.calls.append(sorted(buf[i].name.decode() for i in range(n.value)))
        return out

    def check(self, what):
        names = self.calls[0]
        assert names and all(c == names for c in self.calls), f"{what}: the runs took different launch forms: {self.calls}"
        for p in self.want:
            assert any(n.startswith(p) for n in names), f"{what}: expected {p}, ran {names}"
        for p in self.never:
            assert not any(n.startswith(p) for n in names), f"{what}: {p} must not run, ran {names}"
        FORMS.setdefault(self.family, set()).update(names)


def twin(family, fn, batch, rows, pattern, what, want=(), never=(), **kw):
    run = Run(family, fn, want, never)
    out = P.twin_check(run, batch, rows, pattern, what=what, **kw)
    run.check(what)
    return out


def report(*families):
    for f in families:
        print(f"\n[poison forms] {f}: {sorted(FORMS.get(f, ()))}")


def rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def spread(b):
    return sorted({0, b // 2, b - 1})


class Option:
    """ctx.set_option(name, value) for the duration of a block; the value it had afterwards."""

    def __init__(self, ctx, name, value):
        self.ctx, self.name, self.value = ctx, name, value

    def __enter__(self):
        self.before = self.ctx.get_option(self.name)
        if self.value is not None:
            self.ctx.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.name, self.before)
        return False


class Route:
    """network.set_gemm_split(split) for the duration of a block; the route it had afterwards."""

    def __init__(self, codec, split):
        self.codec, self.split = codec, split

    def __enter__(self):
        self.before = self.codec.network.gemm_split
        self.codec.network.set_gemm_split(self.split)

    def __exit__(self, *exc):
        self.codec.network.set_gemm_split(self.before)
        return False


# ---- 1. the stem ------------------------------------------------------------------------------------------------------------------------------------
STEM_TS = (1, 46, 47, 64, 65, 257, 1000)  # test_stem_clip_isolation_and_run_to_run's sample counts


@pytest.mark.parametrize("form", ["split", "batch"])
def test_stem(form):
    codec, mc, w, ctx = codec_of("1kbps")
    for t in STEM_TS:
        b = 3 if form == "split" else 1024 // -(-t // 64) + 1
        assert TF.few(b, t) == (form == "split")
        x = (torch.rand((b, t), generator=torch.Generator().manual_seed(90 + t)) * 2 - 1).to(DEV)
        rows = [0, 2] if b == 3 else spread(b)
        for pattern in (ALL if form == "split" or t == 1000 else ("P1",)):
            twin(f"stem {form}", lambda a: G.first_block_at(ctx, a), x, rows, pattern, f"stem {form} B={b} T={t}", want=["first_block_kernel"])
    report(f"stem {form}")


def test_stem_strided_rows_and_padding():
    """audio_stride > samples with NaN between the rows, frames > samples (the zero right-padding folded into the load): both forms"""
    codec, mc, w, ctx = codec_of("1kbps")
    for s, f, stride in ((257, 257, 258), (300, 540, 1000)):
        for b in (3, 1024 // -(-f // 64) + 1):
            x = (torch.rand((b, s), generator=torch.Generator().manual_seed(s + b)) * 2 - 1).to(DEV)

            def call(a):
                buf = torch.full((b, stride), float("nan"), device=DEV)
                buf[:, :s] = a
                view = buf[:, :s]
                assert view.stride(0) == stride
                return G.first_block_at(ctx, view, s, f)

            for pattern in (ALL if b == 3 else ("P1",)):
                twin("stem strided", call, x, [0, 2] if b == 3 else spread(b), pattern, f"stem B={b} samples={s} frames={f} stride={stride}",
                     want=["first_block_kernel"])
    report("stem strided")


# ---- 2. ConvUnits -----------------------------------------------------------------------------------------------------------------------------------
UNIT_TS = (1, 15, 17, 31, 33, 47)  # both clip edges fall inside a 16- and a 32-frame tile
UNITS = {  # C -> (config, seed, block)
    8: (GOLDEN / "tiny.toml", 3, "encoder.blocks.1.0.module"), 32: (GOLDEN / "tiny.toml", 3, "decoder.blocks.1.1.module"),
    24: ("1kbps", 0, "encoder.blocks.1.0.module"), 48: ("1kbps", 0, "encoder.blocks.3.0.module"), 96: ("1kbps", 0, "encoder.blocks.5.0.module"),
    192: ("1kbps", 0, "encoder.blocks.7.1.module"), 256: ("1kbps", 0, "decoder.blocks.4.1.module"), 512: ("1kbps", 0, "decoder.blocks.1.2.module"),
    128: (GOLDEN / "refdefault.toml", 5, "decoder.blocks.4.0.module"),
}


def unit_forms(c):
    """(option, value, kernels that must run, kernels that must not) of every form of the ConvUnit at width c; None: the default form"""
    forms = [(None, None, ("dwconv_ln_kernel", "gemm_") if c in (8, 32, 512) else (), ())]  # (widths without a fused kernel: three launches)
    if c in (24, 48):
        forms += [("narrow_ring", 0, ("conv_unit_split_kernel",), ("conv_unit_ring_kernel",)),
                  ("narrow_ring", 2, ("conv_unit_ring_kernel",), ("conv_unit_split_kernel",))]
    if c in (96, 128, 192, 256):
        forms += [("wide_sliced", 0, ("conv_unit_wide_kernel",), ("wide_sliced_out_kernel",)),
                  ("wide_sliced", 2, ("wide_sliced_out_kernel", "wide_sliced_hidden_kernel"), ("conv_unit_wide_kernel",))]
    return forms


def unit_call(ctx, block, in_place=False):
    def call(x):
        b, t, c = x.shape
        if not in_place:
            return G.op_block(ctx, "l3ac_op_conv_unit", block, x, (b, t, c))
        y = x.clone()  # y == x: the in-place call takes the unfused route
        _capi.check(ctx.lib.l3ac_op_conv_unit(ctx.handle, block.encode(), y.data_ptr(), b, t, y.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return y
    return call


@pytest.mark.parametrize("c", sorted(UNITS))
def test_conv_unit_small(c):
    cfg, seed, block = UNITS[c]
    codec, mc, w, ctx = codec_of(cfg, seed)
    fam = f"conv_unit C={c}"
    for t in UNIT_TS:
        x = rand((3, t, c), 1000 + c + t)
        for split in (True, False):
            with Route(codec, split):
                for opt, val, want, never in (unit_forms(c) if split else unit_forms(c)[:1]):
                    with Option(ctx, opt or "unit_counter", val):  # (the default form: nothing is set, the option is only restored)
                        for pattern in ALL:
                            twin(f"{fam} {'bf16x3' if split else 'fp32'} {opt}={val}", unit_call(ctx, block), x, [0, 2], pattern,
                                 f"{block} C={c} T={t} split={split} {opt}={val}", want=want, never=never)
                for pattern in ALL:
                    twin(f"{fam} in place {'bf16x3' if split else 'fp32'}", unit_call(ctx, block, in_place=True), x, [0, 2], pattern,
                         f"{block} C={c} T={t} split={split} in place", never=("conv_unit_wide_kernel", "conv_unit_ring_kernel", "conv_unit_split_kernel",
                                                                                "conv_unit_fused_kernel", "wide_sliced_out_kernel"))
    report(*sorted(f for f in FORMS if f.startswith(fam + " ")))


LARGE = [  # (C, block, B, T, extra poisoned rows, (option, values), kernels that must run): the batch forms, from tests/test_gpu_blocks.py
    (256, "decoder.blocks.4.0.module", 40, 900, [36], ("wide_sliced", (1,)), ("conv_unit_wide_kernel<256>", "wide_sliced_out_kernel<256>")),
    (96, "decoder.blocks.7.0.module", 31, 2700, [], ("unit_counter", (0, 1)), ("conv_unit_wide_kernel<96>",)),
    (48, "decoder.blocks.10.0.module", 300, 97, [], ("narrow_ring", (0, 2)), ()),
    (192, "encoder.blocks.7.1.module", 200, 180, [], ("wide_sliced", (1,)), ("conv_unit_wide_kernel<192>",)),
]


@pytest.mark.parametrize("c,block,b,t,extra,option,want", LARGE, ids=[f"C{r[0]}" for r in LARGE])
def test_conv_unit_large_grid(c, block, b, t, extra, option, want):
    """One large-grid case per family, so that the batch forms run: persistent workgroups handed units by device counters, the weight
    ring re-entered, at C = 256 the sliced tail behind the full passes (rows 32 768 .. fall into clip 36)."""
    codec, mc, w, ctx = codec_of("1kbps")
    x = rand((b, t, c), 2000 + c)
    rows = sorted(set(spread(b) + extra))
    name, values = option
    for v in values:
        with Option(ctx, name, v):
            ring = {0: ("conv_unit_split_kernel",), 2: ("conv_unit_ring_kernel",)}[v] if name == "narrow_ring" else ()
            twin(f"conv_unit C={c} large grid {name}={v}", unit_call(ctx, block), x, rows, "P1", f"{block} B={b} T={t} {name}={v}", want=want + ring)
    report(*sorted(f for f in FORMS if f.startswith(f"conv_unit C={c} large")))


# ---- 3. down, k3, enhance and up layers; the 3kbps model's stride-4 forms against the oracle too --------------------------------------------------
DOWN_OUT = (1, 15, 16, 17, 33)
UP_TS = (1, 2, 13, 14, 15, 29)
K3_TS = (1, 2, 31, 33, 127, 129)
PAIRS = ((2, 3), (5, 6), (8, 9), (11, 12))


def down_ref(w, block, x_bct, s):
    r = F.conv1d(x_bct, w[f"{block}.0.weight"], w[f"{block}.0.bias"], stride=s)
    return O.channel_norm_first(r, w[f"{block}.1.weight"], w[f"{block}.1.bias"])


def up_ref(w, ub, x_bct, s):
    r = F.conv1d(x_bct, w[f"{ub}.0.weight"], w[f"{ub}.0.bias"])
    r = F.interpolate(r, scale_factor=s, mode="linear", align_corners=False)
    return O.channel_norm_first(r, w[f"{ub}.2.weight"], w[f"{ub}.2.bias"])


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
def test_down_layers(tag):
    codec, mc, w, ctx = codec_of(tag)
    for i, s in enumerate(mc.compress_rates):
        block, ci, co = f"encoder.blocks.{2 * i + 2}", mc.encoder_dims[i], mc.encoder_dims[i + 1]
        exact = (ci * s, co) in ((144, 48), (240, 96), (192, 96))  # down_exact_supported
        for t_out in DOWN_OUT:
            x = rand((3, s * t_out, ci), 3000 + ci + t_out)
            for split in (True, False):
                for fused in (0, 2):
                    with Route(codec, split), Option(ctx, "down_fused", fused):
                        call = lambda a: G.op_block(ctx, "l3ac_op_down_layer", block, a, (a.shape[0], t_out, co))
                        for pattern in ALL:
                            clean, _ = twin(f"down {tag} {ci}x{s}->{co} down_fused={fused} {'bf16x3' if split else 'fp32'}", call, x, [0, 2], pattern,
                                            f"{tag} {block} T_out={t_out} down_fused={fused} split={split}",
                                            want=("down_exact_kernel",) if fused == 2 and exact else (), never=() if fused == 2 and exact else ("down_exact_kernel",))
                        if tag == "3kbps":
                            TB._close(f"3kbps {block} T_out={t_out} down_fused={fused} split={split}", G.from_frames(clean),
                                      down_ref(w, block, x.cpu().permute(0, 2, 1), s))
    report(*sorted(f for f in FORMS if f.startswith(f"down {tag}")))


@pytest.mark.parametrize("block", ["encoder.blocks.8", "decoder.blocks.0"])
def test_conv_k3(block):
    codec, mc, w, ctx = codec_of("1kbps")
    co, ci = w[f"{block}.weight"].shape[:2]
    for t in K3_TS:
        x = rand((3, t, ci), 4000 + t)
        for split in (True, False):
            with Route(codec, split):
                for pattern in ALL:
                    twin(f"conv_k3 {ci}->{co} {'bf16x3' if split else 'fp32'}", lambda a: G.op_block(ctx, "l3ac_op_conv_k3", block, a, (3, t, co)), x, [0, 2],
                         pattern, f"{block} T={t} split={split}", want=("gemm_",))
    report(*sorted(f for f in FORMS if f.startswith(f"conv_k3 {ci}->")))


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}+{p[1]}")
def test_enhance_and_up_layers(tag, pair):
    codec, mc, w, ctx = codec_of(tag)
    k = PAIRS.index(pair)
    eb, ub = f"decoder.blocks.{pair[0]}", f"decoder.blocks.{pair[1]}"
    ci, co, s = mc.decoder_dims[k], mc.decoder_dims[k + 1], mc.decode_rates[k]
    fused = (ci, co) in TF.UP_FUSED
    for t in UP_TS:
        x = rand((3, t, ci), 5000 + ci + t)
        x_bct = x.cpu().permute(0, 2, 1)
        for split in (True, False):
            with Route(codec, split):
                route = "bf16x3" if split else "fp32"
                calls = (("enhance", lambda a: G.op_block(ctx, "l3ac_op_enhance", eb, a, (3, t, ci)), ("enhance_branches_kernel",)),
                         ("up", lambda a: G.op_block(ctx, "l3ac_op_up_layer", ub, a, (3, t * s, co)), ("row_kernel",)),
                         ("enhance_up", lambda a: G.op_block2(ctx, "l3ac_op_enhance_up", eb, ub, a, (3, t * s, co)),
                          ("up_fused_kernel",) if fused and split else ("enhance_stats_kernel", "row_kernel")))
                for name, call, want in calls:
                    for pattern in ALL:
                        clean, _ = twin(f"{name} {tag} {ci}->{co} x{s} {route}", call, x, [0, 2], pattern, f"{tag} {name} {eb}+{ub} T={t} split={split}", want=want)
                    if tag == "3kbps" and (t > 1 or name == "up"):  # (one frame: the reference's InstanceNorm1d raises)
                        e = O.enhance_block(w, eb, x_bct) if name != "up" else None
                        ref = {"enhance": lambda: e, "up": lambda: up_ref(w, ub, x_bct, s), "enhance_up": lambda: up_ref(w, ub, e, s)}[name]()
                        TB._close(f"3kbps {name} {eb}+{ub} T={t} split={split}", G.from_frames(clean), ref)
    report(*sorted(f for f in FORMS if f" {tag} {ci}->{co} x{s} " in f))


# ---- 4. the output stage ----------------------------------------------------------------------------------------------------------------------------
def test_output_stage():
    """LegacyUnits 0 .. 2, the head and the whole last block on test_output_stage_clip_isolation_and_run_to_run's lengths, both routes."""
    st = TO.stage("1kbps")
    for split in (True, False):
        route = "bf16x3" if split else "fp32"
        with TO.Route(st, split):
            for u, d in enumerate(TO.DILS):
                for t in (1, 3 * d - 1, 3 * d + 1, 257, 513 + 3 * d):
                    x = G.to_frames(TO._x(3, st.c, t, seed=500 + t, loud=1))
                    for pattern in ALL:
                        twin(f"legacy_unit {route}", lambda a: G.legacy_unit(st.ctx, u, a), x, [0, 2], pattern, f"unit {u} T={t} split={split}",
                             want=(TO.WANT[split],), never=(TO.WANT[not split],))
            for t in (1, 3, 4, 257):
                x = G.to_frames(TO._x(3, st.c, t, seed=600 + t, loud=1))
                for pre in (True, False):
                    st.ctx.set_head_pretanh(pre)
                    try:
                        for pattern in ALL:
                            twin(f"head {route}", lambda a: G.head(st.ctx, a), x, [0, 2], pattern, f"head T={t} pretanh={pre} split={split}", want=("head_fused_kernel",))
                    finally:
                        st.ctx.set_head_pretanh(False)
            for t in (1, 3, 4, 26, 28, 257, 540):
                x = G.to_frames(TO._x(3, st.c, t, seed=700 + t, loud=1))
                for pattern in ALL:
                    twin(f"last_block {route}", lambda a: G.op_plain(st.ctx, "l3ac_op_last_block", a, 3, t, (3, t)), x, [0, 2], pattern,
                         f"last_block T={t} split={split}", want=(TO.WANT[split],))
    report(*sorted(f for f in FORMS if f.split(" ")[0] in ("legacy_unit", "head", "last_block")))


# ---- 5. LocalTrans ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,peaky", [(n, n in LT.WIDE) for n in LT.CONFIGS], ids=lambda v: str(v))
def test_local_trans(name, peaky):
    """test_forms_and_isolation_bit_for_bit's configs and lengths; the stack kernel as the cooperative and as the one-workgroup form
    (trans_coop 1 / 0), the layered route beyond it.  win40: a window edge and a clip edge share a key tile."""
    m = LT.model(name, peaky)
    for stack, window, depth in m.stacks:
        for k, t in enumerate(LT.EXACT_LENGTHS[(name, window)]):
            x = LT.inputs(t, m.dim, window, seed=31 * t + window)[:3].to(DEV)  # noise, noise, loud
            routes = ("coop", "single") if m.takes_stack_kernel(window, t) else ("layered",)
            for route in routes:
                for pattern in (ALL if k == 0 else ("P1",)):  # (LT.run asserts the route from its own launch profile)
                    P.twin_check(lambda a: LT.run(m, stack, a, route), x, [0, 2], pattern, what=f"{m.label} {stack} W={window} T={t} {route}")
                FORMS.setdefault(f"local_trans {m.label}", set()).add(route)
    report(f"local_trans {m.label}")


# ---- 6. the quantiser -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_latents", [False, True], ids=["hot", "generic"])
def test_fsq_forward(want_latents):
    """1001 + 37 tokens at feat 128: rows of the same 8-lane group, wave and workgroup as a poisoned one keep their bits, and a poisoned
    row's index — a float that may be NaN, cast to int32 — stays inside the codebook."""
    codec, mc, w, ctx = codec_of("1kbps")
    dev = {k: w[f"quantizer.{k}"].to(DEV) for k in ("project_in.weight", "project_in.bias", "project_out.weight", "project_out.bias")}
    x = rand((1001 + 37, 128), 90, 2.0)
    rows = [0, 31, 32, x.shape[0] - 1]

    def call(a):
        q, idx, li, lat = G.fsq_forward(a, list(mc.levels), dev["project_in.weight"], dev["project_in.bias"], dev["project_out.weight"],
                                        dev["project_out.bias"], want_latents=want_latents)
        return {"q": q, "indices": idx, "level_indices": li}

    for pattern in ALL:
        clean, bad = twin(f"fsq {'generic' if want_latents else 'hot'}", call, x, rows, pattern, f"fsq want_latents={want_latents}", want=("fsq_kernel",))
        idx = bad["indices"][rows].cpu()
        assert bool(((idx >= 0) & (idx < mc.codebook_size)).all()), f"{pattern}: a poisoned row's index {idx.tolist()} lies outside [0, {mc.codebook_size})"
    report(f"fsq {'generic' if want_latents else 'hot'}")


# ---- 7. public entry points -------------------------------------------------------------------------------------------------------------------------
ROWS5 = [1, 3]


def audio5(n, seed=77):
    return (torch.rand((5, n), generator=torch.Generator().manual_seed(seed)) - 0.5).to(DEV)


def in_codebook(ind, rows, mc, what):
    idx = ind["indices"][rows].cpu()
    assert bool(((idx >= 0) & (idx < mc.codebook_size)).all()), f"{what}: a poisoned clip's indices leave [0, {mc.codebook_size})"


def decode_twins(codec, mc, ctx, clean, bad, pattern, what, lengths=None, decode=None, **kw):
    """decode what the encoder made of the clean and of the poisoned batch, from the indices and from the features; no index is counted bad"""
    decode = decode or codec.decode_audio
    before = ctx.bad_index_count()
    twin(f"{what} decode", lambda i: decode(indices=i, lengths=lengths, **kw), clean[1]["indices"], ROWS5, pattern, f"{what} decode from indices {pattern}",
         bad=bad[1]["indices"])
    twin(f"{what} decode", lambda q: decode(q, lengths=lengths, **kw), clean[0], ROWS5, pattern, f"{what} decode from features {pattern}", bad=bad[0])
    assert ctx.bad_index_count() == before, f"{what} {pattern}: bad_index_count moved"


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
def test_encode_decode_audio(tag):
    codec, mc, w, ctx = codec_of(tag)
    x = audio5(4000)
    for pattern in ALL:
        clean, bad = twin(f"{tag} encode_audio", codec.encode_audio, x, ROWS5, pattern, f"{tag} encode_audio", want=("first_block_kernel", "fsq_kernel"))
        in_codebook(bad[1], ROWS5, mc, f"{tag} encode_audio {pattern}")
        decode_twins(codec, mc, ctx, clean, bad, pattern, f"{tag} audio")
    report(f"{tag} encode_audio", f"{tag} audio decode")


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
def test_encode_decode_ragged_and_sample_rate(tag):
    codec, mc, w, ctx = codec_of(tag)
    pool = TR._boundary_lengths(mc)
    lens = [pool[4], pool[9], pool[1], pool[11], pool[6]]  # 2 hop + 3, the 193-frame edge, hop - 1, just under a window, half a hop under the 180-frame edge
    x = audio5(max(lens), seed=78)
    for pattern in ALL:
        clean, bad = twin(f"{tag} encode_audio lengths=", lambda a: codec.encode_audio(a, lengths=lens), x, ROWS5, pattern, f"{tag} ragged encode", extent=lens,
                          want=("first_block_kernel<RAGGED>", "fsq_kernel"))
        in_codebook(bad[1], ROWS5, mc, f"{tag} ragged encode {pattern}")
        nd = [max(k, TR._min_tok(mc)) for k in clean[1]["lengths"].tolist()]
        decode_twins(codec, mc, ctx, clean, bad, pattern, f"{tag} ragged", lengths=nd)
    x = audio5(4000, seed=79)
    for pattern in ALL:
        clean, bad = twin(f"{tag} encode_audio sample_rate=", lambda a: codec.encode_audio(a, sample_rate=48000), x, ROWS5, pattern, f"{tag} encode at 48 kHz",
                          want=("resample_poly_kernel", "fsq_kernel"))
        in_codebook(bad[1], ROWS5, mc, f"{tag} encode at 48 kHz {pattern}")
        decode_twins(codec, mc, ctx, clean, bad, pattern, f"{tag} 48 kHz", sample_rate=48000)
    report(*sorted(f for f in FORMS if f.startswith(f"{tag} encode_audio ") or f.startswith(f"{tag} ragged") or f.startswith(f"{tag} 48 kHz")))


LONG = dict(process_window=2700, prefix_tokens=3)
LONG_LENS = [9000, 4800, 7777, 6001, 8100]


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
def test_long_and_compressed(tag):
    codec, mc, w, ctx = codec_of(tag)
    x = audio5(max(LONG_LENS), seed=80)
    for pattern in ALL:
        clean, bad = twin(f"{tag} encode_long", lambda a: codec.encode_long(a, lengths=LONG_LENS, **LONG), x, ROWS5, pattern, f"{tag} encode_long", extent=LONG_LENS,
                          want=("chunk_cut_kernel", "chunk_merge_kernel", "fsq_kernel"))
        in_codebook(bad[1], ROWS5, mc, f"{tag} encode_long {pattern}")
        decode_twins(codec, mc, ctx, clean, bad, pattern, f"{tag} long", lengths=clean[1]["lengths"].tolist(), decode=codec.decode_long, **LONG)

        def there_and_back(a):
            frames = codec.compress(a, lengths=LONG_LENS, **LONG)
            audio, n = codec.decompress(frames, **LONG)
            return {"frames": [torch.frombuffer(bytearray(f), dtype=torch.uint8) for f in frames], "audio": audio, "samples": n}

        before = ctx.bad_index_count()
        twin(f"{tag} compress + decompress", there_and_back, x, ROWS5, pattern, f"{tag} compress / decompress", extent=LONG_LENS, want=("pack_", "unpack_"))
        assert ctx.bad_index_count() == before
    report(f"{tag} encode_long", f"{tag} long decode", f"{tag} compress + decompress")


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
def test_stream_sessions(tag):
    """Three streams, five pushes; stream 1 receives one poisoned packet in the middle: streams 0 and 2 equal the twin session at every
    push, and after reset([1]) stream 1 equals a fresh session."""
    codec, mc, w, ctx = codec_of(tag)
    hop = mc.hop_length
    n = 15 * hop  # half a window per push
    x = (torch.rand((3, 7 * n), generator=torch.Generator().manual_seed(81)) - 0.5).to(DEV)
    tokens = codec.encode_long(x, **LONG)[0]  # features of the clean streams: what the decoder sessions are fed
    m = tokens.shape[1] // 7

    def enc_session(a, keep=None):
        enc = codec.stream_encoder(3, **LONG)
        outs = [enc.push(a[:, k * n:(k + 1) * n].contiguous(), end=[k == 4, False, k == 4]) for k in range(5)]  # (stream 1 stays open: reset below)
        if keep is not None:
            keep.append(enc)
        return outs

    def dec_session(q, keep=None):
        dec = codec.stream_decoder(3, **LONG)
        outs = [dec.push(audio_feature=q[:, k * m:(k + 1) * m].contiguous(), end=[k == 4, False, k == 4]) for k in range(5)]
        if keep is not None:
            keep.append(dec)
        return outs

    for pattern in ALL:
        for what, session, data, step, tail in (("stream_encoder", enc_session, x, n, lambda s, a: s.push(a, lengths=[0, a.shape[1], 0], end=True)),
                                                ("stream_decoder", dec_session, tokens, m, lambda s, a: s.push(audio_feature=a, lengths=[0, a.shape[1], 0], end=True))):
            bad = data.clone()
            bad[1, 2 * step:3 * step] = P.patterns(data[1, 2 * step:3 * step])[pattern]
            sessions = []
            twin(f"{tag} {what}", lambda a: session(a, sessions), data[:, :5 * step], [1], pattern, f"{tag} {what}", bad=bad[:, :5 * step])
            # the poisoned session (the second of the three) after reset([1]) against a session that never saw the poison
            used, fresh = sessions[1], sessions[2]
            used.reset([1])
            fresh.reset([1])
            rest = data[:, 5 * step:7 * step].contiguous()
            got, ref = tail(used, rest), tail(fresh, rest)
            for (name, a), (_, b) in zip(P._as_outputs(got), P._as_outputs(ref)):
                assert a.shape == b.shape and np.array_equal(P._bits(a[1]), P._bits(b[1])) and P._finite(a[1]), f"{tag} {what} {pattern}: {name} of stream 1 after reset"
    report(f"{tag} stream_encoder", f"{tag} stream_decoder")


# ---- 8. the resamplers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(48000, 16000), (16000, 44100)])
def test_resamplers(a, b):
    """65 clips of 333 samples: two workgroups of 64 lanes = clips; rows 0, 63 and 64 poisoned.  The session in three pushes."""
    x = rand((65, 333), 82, 0.3)
    rows = [0, 63, 64]

    def session(v):
        rs = l3ac_amd.stream_resampler(65, a, b)
        return [rs.push(v[:, k * 111:(k + 1) * 111].contiguous(), end=k == 2) for k in range(3)]

    for pattern in ALL:
        twin(f"resample {a}->{b}", lambda v: l3ac_amd.resample(v, a, b), x, rows, pattern, f"resample {a} -> {b}", want=("resample_poly_kernel",))
        twin(f"stream_resampler {a}->{b}", session, x, rows, pattern, f"stream_resampler {a} -> {b}", want=("resample_stream_kernel",))
    report(f"resample {a}->{b}", f"stream_resampler {a}->{b}")


# ---- 9. the metric families that lacked the statement -----------------------------------------------------------------------------------------------
def pair_batch(ref, est, lens, pattern):
    """[B, 2, T] pairs and their poisoned version: the pattern in the REFERENCE of pair 0 and in the ESTIMATE of the last pair"""
    batch = torch.stack([ref, est], dim=1).to(DEV)
    bad = batch.clone()
    last = batch.shape[0] - 1
    bad[0, 0, :lens[0]] = P.patterns(batch[0, 0, :lens[0]])[pattern]
    bad[last, 1, :lens[last]] = P.patterns(batch[last, 1, :lens[last]])[pattern]
    return batch, bad, [0, last]


def test_stft_log_mel_and_mfcc():
    """the ragged shapes of test_ragged_batch_across_the_gemm_row_panel (40 + 60 + 28 frames: clip edges inside a 128-row GEMM panel) and
    of the cepstra's ragged case (127, 128 and 129 frames)"""
    from tests.test_gpu_metrics import signal
    n_fft, hop, n_mels = 64, 16, 8
    lens = [39 * hop + 15, 59 * hop, 27 * hop + 1]
    x = torch.zeros((3, max(lens) + 7))
    for i, n in enumerate(lens):
        x[i, :n] = signal(n, seed=128 + i)
    x = x.to(DEV)
    for pattern in ALL:
        twin("stft", lambda a: l3ac_amd.stft(a, n_fft, hop, lengths=lens), x, [0, 2], pattern, "stft", extent=lens, want=("metrics_stage_kernel",))
        twin("log_mel", lambda a: l3ac_amd.log_mel(a, 16000, n_fft, hop, n_mels, lengths=lens), x, [0, 2], pattern, "log_mel", extent=lens, want=("metrics_mel_kernel",))
    lens = [126 * 160, 127 * 160 + 159, 128 * 160]
    x = rand((3, max(lens) + 100), 83, 0.1)
    for pattern in ALL:
        twin("mfcc", lambda a: l3ac_amd.mfcc(a, n_coeffs=13, lengths=lens), x, [0, 2], pattern, "mfcc", extent=lens, want=("mfcc_dct_kernel",))
    report("stft", "log_mel", "mfcc")


def test_mel_distance_and_signal_metrics():
    from tests.test_gpu_metrics import signal
    lens = [1000, 333, 64]  # test_mel_distance_is_the_fp64_mean_of_log_mel_cells
    scales = [(64, 16, 8), (32, 8, 24), (256, 64, 20)]
    ref = torch.stack([signal(1000, 20 + i) for i in range(3)])
    est = 0.9 * ref + 0.01 * torch.randn(ref.shape, generator=torch.Generator().manual_seed(5))
    for pattern in ALL:
        batch, bad, rows = pair_batch(ref, est, lens, pattern)
        twin("mel_distance", lambda p: l3ac_amd.mel_distance(p[:, 0], p[:, 1], 16000, scales=scales, lengths=lens), batch, rows, pattern, "mel_distance", bad=bad,
             want=("metrics_mean_kernel",))
        twin("signal_metrics", lambda p: l3ac_amd.signal_metrics(p[:, 0], p[:, 1], lengths=lens), batch, rows, pattern, "signal_metrics", bad=bad,
             want=("signal_metrics_kernel",))
    report("mel_distance", "signal_metrics")


def test_stoi():
    lens, ref, est, clips = TS.ragged_batch()  # 31, 32 and 77 analysis frames, junk after every clip's end
    for pattern in ALL:
        batch, bad, rows = pair_batch(ref[:, :10000], est[:, :10000], lens, pattern)
        twin("stoi", lambda p: l3ac_amd.stoi(p[:, 0], p[:, 1], TS.RATE, lengths=lens), batch, rows, pattern, "stoi", bad=bad, want=("stoi_select_kernel", "stoi_segment_kernel"))
    report("stoi")


def test_loudness_and_normalize():
    lens, rows_, clips = TL.ragged_batch()  # fs = 8000: three, two and a bit, one and a bit seconds; junk after every clip's end
    x = rows_[:, :3 * 8000].to(DEV)
    for pattern in ALL:
        clean, _ = twin("loudness", lambda a: l3ac_amd.loudness(a, 8000, lengths=lens, return_momentary=True), x, [0, 2], pattern, "loudness", extent=lens,
                        finite=False, want=("loudness_gate_kernel",))  # (momentary is -inf after a clip's own blocks)
        assert torch.isfinite(clean["lufs"][1]) and torch.isfinite(clean["peak"][1])
        clean, _ = twin("normalize_loudness", lambda a: l3ac_amd.normalize_loudness(a, -23.0, 8000, lengths=lens), x, [0, 2], pattern, "normalize_loudness",
                        extent=lens, finite=False, want=("loudness_gain_kernel", "apply_gain_kernel"))  # (the junk after a clip's end passes through scaled)
        assert torch.isfinite(clean[0][1, :lens[1]]).all() and torch.isfinite(clean[1]["gain"][1])
    report("loudness", "normalize_loudness")


def test_lpc_metrics():
    fs, p, n, hop = 16000, 16, 100, 25
    lens = [1500, 733, 99, 100]  # test_a_pair_does_not_depend_on_...: 99 < frame: no frame at all (poisoned here); 100: exactly one
    lens = [lens[0], lens[1], lens[3], lens[2]]
    t = max(lens)
    ref = np.stack([lpc_ref.resonator(t, fs, seed=30 + i) for i in range(4)])
    est = np.stack([lpc_ref.add_noise(ref[i], 12.0, 50 + i) for i in range(4)])
    ref, est = torch.from_numpy(ref).float(), torch.from_numpy(est).float()
    for pattern in ALL:
        batch, bad, rows = pair_batch(ref, est, lens, pattern)
        twin("lpc_metrics", lambda q: l3ac_amd.lpc_metrics(q[:, 0], q[:, 1], sample_rate=fs, order=p, frame=n, hop=hop, lengths=lens), batch, rows, pattern,
             "lpc_metrics", bad=bad, want=("lpc_frame_kernel", "lpc_pair_kernel"))
    report("lpc_metrics")


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
def test_evaluate_with_every_family(tag):
    codec, mc, w, ctx = codec_of(tag)
    lens = [8000, 7000, 7500]
    tt = torch.arange(8000, dtype=torch.float64) / 16000
    g = torch.Generator().manual_seed(84)
    x = torch.stack([(0.2 * sum(torch.sin(2 * math.pi * f0 * h * tt + h) / h for h in range(1, 6)) * (1 + 0.5 * torch.sin(2 * math.pi * 3 * tt))).float()
                     for f0 in (120.0, 160.0, 210.0)]) + 0.01 * torch.randn((3, 8000), generator=g)
    x = x.to(DEV)
    call = lambda a: codec.evaluate(a, lengths=lens, intelligibility=True, loudness=True, pitch=True, mcd=True, lpc=True, **LONG)
    for pattern in ALL:
        clean, _ = twin(f"{tag} evaluate", call, x, [0, 2], pattern, f"{tag} evaluate", extent=lens, finite=False)  # (a random-weight codec's output may be unvoiced)
        for key in ("mel_distance", "mse", "stoi", "loudness_reference", "mcd_db"):
            assert torch.isfinite(clean[key][1]).all(), key
    report(f"{tag} evaluate")
