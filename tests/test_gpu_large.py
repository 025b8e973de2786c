"""The codec kernels past 2^30 and 2^31 elements (needs an MI355X: `pytest -m gpu tests/test_gpu_large.py`).

The rest of the suite never hands a kernel more than 0.79 G elements.  Here every op of the codec path runs once on a tensor of
2^31 elements and a little more, so that both boundaries -- 2^30 elements (a 32-bit BYTE offset wraps) and 2^31 elements (a signed
32-bit ELEMENT offset wraps) -- fall inside the tensor, inside a clip and away from the clip's edges.  DESIGN.md section 3.20.1 is the
audit these cases were written from: each 32-bit quantity of each kernel with the launcher condition that bounds it.

Shapes.  "Many clips": B = 5600 clips of T frames, T % 32 not in {0, 1, 31} and (B - 2) T C >= 2^31 (C = 24 -> T = 16003, 48 -> 8003,
96 -> 4003, 192 -> 2003, 256 -> 1501, 512 -> 751; for the layers that change the rate the same rule on the larger of input and
output).  "One long clip": B = 1 with T C >= 2^31 + 2^16, for the offsets INSIDE a clip.  (The issue asked for B = 2 there; two such
clips are a tensor past 2^32 elements, which it rules out of scope in the same breath, so the family is run with one clip and the
"same clip alone" comparison, which B = 1 makes empty, is left to the tail comparison below.)

Assertions per case (inputs torch.randn on the device, the output pre-filled with NaN):
1. bit equality with the same op over four consecutive slices of the batch, each under 2^30 elements, slice by slice (the project's
   batch invariance: no tolerance, every element);  for a long clip: bit equality of its last T / 4 frames with a run of those frames
   plus a halo as a clip of their own (64 frames: every op reaches less; the layered LocalTrans: 1500, cut at a multiple of 8000);
2. the fp64 oracle (oracle/l3ac_oracle.py on .double() weights) on the first clip, the last clip and the clips that contain each
   boundary with their two neighbours (long clip: 400-frame windows at the clip's ends and around both boundaries), at the tolerances
   tests/test_gpu_blocks.py uses for the op;
3. the whole output finite (no NaN left: nothing skipped) and the 4096 sentinel floats behind it untouched;
   (memory: x, y and one slice are 20 GiB; an l3ac_op_* entry also sizes the context's workspace for the call -- x0, x1, a, 4 C floats of
   hidden tensor per row -- 60 GiB at 2^31 elements, up to 78 GiB for the layered LocalTrans: a case skips only if mem_get_info shows
   less free than that, and the recorded run skipped none)
4. the kernel names of the launch profile.

The long-clip family, op by op: first_block; conv_unit as c24-split, c48-split, c96-wide, c96-wide-unsliced, c192-wide, c256-wide,
c256-wide-unsliced, c256 in place, c512-unfused -- the ring kernel (c24-ring, c48-ring) REFUSES such a clip, asserted; down_layer in both
forms (the INPUT passes 2^31); conv_k3; enhance (its InstanceNorm spans the clip: no tail comparison, the oracle takes the branch
statistics from the whole clip); legacy_unit, head, last_block; the layered LocalTrans; every up layer (l3ac_op_up_layer,
l3ac_op_enhance_up, row kernel and up_fused_kernel alike) REFUSES it, asserted: 2^31 elements of at most 256 channels are more than
2^23 output frames.  Not in the family, and why: the transformer stack kernel (at most 192 frames), fsq, gemm and snake (rows, not clips:
their many-rows cases are the long clip), resample (its own long-clip tests).

Findings of the audit, fixed before these cases first ran (each with a refusal test below, which also asks that a refused call leaves
the context's workspace as it was: the entries ask before they size it):
* conv_unit_ring_kernel takes (unsigned)(frame * C + channel) from ints inside a clip; only a comment said frames * C < 2^29.  Now
  refused (L3AC_MAX_RING_CLIP_ELEMS).
* the linear upsampling takes ATen's source position in fp32.  Up to 2^23 output frames per clip it is within half a frame of the exact
  one; past that row_kernel<LERP,...> can take frame `frames_in`, one row past the clip (past the tensor for the last clip), and
  up_fused_kernel, which picks the neighbours among the lanes of frames f - 1, f, f + 1, the wrong one -- its old guard was 2^30.  Both
  forms now refuse (L3AC_MAX_LERP_FRAMES_OUT), one predicate.
* frame numbers with a tile and a halo added are ints in the stem, dwconv_ln_kernel, the enhance kernels, the LegacyUnit and head kernels,
  and the LegacyUnit looks two grids of tiles ahead: frames <= L3AC_MAX_CLIP_FRAMES in each launcher, and in every block entry together
  with batch * frames < L3AC_MAX_ROWS, which keeps every kernel's tile count under its launcher's bound.

Not as the issue expected:
* launch_rows leaves gate_flat_kernel for row_kernel<GATE,NONE> at 2^31 float4 chunks (2^33 elements), not at 2^31 elements: within
  2^32 elements l3ac_op_enhance always runs gate_flat_kernel, whose 32-bit chunk number is bounded by that very condition.  The case
  asserts gate_flat_kernel.  The int64_t row_kernel instantiations ARE reached by size: <LERP,CN> (up layers), <PLAIN,CN> (down layer,
  "down_fused" = 0), <PLAIN,LN> (layered LocalTrans); the profile name does not carry the index type, the launcher's rule
  (any tensor >= 2^31 elements) does.
* the launchers' own tile-count bounds (2^31 - 65536 tiles of 14 - 64 frames) are out of reach of any buffer that exists; what is
  tested is the entries' batch * frames < 2^34, which implies them.
* the up layers' reference is ATen's lerp with its fp32 source positions and fp64 sums (_lerp_aten_fp32_positions, held to F.interpolate
  on fp32 data by test_up_reference_is_atens_fp32_upsampling): F.interpolate on fp64 tensors takes the positions in fp64, another
  operation at these lengths (after the norm, 512 -> 256 at 1500 output frames: 1.35e-4 from the kernels, measured).

Measured (one MI355X): this file alone 64 passed, no skip, 37.8 s; the whole GPU suite with it 813 passed, no skip,
352.8 s (the parent's 749 tests: about 316 s; its slowest test takes 29 s).  A case takes 0.0 - 0.5 s (the kernels, the fills and the
comparisons of 8.6 GB are milliseconds each) except where the CPU oracle takes seconds: the first fp64 evaluation at a width (c48-split
long clip 4.6, legacy_unit long clip 4.7, enhance_up 96 -> 48 5.5), local_trans layered 2.9 - 8.0, its long clip 1.2; encode + decode
5600 x 1 s 1.0 (workspace after l3ac_reserve(5600, 16000): 58.13 GiB, under the 64 GiB above which the issue asks for that test to
be left out).  Kernels named by the profile: first_block_kernel; conv_unit_split_kernel<24|48>; conv_unit_ring_kernel<24|48>;
conv_unit_wide_kernel<96|192|256> (+ dwconv_ln_split_kernel<192|256>); dwconv_ln_kernel + gemm_split_kernel Mx2048x512 e3 +
gemm_split_kernel_w256 Mx512x2048 e1 (C = 512, and the same pair of shapes at C = 256 in place, in clip groups of 31: M = 24032 /
48032; one long clip: M = 4194563); gemm_f32_kernel<2,false,16,true> 14924000x48x144 + row_kernel<PLAIN,CN> (down_fused 0),
down_exact_kernel<144,48>; gemm_split_conv_kernel 4205600x512x384; enhance_branches_kernel + enhance_stats_kernel + gate_flat_kernel;
gemm_* + row_kernel<LERP,CN>; up_fused_kernel<256,96|96,48|48,24>; legacy_unit_split_kernel; head_fused_kernel; row_kernel<PLAIN,LN> +
attention_kernel + gemm_*; trans_stack_kernel 50000x180; resample_poly_kernel.
Left out, and why: the B = 2 long-clip family (past 2^32 elements: run with B = 1); row_kernel<GATE,NONE> (out of reach inside 2^32
elements, above); l3ac_vq_argmin (audited, not on the codec path and not among the ops the issue lists).
"""
import gc
import math
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import l3ac_amd
from l3ac_amd import _capi, weights as W
from oracle import l3ac_oracle as O
from tests import resample_ref as R
from tests.helpers import index_mismatch_report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B30, B31 = 1 << 30, 1 << 31
BATCH = 5600
SENT, SENT_VALUE = 4096, -7.0
HALO = 64
FRAMES_OF = {24: 16003, 48: 8003, 96: 4003, 192: 2003, 256: 1501, 512: 751}  # the issue's table
GIB = float(1 << 30)
TIMES = {}


def frames_for(elems_per_frame, batch=BATCH, multiple=1):
    """Smallest T (a multiple of `multiple`) with T % 32 not in {0, 1, 31} and (batch - 2) T elems_per_frame >= 2^31."""
    t = -(-B31 // ((batch - 2) * elems_per_frame))
    t = -(-t // multiple) * multiple
    while t % 32 in (0, 1, 31):
        t += multiple
    return t


def test_shapes_of_this_file():
    """(no kernel) the many-clip shapes put both boundaries inside a clip, two clips or more from the tensor's ends"""
    for c, t in FRAMES_OF.items():
        assert t % 32 not in (0, 1, 31) and BATCH * t * c >= B31 + 2 * t * c and (BATCH // 4) * t * c < B30
        assert t >= frames_for(c)  # (the issue's table is a little above the smallest such T)
        for bound in (B30, B31):
            assert 16 * c < bound % (t * c) < (t - 16) * c, (c, t, bound)


@pytest.fixture(scope="module")
def model():
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.to(device=DEV).eval()
    w = W.folded_weights(codec.network.state_dicts())
    wd = {k: v.double() for k, v in w.items()}
    yield codec.network.context(), codec.network.mc, w, wd
    codec.network.cpu()
    gc.collect()
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs {gib:.0f} GiB of free device memory, {free / GIB:.0f} GiB are free")


def _alloc_out(shape, dtype=torch.float32):
    n = math.prod(shape)
    flat = torch.empty(n + SENT, dtype=dtype, device=DEV)
    flat[:n].fill_(float("nan") if dtype.is_floating_point else -1)
    flat[n:].fill_(SENT_VALUE)
    return flat, flat[:n].view(shape)


def _close(name, got, ref, atol, rtol):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    print(f"[{name}] max|err|={err.max().item():.3e} max|ref|={ref.abs().max().item():.3e}")
    assert (err <= bound).all(), f"{name}: max err {err.max().item():.3e} (worst excess {(err - bound).max().item():.3e})"


def _profiled(fn, want=(), never=()):
    with _capi.profile() as prof:
        fn()
        torch.cuda.synchronize()
    names = sorted(e["name"] for e in prof.entries)
    for p in want:
        assert any(n.startswith(p) for n in names), f"expected {p}, ran {names}"
    for p in never:
        assert not any(n.startswith(p) for n in names), f"{p} must not run, ran {names}"
    return names


def _boundary_clips(batch, *elems_per_clip):
    clips = {0, batch - 1}
    for e in elems_per_clip:
        for bound in (B30, B31):
            if batch * e > bound:
                clips.update(bound // e + d for d in (-1, 0, 1))
    return sorted(b for b in clips if 0 <= b < batch)


def many_clips(what, fn, x, out_clip, oracle=None, tol=None, want=(), never=(), n_slices=4, out_dtype=torch.float32):
    """fn(x_part, y_part): the op on the clips x_part [b][...] -> y_part [b][*out_clip] (both contiguous device views)."""
    t_start = time.perf_counter()
    b = x.shape[0]
    in_clip, n_out_clip = x[0].numel(), math.prod(out_clip)
    flat, y = _alloc_out((b, *out_clip), out_dtype)
    names = _profiled(lambda: fn(x, y), want, never)
    print(f"\n[large] {what}: x {tuple(x.shape)} ({x.numel() / B31:.3f} x 2^31) -> y {tuple(y.shape)} ({y.numel() / B31:.3f} x 2^31): {names}")
    assert max(x.numel(), y.numel()) >= B31 + 2 * max(in_clip, n_out_clip) or b * max(in_clip, n_out_clip) >= B30, "the case crosses no boundary"
    assert bool((flat[y.numel():] == SENT_VALUE).all()), f"{what}: wrote past the end of its output"
    step = -(-b // n_slices)
    for b0 in range(0, b, step):
        b1 = min(b, b0 + step)
        assert (b1 - b0) * max(in_clip, n_out_clip) < B30
        big = y[b0:b1]
        assert bool(torch.isfinite(big).all()) if out_dtype.is_floating_point else int(big.min()) >= 0, \
            f"{what}: clips {b0}..{b1 - 1} of the big call hold values that were never written"
        part = torch.full((b1 - b0, *out_clip), float("nan") if out_dtype.is_floating_point else -1, dtype=out_dtype, device=DEV)
        fn(x[b0:b1], part)
        torch.cuda.synchronize()
        if not torch.equal(part, big):
            bad = (part != big).flatten(1).any(1).nonzero().flatten()
            raise AssertionError(f"{what}: clips {[b0 + int(i) for i in bad[:8]]} (of {bad.numel()}) of the big call differ from the same clips "
                                 f"in a call of clips {b0}..{b1 - 1}")
        del part, big
    if oracle is not None:
        clips = _boundary_clips(b, in_clip, n_out_clip)
        _close(f"{what} clips {clips}", y[clips].cpu(), oracle(x[clips].cpu().double()), *tol)
    del flat, y
    torch.cuda.empty_cache()
    TIMES[what] = time.perf_counter() - t_start
    print(f"[large] {what}: {TIMES[what]:.1f} s")
    return names


def long_clip(what, fn, x, out_frame, oracle, tol, want=(), never=(), halo=HALO, span=400, align=1, tail=True, tail_align=1, window_oracle=None):
    """One clip x [1][T][...] whose tensor passes 2^31 elements: fn(x_part, y_part) as in many_clips; out_frame: the shape of one output
    frame.  halo: frames the op reaches back or ahead; span: frames of an oracle window; align: cuts fall on multiples of it (the
    bucketed attention; tail_align: the tail's cut); tail=False for an op that is not local in time; window_oracle(f0, f1) replaces oracle(x window) for such an op."""
    t_start = time.perf_counter()
    t = x.shape[1]
    e_in, e_out = x[0, 0].numel(), math.prod(out_frame)
    flat, y = _alloc_out((1, t, *out_frame))
    names = _profiled(lambda: fn(x, y), want, never)
    print(f"\n[large] {what}: one clip x {tuple(x.shape)} -> y {tuple(y.shape)} ({max(x.numel(), y.numel()) / B31:.3f} x 2^31): {names}")
    assert max(x.numel(), y.numel()) > B31 + (1 << 16)
    assert bool((flat[y.numel():] == SENT_VALUE).all()), f"{what}: wrote past the end of its output"
    assert bool(torch.isfinite(flat[:y.numel()]).all()), f"{what}: values that were never written"
    if tail:
        cut = (t - t // 4 - halo) // tail_align * tail_align  # the tail clip starts here; compared from cut + halo on
        tail_in = x[:, cut:].contiguous()
        part = torch.full((1, t - cut, *out_frame), float("nan"), device=DEV)
        fn(tail_in, part)
        torch.cuda.synchronize()
        assert torch.equal(part[:, halo:], y[:, cut + halo:]), f"{what}: the clip's last {t - cut - halo} frames differ from the same frames run as a clip of their own"
        del part, tail_in
    starts = {0, (t - span) // align * align}
    for e in (e_in, e_out):
        for bound in (B30, B31):
            if t * e > bound:
                starts.add((bound // e - span // 2) // align * align)
    for f0 in sorted(starts):
        f1 = t if f0 + span + align > t else f0 + span
        lo = 0 if f0 == 0 else halo
        hi = f1 - f0 if f1 == t else f1 - f0 - halo
        if window_oracle is not None:
            ref = window_oracle(f0 + lo, f0 + hi)
        else:  # the window as a clip of its own: exact `halo` frames from a cut end
            ref = oracle(x[:, f0:f1].cpu().double())[:, lo:hi]
        _close(f"{what} frames {f0 + lo}..{f0 + hi - 1}", y[:, f0 + lo:f0 + hi].cpu(), ref, *tol)
    del flat, y
    torch.cuda.empty_cache()
    TIMES[what] = time.perf_counter() - t_start
    print(f"[large] {what}: {TIMES[what]:.1f} s")
    return names


# ---- callers of the C entries: fn(x_part, y_part) ---------------------------------------------------------------------------------
def op_block(ctx, entry, *blocks):
    def fn(x, y):
        _capi.check(getattr(ctx.lib, entry)(ctx.handle, *(b.encode() for b in blocks), x.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), _stream()))
    return fn


def op_plain(ctx, entry, *lead):
    def fn(x, y):
        _capi.check(getattr(ctx.lib, entry)(ctx.handle, *lead, x.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), _stream()))
    return fn


def bct(f):
    """an oracle on (B, C, T) as a function of frame-major (B, T, C) fp64 clips"""
    return lambda x: f(x.permute(0, 2, 1)).permute(0, 2, 1)


class option:
    def __init__(self, ctx, name, value, default):
        self.args = (ctx, name, value, default)

    def __enter__(self):
        self.args[0].set_option(self.args[1], self.args[2])

    def __exit__(self, *exc):
        self.args[0].set_option(self.args[1], self.args[3])
        return False


# GiB a case on n elements needs free: x, y and one slice, and what the context's workspace may still have to grow by -- an l3ac_op_*
# call on n elements keeps x0, x1, a (n floats each), h (4 n) and yi; the workspace only grows and stays with the context
WS = lambda n: (7.2 * n * 4) / GIB  # noqa: E731


def CASE(ctx, n, ws=None):
    return 2.3 * n * 4 / GIB + 4 + max(0.0, (WS(n) if ws is None else ws) - ctx.workspace_bytes / GIB)


CONV_TOL = (5e-5, 5e-5)   # test_conv_units*, the 1kbps model
BLOCK_TOL = (2e-5, 2e-5)  # ATOL_BLOCK / RTOL_BLOCK: first block, down / k3 / enhance / up layers
LAST_TOL = (5e-5, 5e-5)   # test_last_block (the whole output stage; its parts are held to the same figure here)
TRANS_TOL = (1e-4, 1e-4)  # test_local_trans_*, the 1kbps model


# ---- many clips -------------------------------------------------------------------------------------------------------------------
def test_first_block_output_past_2_31(model):
    ctx, mc, w, wd = model
    t = FRAMES_OF[24]
    _need(2.4 * BATCH * t * 24 * 4 / GIB + 4)
    x = torch.randn(BATCH, t, device=DEV)
    fn = lambda a, y: _capi.check(ctx.lib.l3ac_op_first_block(ctx.handle, a.data_ptr(), a.shape[0], a.shape[1], y.data_ptr(), _stream()))  # noqa: E731
    many_clips("first_block", fn, x, (t, 24), lambda a: O.first_block(wd, "encoder.blocks.0", a.unsqueeze(1)).permute(0, 2, 1), BLOCK_TOL,
               want=("first_block_kernel",))


CONV_CASES = [  # (id, block, C, option or None, kernels that must run, kernels that must not)
    ("c24-split", "encoder.blocks.1.0.module", 24, ("narrow_ring", 0, 1), ("conv_unit_split_kernel<24>",), ("conv_unit_ring",)),
    ("c24-ring", "encoder.blocks.1.0.module", 24, ("narrow_ring", 2, 1), ("conv_unit_ring_kernel<24>",), ("conv_unit_split",)),
    ("c48-split", "encoder.blocks.3.0.module", 48, ("narrow_ring", 0, 1), ("conv_unit_split_kernel<48>",), ("conv_unit_ring",)),
    ("c48-ring", "encoder.blocks.3.0.module", 48, ("narrow_ring", 2, 1), ("conv_unit_ring_kernel<48>",), ("conv_unit_split",)),
    ("c96-wide", "encoder.blocks.5.0.module", 96, None, ("conv_unit_wide_kernel<96>",), ("gemm_", "dwconv_ln_kernel")),
    ("c96-wide-unsliced", "encoder.blocks.5.0.module", 96, ("wide_sliced", 0, 1), ("conv_unit_wide_kernel<96>",), ("gemm_", "wide_sliced_")),
    ("c192-wide", "encoder.blocks.7.0.module", 192, None, ("conv_unit_wide_kernel<192>", "dwconv_ln_split_kernel<192>"), ("gemm_",)),
    ("c192-wide-unsliced", "encoder.blocks.7.0.module", 192, ("wide_sliced", 0, 1), ("conv_unit_wide_kernel<192>",), ("gemm_", "wide_sliced_")),
    ("c256-wide", "decoder.blocks.4.0.module", 256, None, ("conv_unit_wide_kernel<256>", "dwconv_ln_split_kernel<256>"), ("gemm_",)),
    ("c256-wide-unsliced", "decoder.blocks.4.0.module", 256, ("wide_sliced", 0, 1), ("conv_unit_wide_kernel<256>",), ("gemm_", "wide_sliced_")),
    ("c512-unfused", "decoder.blocks.1.0.module", 512, None, ("dwconv_ln_kernel", "gemm_split_kernel"), ("conv_unit_",)),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_unit(model, case):
    ctx, mc, w, wd = model
    name, block, c, opt, want, never = case
    t = FRAMES_OF[c]
    _need(CASE(ctx, BATCH * t * c))
    x = torch.randn(BATCH, t, c, device=DEV)
    fn = op_block(ctx, "l3ac_op_conv_unit", block)
    oracle = bct(lambda a: O.conv_unit(wd, block, a))
    if opt is None:
        many_clips(f"conv_unit {name}", fn, x, (t, c), oracle, CONV_TOL, want, never)
    else:
        with option(ctx, *opt):
            many_clips(f"conv_unit {name}", fn, x, (t, c), oracle, CONV_TOL, want, never)


def test_conv_unit_c256_in_place_takes_the_unfused_route(model):
    """x == y: dwconv_ln_kernel and the two GEMMs, in clip groups of "unit_chunk_mb" (192 MB of hidden tensor: 31 clips here, 181 groups)"""
    ctx, mc, w, wd = model
    block, c, t = "decoder.blocks.4.0.module", 256, FRAMES_OF[256]
    _need(CASE(ctx, BATCH * t * c) + BATCH * t * c * 4 / GIB)
    x = torch.randn(BATCH, t, c, device=DEV)

    def fn(a, y):
        y.copy_(a)
        _capi.check(ctx.lib.l3ac_op_conv_unit(ctx.handle, block.encode(), y.data_ptr(), y.shape[0], y.shape[1], y.data_ptr(), _stream()))
    many_clips("conv_unit c256 in place", fn, x, (t, c), bct(lambda a: O.conv_unit(wd, block, a)), CONV_TOL,
               want=("dwconv_ln_kernel", "gemm_split_kernel"), never=("conv_unit_",))


@pytest.mark.parametrize("fused", (0, 2))
def test_down_layer(model, fused):
    ctx, mc, w, wd = model
    block, ci, co, s = "encoder.blocks.2", 24, 48, 6
    t = frames_for(ci, multiple=s)
    _need(CASE(ctx, BATCH * t * ci))
    x = torch.randn(BATCH, t, ci, device=DEV)

    def oracle(a):
        r = F.conv1d(a, wd[f"{block}.0.weight"], wd[f"{block}.0.bias"], stride=s)
        return O.channel_norm_first(r, wd[f"{block}.1.weight"], wd[f"{block}.1.bias"])
    with option(ctx, "down_fused", fused, 2):
        many_clips(f"down_layer down_fused={fused}", op_block(ctx, "l3ac_op_down_layer", block), x, (t // s, co), bct(oracle), BLOCK_TOL,
                   want=("down_exact_kernel<144,48>",) if fused else ("gemm_", "row_kernel<PLAIN,CN>"),
                   never=("gemm_",) if fused else ("down_exact",))


def test_conv_k3(model):
    ctx, mc, w, wd = model
    block, ci, co, t = "decoder.blocks.0", 128, 512, FRAMES_OF[512]
    _need(CASE(ctx, BATCH * t * co))
    x = torch.randn(BATCH, t, ci, device=DEV)
    many_clips("conv_k3", op_block(ctx, "l3ac_op_conv_k3", block), x, (t, co),
               bct(lambda a: F.conv1d(a, wd[f"{block}.weight"], wd[f"{block}.bias"], padding=1)), BLOCK_TOL, want=("gemm_split_conv_kernel",))


STAGES = [("decoder.blocks.2", "decoder.blocks.3", 512, 256, 5), ("decoder.blocks.5", "decoder.blocks.6", 256, 96, 3),
          ("decoder.blocks.8", "decoder.blocks.9", 96, 48, 3), ("decoder.blocks.11", "decoder.blocks.12", 48, 24, 2)]


def _lerp_aten_fp32_positions(r, s):
    """nn.Upsample(scale_factor=s, mode='linear') of r (B, C, T) fp64 as the fp32 model defines it: ATen's upsample_linear1d takes the
    source position fma(fp32(1 / s), dst + 0.5, -0.5) and the two weights in the tensor's own precision, fp32 (rows.hip SRC_LERP and
    up_fused_kernel restate that; their product and difference come out as the one fma, as in ATen's build: with two roundings this
    reference is 1.7e-4 of a sample difference away from F.interpolate at 8000 frames, with one it is F.interpolate on fp32 data to 2e-7,
    and the kernels meet it at BLOCK_TOL).  The sums here are fp64.  F.interpolate on fp64 tensors takes the positions in
    fp64 instead, another operation: its weights differ from the model's by up to an ulp of the position, ~ t 2^-24, which at these
    lengths is 3e-5 to 1e-3 of |x[i + 1] - x[i]| (measured against it after the norm, 512 -> 256 at 1500 output frames: 1.35e-4).
    test_up_reference_is_atens_fp32_upsampling holds this function to F.interpolate on fp32 data."""
    t_in = r.shape[-1]
    dst = torch.arange(t_in * s, dtype=torch.float32)
    src = (torch.tensor(1.0 / s, dtype=torch.float32).double() * (dst + 0.5).double() - 0.5).float()  # (exact in fp64, rounded once)
    src = src.clamp_min(0.0)
    i0 = src.long()
    i1 = i0 + (i0 + 1 < t_in).long()
    l1 = (src - i0.float()).clamp(0.0, 1.0)
    l0 = 1.0 - l1
    return l0.double() * r[..., i0] + l1.double() * r[..., i1]


def _up_oracle(wd, ub, s):
    def f(a):
        r = F.conv1d(a, wd[f"{ub}.0.weight"], wd[f"{ub}.0.bias"])
        return O.channel_norm_first(_lerp_aten_fp32_positions(r, s), wd[f"{ub}.2.weight"], wd[f"{ub}.2.bias"])
    return f


def test_up_reference_is_atens_fp32_upsampling():
    """(no kernel) the restated positions are ATen's, not rows.hip's: on fp32 data the reference IS F.interpolate up to the rounding of
    fp32 sums, for every scale and length this file uses -- and the fp64-position variant is not"""
    g = torch.Generator().manual_seed(3)
    for _, _, ci, co, s in STAGES:
        t = frames_for(s * co)
        r = torch.randn(2, 8, t, generator=g)
        aten = F.interpolate(r, scale_factor=s, mode="linear", align_corners=False).double()
        ours = _lerp_aten_fp32_positions(r.double(), s)
        d = (ours - aten).abs().max().item()
        assert d <= 1e-6, f"x{s}, {t} frames: {d:.3e}"  # |x| < 6: an fp32 lerp rounds by < 3 x 2^-24 x 6 = 1.1e-6
        d64 = (F.interpolate(r.double(), scale_factor=s, mode="linear", align_corners=False) - aten).abs().max().item()
        print(f"[lerp x{s}, {t} frames] reference vs ATen fp32 {d:.2e}; ATen fp64 positions vs ATen fp32 {d64:.2e}")


@pytest.mark.parametrize("stage", STAGES, ids=[f"{s[2]}to{s[3]}" for s in STAGES])
def test_enhance(model, stage):
    ctx, mc, w, wd = model
    eb, ub, ci, co, s = stage
    t = FRAMES_OF[ci]
    _need(CASE(ctx, BATCH * t * ci))
    x = torch.randn(BATCH, t, ci, device=DEV)
    many_clips(f"enhance C={ci}", op_block(ctx, "l3ac_op_enhance", eb), x, (t, ci), bct(lambda a: O.enhance_block(wd, eb, a)), BLOCK_TOL,
               want=("enhance_branches_kernel", "enhance_stats_kernel", "gate_flat_kernel"), never=("row_kernel",))


@pytest.mark.parametrize("stage", STAGES, ids=[f"{s[2]}to{s[3]}" for s in STAGES])
def test_up_layer(model, stage):
    ctx, mc, w, wd = model
    eb, ub, ci, co, s = stage
    t = frames_for(s * co)
    _need(CASE(ctx, BATCH * t * s * co))
    x = torch.randn(BATCH, t, ci, device=DEV)
    many_clips(f"up_layer {ci}->{co} x{s}", op_block(ctx, "l3ac_op_up_layer", ub), x, (t * s, co), bct(_up_oracle(wd, ub, s)), BLOCK_TOL,
               want=("gemm_", "row_kernel<LERP,CN>"), never=("up_fused",))


@pytest.mark.parametrize("stage", STAGES, ids=[f"{s[2]}to{s[3]}" for s in STAGES])
def test_enhance_up(model, stage):
    ctx, mc, w, wd = model
    eb, ub, ci, co, s = stage
    t = frames_for(s * co)
    _need(CASE(ctx, BATCH * t * s * co))
    x = torch.randn(BATCH, t, ci, device=DEV)
    up = _up_oracle(wd, ub, s)
    wide = ci == 512  # 512 -> 256: a gate pass and the split GEMM, then the row kernel; the narrower stages: up_fused_kernel
    many_clips(f"enhance_up {ci}->{co} x{s}", op_block(ctx, "l3ac_op_enhance_up", eb, ub), x, (t * s, co),
               bct(lambda a: up(O.enhance_block(wd, eb, a))), BLOCK_TOL,
               want=("gate_flat_kernel", "gemm_split_kernel", "row_kernel<LERP,CN>") if wide else (f"up_fused_kernel<{ci},{co}>",),
               never=("up_fused",) if wide else ("row_kernel", "gemm_"))


@pytest.mark.parametrize("unit", (0, 1, 2))
def test_legacy_unit(model, unit):
    ctx, mc, w, wd = model
    t, blk = FRAMES_OF[24], "decoder.blocks.13.block"
    _need(CASE(ctx, BATCH * t * 24))
    x = torch.randn(BATCH, t, 24, device=DEV)
    many_clips(f"legacy_unit {unit}", op_plain(ctx, "l3ac_op_legacy_unit", unit), x, (t, 24),
               bct(lambda a: O.legacy_unit(wd, f"{blk}.0.{unit}.module", a, (1, 3, 9)[unit])), LAST_TOL, want=("legacy_unit_split_kernel",))


def _head_oracle(wd, blk):
    def f(a):  # (B, T, C) -> (B, T)
        r = O.snake(a.permute(0, 2, 1), wd[f"{blk}.1.alpha"])
        return torch.tanh(F.conv1d(r, wd[f"{blk}.2.weight"], wd[f"{blk}.2.bias"], padding=3)).squeeze(1)
    return f


def test_head_and_last_block(model):
    """the head's INPUT passes 2^31 (its output is one float per frame); the whole output stage on the same input"""
    ctx, mc, w, wd = model
    t, blk = FRAMES_OF[24], "decoder.blocks.13.block"
    _need(CASE(ctx, BATCH * t * 24))
    x = torch.randn(BATCH, t, 24, device=DEV)
    head = _head_oracle(wd, blk)
    many_clips("head", op_plain(ctx, "l3ac_op_head"), x, (t,), head, LAST_TOL, want=("head_fused_kernel",))

    def last(a):
        r = a.permute(0, 2, 1)
        for u, d in enumerate((1, 3, 9)):
            r = O.legacy_unit(wd, f"{blk}.0.{u}.module", r, d)
        return head(r.permute(0, 2, 1))
    many_clips("last_block", op_plain(ctx, "l3ac_op_last_block"), x, (t,), last, LAST_TOL, want=("legacy_unit_split_kernel", "head_fused_kernel"))


def test_local_trans_layered_route(model):
    """T = 3001 > 192 frames: LayerNorm rows, the GEMMs, attention_kernel; 16.8 M rows x 128"""
    ctx, mc, w, wd = model
    block, window, depth, t = "en_decoder.local_trans", 250, 3, 3001
    n = BATCH * t * 128
    _need(CASE(ctx, n, (2 * n + 192 / 128 * n + 704 / 128 * n) * 4 / GIB))  # x0, x1, a [rows][192], h [rows][704]
    x = torch.randn(BATCH, t, 128, device=DEV)
    many_clips("local_trans layered", op_block(ctx, "l3ac_op_local_trans", block), x, (t, 128),
               lambda a: O.local_trans(wd, block, a, window, depth), TRANS_TOL,
               want=("row_kernel<PLAIN,LN>", "attention_kernel", "gemm_"), never=("trans_stack",))


def test_local_trans_stack_kernel_past_2_30(model):
    """trans_stack_kernel takes at most 192 frames and the entries at most 65535 clips: 2^31 elements are out of its reach, 2^30 are not"""
    ctx, mc, w, wd = model
    block, window, depth, t, b = "en_encoder.down_trans.trans", 750, 1, 180, 50000
    _need(6 * b * t * 128 * 4 / GIB + 4)
    x = torch.randn(b, t, 128, device=DEV)
    many_clips("local_trans stack", op_block(ctx, "l3ac_op_local_trans", block), x, (t, 128),
               lambda a: O.local_trans(wd, block, a, window, depth), TRANS_TOL, want=(f"trans_stack_kernel {b}x{t}",), never=("attention", "<coop>"))


def test_snake(model):
    rows, c = -(-(B31 + (1 << 20)) // 96), 96
    _need(2.3 * rows * c * 4 / GIB + 4)
    lib = _capi.load_library()
    x = torch.randn(rows, c, device=DEV) * 3.0
    al = (torch.rand(c, generator=torch.Generator().manual_seed(9)) * 3 + 0.05)
    ald = al.to(DEV)
    for mode in (0, 1):
        t0 = time.perf_counter()
        flat, y = _alloc_out((rows, c))
        _capi.check(lib.l3ac_op_snake(x.data_ptr(), y.data_ptr(), rows, c, ald.data_ptr(), mode, _stream()))
        torch.cuda.synchronize()
        assert bool((flat[y.numel():] == SENT_VALUE).all()) and bool(torch.isfinite(y).all())
        step = -(-rows // 4)
        for r0 in range(0, rows, step):
            part = torch.full_like(x[r0:r0 + step], float("nan"))
            _capi.check(lib.l3ac_op_snake(x[r0:r0 + step].data_ptr(), part.data_ptr(), part.shape[0], c, ald.data_ptr(), mode, _stream()))
            torch.cuda.synchronize()
            assert torch.equal(part, y[r0:r0 + step]), f"snake mode {mode}: rows {r0}.. differ from the same rows in a smaller call"
            del part
        for r0 in (0, B30 // c - 512, B31 // c - 512, rows - 1024):
            _close(f"snake mode {mode} rows {r0}..", y[r0:r0 + 1024].cpu(), O.snake(x[r0:r0 + 1024].cpu().double(), al.double()), 1e-6, 1e-6)
        del flat, y
        TIMES[f"snake mode {mode}"] = time.perf_counter() - t0
    torch.cuda.empty_cache()


@pytest.mark.parametrize("split", (False, True), ids=("gemm_f32", "gemm_split_f32"))
def test_gemm_row_strides_past_2_31(split):
    """m * lda and m * ldc past 2^31 at K = 32: A is the first 32 columns of rows `lda` floats apart"""
    lib = _capi.load_library()
    n, k = (192, 32) if split else (96, 32)
    lda = ldc = n
    m = -(-(B31 + (1 << 20)) // n)
    _need(2.3 * m * n * 4 / GIB + 4)
    t0 = time.perf_counter()
    g = torch.Generator().manual_seed(11)
    a = torch.randn(m, lda, device=DEV)
    wt, bias = torch.randn(n, k, generator=g) * 0.1, torch.randn(n, generator=g)
    wdev, bdev = wt.to(DEV), bias.to(DEV)
    if split:
        img = torch.empty((lib.l3ac_gemm_split_image_bytes(n, k),), dtype=torch.uint8, device=DEV)
        _capi.check(lib.l3ac_gemm_split_image(wdev.data_ptr(), n, k, img.data_ptr(), _stream()))

    def run(a_, c_):
        if split:
            _capi.check(lib.l3ac_gemm_split_f32(a_.data_ptr(), lda, img.data_ptr(), bdev.data_ptr(), c_.data_ptr(), ldc, a_.shape[0], n, k, _stream()))
        else:
            _capi.check(lib.l3ac_gemm_f32(a_.data_ptr(), lda, wdev.data_ptr(), bdev.data_ptr(), c_.data_ptr(), ldc, a_.shape[0], n, k, _stream()))
    flat, c = _alloc_out((m, ldc))
    names = _profiled(lambda: run(a, c), want=("gemm_split_kernel" if split else "gemm_f32_kernel",))
    print(f"\n[large] gemm split={split} m={m} lda={lda}: {names}")
    assert bool((flat[c.numel():] == SENT_VALUE).all()) and bool(torch.isfinite(c).all())
    step = -(-m // 4)
    for r0 in range(0, m, step):
        part = torch.full_like(c[r0:r0 + step], float("nan"))
        run(a[r0:r0 + step], part)
        torch.cuda.synchronize()
        assert torch.equal(part, c[r0:r0 + step]), f"rows {r0}.. differ from the same rows in a smaller call"
        del part
    for r0 in (0, B30 // n - 512, B31 // n - 512, m - 1024):
        a64 = a[r0:r0 + 1024, :k].cpu().double()
        ref = a64 @ wt.double().T + bias.double()
        mag = a64.abs() @ wt.abs().double().T + bias.abs().double()
        err = (c[r0:r0 + 1024].cpu().double() - ref).abs()
        print(f"[gemm split={split} rows {r0}..] max err {err.max().item():.3e}, max err / sum|a.w| {(err / mag).max().item():.3e}")
        if split:  # test_gemm_split_accuracy: max(4e-7, 1.05 x the fp32 kernel's) of sum|a||w| + |b|; the first is the tighter one
            assert (err / mag).max().item() <= 4e-7
        else:      # test_gemm_against_fp64
            assert err.max().item() <= 4e-7 * (a64.abs() @ wt.abs().double().T).max().item() + 1e-6
    del flat, c, a
    torch.cuda.empty_cache()
    TIMES[f"gemm split={split}"] = time.perf_counter() - t0


def test_fsq_forward_and_decode_16_9_m_tokens(model):
    ctx, mc, w, wd = model
    lib = _capi.load_library()
    n, feat, levels = 16_900_000, 128, list(mc.levels)
    d = len(levels)
    assert n * feat > B31 + (1 << 20)
    _need(3.6 * n * feat * 4 / GIB + 4)
    t0 = time.perf_counter()
    dev = {k: w[f"quantizer.{k}"].to(DEV) for k in ("project_in.weight", "project_in.bias", "project_out.weight", "project_out.bias")}
    lv = (_capi.C.c_int32 * d)(*levels)
    x = torch.randn(n, feat, device=DEV) * 2.0

    def forward(x_, q_, idx_, li_, lat_):
        _capi.check(lib.l3ac_fsq_forward(x_.data_ptr(), x_.shape[0], feat, lv, d, dev["project_in.weight"].data_ptr(), dev["project_in.bias"].data_ptr(),
                                         dev["project_out.weight"].data_ptr(), dev["project_out.bias"].data_ptr(), q_.data_ptr(), idx_.data_ptr(),
                                         li_.data_ptr(), lat_.data_ptr() if lat_ is not None else None, _stream()))
    qf, q = _alloc_out((n, feat))
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    li = torch.full((n, d), float("nan"), device=DEV)
    lat = torch.full((n, d), float("nan"), device=DEV)
    forward(x, q, idx, li, lat)  # the generic kernel (it stores the latents)
    torch.cuda.synchronize()
    assert bool((qf[q.numel():] == SENT_VALUE).all()) and bool(torch.isfinite(q).all()) and bool(torch.isfinite(li).all()) and bool(torch.isfinite(lat).all())
    assert int(idx.min()) >= 0 and int(idx.max()) < mc.codebook_size
    # the hot kernel (no latents) and the decode entry: the generic kernel's bits
    q2f, q2 = _alloc_out((n, feat))
    idx2, li2 = torch.full_like(idx, -1), torch.full_like(li, float("nan"))
    forward(x, q2, idx2, li2, None)
    torch.cuda.synchronize()
    assert bool((q2f[q2.numel():] == SENT_VALUE).all())
    assert torch.equal(idx2, idx) and torch.equal(li2, li) and torch.equal(q2, q), "hot and generic quantiser kernels differ"
    q2.fill_(float("nan"))
    _capi.check(lib.l3ac_fsq_decode(idx.data_ptr(), n, feat, lv, d, dev["project_out.weight"].data_ptr(), dev["project_out.bias"].data_ptr(),
                                    q2.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert bool((q2f[q2.numel():] == SENT_VALUE).all()) and torch.equal(q2, q), "to_features(indices) != q_feature"
    del q2f, q2, idx2, li2
    step = -(-n // 4)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        qs, ids, lis, lats = (torch.empty_like(t_[r0:r1]) for t_ in (q, idx, li, lat))
        forward(x[r0:r1], qs, ids, lis, lats)
        torch.cuda.synchronize()
        assert torch.equal(qs, q[r0:r1]) and torch.equal(ids, idx[r0:r1]) and torch.equal(lis, li[r0:r1]) and torch.equal(lats, lat[r0:r1]), \
            f"tokens {r0}.. differ from the same tokens in a smaller call"
        del qs, ids, lis, lats
    for r0 in (0, B30 // feat - 2048, B31 // feat - 2048, n - 4096):  # test_fsq_fused_forward_and_roundtrip, per window of 4096 tokens
        q_ref, ind_ref, lat_ref = O.quantizer(w, mc, x[r0:r0 + 4096].cpu())
        _close(f"fsq latents tokens {r0}..", lat[r0:r0 + 4096].cpu(), lat_ref, 2e-6, 2e-6)
        n_bad, ok = index_mismatch_report(idx[r0:r0 + 4096].cpu().numpy(), ind_ref["indices"].numpy(), lat_ref.numpy(), mc.levels, tau=1e-4)
        assert ok and n_bad <= 1, f"tokens {r0}..: {n_bad} index mismatches"
    del qf, q, idx, li, lat, x
    torch.cuda.empty_cache()
    TIMES["fsq"] = time.perf_counter() - t0


# ---- one long clip ----------------------------------------------------------------------------------------------------------------
def _long_frames(c):
    t = -(-(B31 + (1 << 17)) // c)
    return t + (3 if t % 32 in (0, 1, 31) else 0)


def test_long_clip_first_block(model):
    ctx, mc, w, wd = model
    t = _long_frames(24)
    _need(2.0 * t * 24 * 4 / GIB + 4)
    x = torch.randn(1, t, device=DEV)
    fn = lambda a, y: _capi.check(ctx.lib.l3ac_op_first_block(ctx.handle, a.data_ptr(), 1, a.shape[1], y.data_ptr(), _stream()))  # noqa: E731
    long_clip("first_block, one clip", fn, x, (24,), lambda a: O.first_block(wd, "encoder.blocks.0", a.unsqueeze(1)).permute(0, 2, 1), BLOCK_TOL,
              want=("first_block_kernel",))


LONG_CONV = [("c24-split", "encoder.blocks.1.0.module", 24, ("narrow_ring", 0, 1), False, ("conv_unit_split_kernel<24>",)),
             ("c48-split", "encoder.blocks.3.0.module", 48, ("narrow_ring", 0, 1), False, ("conv_unit_split_kernel<48>",)),
             ("c96-wide", "encoder.blocks.5.0.module", 96, None, False, ("conv_unit_wide_kernel<96>",)),
             ("c96-wide-unsliced", "encoder.blocks.5.0.module", 96, ("wide_sliced", 0, 1), False, ("conv_unit_wide_kernel<96>",)),
             ("c192-wide", "encoder.blocks.7.0.module", 192, None, False, ("conv_unit_wide_kernel<192>", "dwconv_ln_split_kernel<192>")),
             ("c256-wide", "decoder.blocks.4.0.module", 256, None, False, ("conv_unit_wide_kernel<256>", "dwconv_ln_split_kernel<256>")),
             ("c256-wide-unsliced", "decoder.blocks.4.0.module", 256, ("wide_sliced", 0, 1), False, ("conv_unit_wide_kernel<256>",)),
             ("c256-in-place", "decoder.blocks.4.0.module", 256, None, True, ("dwconv_ln_kernel", "gemm_split_kernel")),
             ("c512-unfused", "decoder.blocks.1.0.module", 512, None, False, ("dwconv_ln_kernel", "gemm_split_kernel"))]


@pytest.mark.parametrize("case", LONG_CONV, ids=[c[0] for c in LONG_CONV])
def test_long_clip_conv_unit(model, case):
    """offsets INSIDE a clip past 2^31: the split kernel, the wide kernel and the unfused route keep them in 64 bits (the ring kernel
    refuses such a clip: test_ring_kernel_refuses_a_clip_of_2_29_elements)"""
    ctx, mc, w, wd = model
    name, block, c, opt, in_place, want = case
    t = _long_frames(c)
    _need(CASE(ctx, t * c))
    x = torch.randn(1, t, c, device=DEV)
    fn = op_block(ctx, "l3ac_op_conv_unit", block)
    if in_place:
        def fn(a, y):
            y.copy_(a)
            _capi.check(ctx.lib.l3ac_op_conv_unit(ctx.handle, block.encode(), y.data_ptr(), 1, y.shape[1], y.data_ptr(), _stream()))
    oracle = bct(lambda a: O.conv_unit(wd, block, a))
    if opt is None:
        long_clip(f"conv_unit {name}, one clip", fn, x, (c,), oracle, CONV_TOL, want)
    else:
        with option(ctx, *opt):
            long_clip(f"conv_unit {name}, one clip", fn, x, (c,), oracle, CONV_TOL, want)


def test_long_clip_legacy_unit_head_and_last_block(model):
    ctx, mc, w, wd = model
    t, blk = _long_frames(24), "decoder.blocks.13.block"
    _need(CASE(ctx, t * 24))
    x = torch.randn(1, t, 24, device=DEV)
    long_clip("legacy_unit 2, one clip", op_plain(ctx, "l3ac_op_legacy_unit", 2), x, (24,),
              bct(lambda a: O.legacy_unit(wd, f"{blk}.0.2.module", a, 9)), LAST_TOL, want=("legacy_unit_split_kernel",))
    head = _head_oracle(wd, blk)
    long_clip("head, one clip", op_plain(ctx, "l3ac_op_head"), x, (), head, LAST_TOL, want=("head_fused_kernel",))

    def last(a):  # reaches 3 + 9 + 27 + 3 = 42 frames: inside the 64-frame halo
        r = a.permute(0, 2, 1)
        for u, d in enumerate((1, 3, 9)):
            r = O.legacy_unit(wd, f"{blk}.0.{u}.module", r, d)
        return head(r.permute(0, 2, 1))
    long_clip("last_block, one clip", op_plain(ctx, "l3ac_op_last_block"), x, (), last, LAST_TOL, want=("legacy_unit_split_kernel", "head_fused_kernel"))


@pytest.mark.parametrize("fused", (0, 2))
def test_long_clip_down_layer(model, fused):
    ctx, mc, w, wd = model
    block, ci, co, s = "encoder.blocks.2", 24, 48, 6
    t = -(-_long_frames(ci) // (32 * s)) * 32 * s + 5 * s  # whole patches of 6; output frames % 32 == 5
    _need(CASE(ctx, t * ci))
    x = torch.randn(1, t, ci, device=DEV)

    def oracle(a):
        r = F.conv1d(a, wd[f"{block}.0.weight"], wd[f"{block}.0.bias"], stride=s)
        return O.channel_norm_first(r, wd[f"{block}.1.weight"], wd[f"{block}.1.bias"])
    fn = op_block(ctx, "l3ac_op_down_layer", block)
    t_start = time.perf_counter()
    with option(ctx, "down_fused", fused, 2):  # (input and output frames differ by the stride: the helper's steps, on output frames)
        y = torch.full((1, t // s, co), float("nan"), device=DEV)
        names = _profiled(lambda: fn(x, y), want=("down_exact_kernel<144,48>",) if fused else ("gemm_", "row_kernel<PLAIN,CN>"))
        print(f"\n[large] down_layer down_fused={fused}, one clip: x {tuple(x.shape)} ({x.numel() / B31:.3f} x 2^31) -> y {tuple(y.shape)}: {names}")
        assert x.numel() > B31 + (1 << 16) and bool(torch.isfinite(y).all())
        q = (t // s) // 4
        part = torch.full((1, q, co), float("nan"), device=DEV)
        fn(x[:, t - q * s:].contiguous(), part)  # (a patch reads no neighbour: no halo)
        torch.cuda.synchronize()
        assert torch.equal(part, y[:, t // s - q:]), "the clip's last quarter differs from the same frames run as a clip of their own"
        for f0 in sorted({0, t // s - 400, B30 // (s * ci) - 200, B31 // (s * ci) - 200}):  # output frames around the INPUT's boundaries
            _close(f"down_layer down_fused={fused} output frames {f0}..{f0 + 399}", y[:, f0:f0 + 400].cpu(),
                   bct(oracle)(x[:, f0 * s:(f0 + 400) * s].cpu().double()), *BLOCK_TOL)
    del y, part, x
    torch.cuda.empty_cache()
    TIMES[f"down_layer down_fused={fused}, one clip"] = time.perf_counter() - t_start


def test_long_clip_conv_k3(model):
    ctx, mc, w, wd = model
    block, ci, co = "decoder.blocks.0", 128, 512
    t = _long_frames(co)
    _need(CASE(ctx, t * co))
    x = torch.randn(1, t, ci, device=DEV)
    long_clip("conv_k3, one clip", op_block(ctx, "l3ac_op_conv_k3", block), x, (co,),
              bct(lambda a: F.conv1d(a, wd[f"{block}.weight"], wd[f"{block}.bias"], padding=1)), BLOCK_TOL, want=("gemm_split_conv_kernel",))


def test_long_clip_enhance(model):
    """EnhanceBlock normalises its four branch signals over the WHOLE clip (InstanceNorm): no tail comparison, and the oracle takes the
    branches and their statistics from all 44.7 M frames of channel 0 in fp64, then the gate on the compared windows"""
    ctx, mc, w, wd = model
    eb, c = "decoder.blocks.11", 48
    t = _long_frames(c)
    _need(CASE(ctx, t * c))
    x = torch.randn(1, t, c, device=DEV)
    yi = O.trend_branches(wd, eb, x[:, :, 0].cpu().double().unsqueeze(1), (1, 3, 5, 9), 2)
    yi = F.instance_norm(yi, weight=wd[f"{eb}.merge_layer.0.weight"], bias=wd[f"{eb}.merge_layer.0.bias"], use_input_stats=True, eps=1e-5)

    def window(f0, f1):
        xw = x[:, f0:f1].cpu().double().permute(0, 2, 1)
        g = F.conv1d(yi[:, :, f0:f1], wd[f"{eb}.merge_layer.1.weight"], wd[f"{eb}.merge_layer.1.bias"])
        return (xw + g * xw).permute(0, 2, 1)
    long_clip("enhance C=48, one clip", op_block(ctx, "l3ac_op_enhance", eb), x, (c,), None, BLOCK_TOL,
              want=("enhance_branches_kernel", "enhance_stats_kernel", "gate_flat_kernel"), tail=False, window_oracle=window)


def test_long_clip_local_trans_layered(model):
    """16.8 M frames x 128 in one clip.  The attention is bucketed: a query sees its own window of 250 frames and the one before, by
    absolute position, so cuts fall on multiples of 250 and three layers reach 3 x 499 frames back: a halo of 1500.  The tail is cut at
    a multiple of 8000 = lcm(250, 64), so that attention_kernel's 64-query workgroups meet the buckets as they do in the whole clip"""
    ctx, mc, w, wd = model
    block, window, depth = "en_decoder.local_trans", 250, 3
    t = _long_frames(128)
    n = t * 128
    _need(CASE(ctx, n, (2 * n + 192 / 128 * n + 704 / 128 * n) * 4 / GIB))
    x = torch.randn(1, t, 128, device=DEV)
    long_clip("local_trans layered, one clip", op_block(ctx, "l3ac_op_local_trans", block), x, (128,),
              lambda a: O.local_trans(wd, block, a, window, depth), TRANS_TOL, want=("row_kernel<PLAIN,LN>", "attention_kernel", "gemm_"),
              never=("trans_stack",), halo=1500, span=3500, align=250, tail_align=8000)


# ---- refusals: a shape past a limit is refused before anything is launched AND before the workspace is sized (small real buffers) --
def _refused(ctx, call, *needles):
    """call() -> the entry's return code: L3AC_EINVAL, the message, nothing launched, the context's workspace as it was"""
    ws = ctx.workspace_bytes
    with _capi.profile() as prof:
        rc = call()
    msg = ctx.lib.l3ac_last_error().decode()
    assert rc == -1 and not prof.entries, (rc, msg, prof.entries)
    assert all(n in msg for n in needles), msg
    assert ctx.workspace_bytes == ws, f"a refused call grew the workspace: {ws} -> {ctx.workspace_bytes}"


@pytest.fixture()
def small():
    x, y = torch.zeros(64, 48, device=DEV), torch.full((64, 512), float("nan"), device=DEV)
    yield x, y
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


def test_ring_kernel_refuses_a_clip_of_2_29_elements(model, small):
    ctx, mc, w, wd = model
    x, y = small
    for block, c, ring in (("encoder.blocks.1.0.module", 24, 2), ("encoder.blocks.3.0.module", 48, 1)):  # C = 48 takes the ring kernel by default
        frames = -(-(1 << 29) // c)
        with option(ctx, "narrow_ring", ring, 1):
            _refused(ctx, lambda: ctx.lib.l3ac_op_conv_unit(ctx.handle, block.encode(), x.data_ptr(), 1, frames, y.data_ptr(), _stream()),
                     "conv_unit_ring: clip too long", "2^29", f"C={c}")


def test_up_layers_refuse_more_than_2_23_output_frames(model, small):
    """both forms: the row kernel (l3ac_op_up_layer; 512 -> 256 in l3ac_op_enhance_up) and up_fused_kernel (the narrower stages)"""
    ctx, mc, w, wd = model
    x, y = small
    for eb, ub, ci, co, s in STAGES:
        frames = (1 << 23) // s + 1
        for entry, blocks in (("l3ac_op_up_layer", (ub,)), ("l3ac_op_enhance_up", (eb, ub))):
            _refused(ctx, lambda: getattr(ctx.lib, entry)(ctx.handle, *(b.encode() for b in blocks), x.data_ptr(), 1, frames, y.data_ptr(), _stream()),
                     "more than 2^23 output frames per clip")
        # which is why no up layer has a long-clip case: one clip whose output passes 2^31 elements has more output frames than that
        assert -(-(B31 + (1 << 16)) // co) > 1 << 23


def test_first_block_refuses_frames_past_its_32_bit_frame_numbers(model):
    ctx, mc, w, wd = model
    x, y = torch.zeros(4096, device=DEV), torch.full((4096,), float("nan"), device=DEV)
    _refused(ctx, lambda: ctx.lib.l3ac_op_first_block(ctx.handle, x.data_ptr(), 1, (1 << 31) - 65535, y.data_ptr(), _stream()), "first_block", "2^31 - 65536")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


def _block_entries(ctx, x, y):
    """every entry that sizes the workspace for (batch, frames): name -> call(batch, frames)"""
    def blk(entry, *blocks):
        return lambda b, f: getattr(ctx.lib, entry)(ctx.handle, *(n.encode() for n in blocks), x.data_ptr(), b, f, y.data_ptr(), _stream())
    return {"conv_unit c24": blk("l3ac_op_conv_unit", "encoder.blocks.1.0.module"), "conv_unit c256": blk("l3ac_op_conv_unit", "decoder.blocks.4.0.module"),
            "conv_unit c512": blk("l3ac_op_conv_unit", "decoder.blocks.1.0.module"), "enhance": blk("l3ac_op_enhance", "decoder.blocks.11"),
            "legacy_unit": lambda b, f: ctx.lib.l3ac_op_legacy_unit(ctx.handle, 1, x.data_ptr(), b, f, y.data_ptr(), _stream()),
            "head": lambda b, f: ctx.lib.l3ac_op_head(ctx.handle, x.data_ptr(), b, f, y.data_ptr(), _stream()),
            "last_block": lambda b, f: ctx.lib.l3ac_op_last_block(ctx.handle, x.data_ptr(), b, f, y.data_ptr(), _stream())}


def test_block_entries_refuse_frames_and_rows_past_the_32_bit_frame_and_tile_numbers(model, small):
    """dwconv_ln_kernel, the enhance kernels, the LegacyUnit and head kernels add a tile and a halo to an int frame number, and every fused
    kernel numbers its tiles (14 frames and more) in 32 bits: the entries ask frames <= 2^31 - 65536 and batch * frames < 2^34 first"""
    ctx, mc, w, wd = model
    x, y = small
    for name, call in _block_entries(ctx, x, y).items():
        _refused(ctx, lambda: call(1, (1 << 31) - 65535), "frames per clip", "2^31 - 65536")
        _refused(ctx, lambda: call(65535, (1 << 18) + 8), "batch * frames", "2^34")


# ---- sample-rate conversion --------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -24


def _polyphase_ref(x_dev, a, b, m_lo, m_hi):
    """fp64 y[m] and sum|h x| for m_lo <= m < m_hi of ONE clip x_dev (n,) from resample.hip's header formula, on the input span they read"""
    up, down = R.factors(a, b)
    half_len = 10 * max(up, down)
    _, K, bank = R.polyphase_taps(a, b)
    n = x_dev.shape[0]
    m = np.arange(m_lo, m_hi, dtype=np.int64)
    q = m * down + half_len
    xi = (q // up)[:, None] - np.arange(K)[None, :]
    lo, hi = max(int(xi.min()), 0), min(int(xi.max()) + 1, n)
    xs = x_dev[lo:hi].cpu().double().numpy()
    ok = (xi >= 0) & (xi < n)
    prod = bank[q % up] * np.where(ok, xs[np.clip(xi, lo, hi - 1) - lo], 0.0)
    return prod.sum(-1), np.abs(prod).sum(-1), K


@pytest.mark.parametrize("a,b", [(192000, 44100), (44100, 48000)])
def test_resample_long_clip_across_the_64_bit_division(a, b):
    """resample_poly_kernel divides m down + half_len by `up` in 32 bits while it fits and in 64 bits past 2^31 - 1: outputs on both sides"""
    up, down = R.factors(a, b)
    half_len = 10 * max(up, down)
    m_cross = -(-(B31 - half_len) // down)  # the first output on the 64-bit branch
    n_out = m_cross + 6000
    n_in = n_out * down // up  # ceil(n_in up / down) == n_out or n_out - 1 ... taken from the library below
    t0 = time.perf_counter()
    x = torch.randn(1, n_in, device=DEV) * 0.3
    with _capi.profile() as prof:
        y = l3ac_amd.resample(x, a, b)
        torch.cuda.synchronize()
    n_out = y.shape[1]
    assert [e["name"] for e in prof.entries] == ["resample_poly_kernel"] and n_out == R.out_length(a, b, n_in) and n_out >= m_cross + 4000
    assert (m_cross - 1) * down + half_len <= B31 - 1 < m_cross * down + half_len
    assert bool(torch.isfinite(y).all())
    windows = [(m_cross - 2000, m_cross + 2000), (n_out - 2000, n_out)]
    for m_lo, m_hi in windows:
        ref, absdot, K = _polyphase_ref(x[0], a, b, m_lo, m_hi)
        err = np.abs(y[0, m_lo:m_hi].cpu().double().numpy() - ref)
        bound = (K + 2) * EPS * absdot
        print(f"\n[resample {a}->{b} outputs {m_lo}..{m_hi - 1}] max err {err.max():.3e}, worst err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
    # the same samples as a clip that starts inside the 32-bit range: shifted by a multiple of `down` inputs, the phases line up
    _, K, _ = R.polyphase_taps(a, b)
    i_first = ((m_cross - 2000) * down + half_len) // up - K  # before the oldest input of the first compared output
    shift = i_first // down * down
    dm = shift // down * up
    y2 = l3ac_amd.resample(x[:, shift:].clone(), a, b)
    assert y2.shape[1] == n_out - dm and (y2.shape[1] * down + half_len) < B31
    for m_lo, m_hi in windows:
        assert torch.equal(y2[0, m_lo - dm:m_hi - dm], y[0, m_lo:m_hi]), f"outputs {m_lo}..{m_hi - 1} differ from the same samples resampled as a short clip"
    TIMES[f"resample {a}->{b}"] = time.perf_counter() - t0


def test_resample_batch_times_n_out_past_2_31():
    a, b, n_in = 16000, 48000, 16000
    batch = -(-(B31 + 2 * 48000) // 48000)
    _need((batch * n_in + 1.3 * batch * 48000) * 4 / GIB + 4)
    t0 = time.perf_counter()
    x = torch.randn(batch, n_in, device=DEV) * 0.3
    y = l3ac_amd.resample(x, a, b)
    torch.cuda.synchronize()
    assert y.shape == (batch, 48000) and y.numel() > B31 and bool(torch.isfinite(y).all())
    step = -(-batch // 4)
    for b0 in range(0, batch, step):
        assert torch.equal(l3ac_amd.resample(x[b0:b0 + step], a, b), y[b0:b0 + step]), f"clips {b0}.. differ from the same clips in a smaller call"
    clips = _boundary_clips(batch, 48000)
    ref, absdot = R.resample_ref(x[clips].cpu().double().numpy(), a, b)
    _, K, _ = R.polyphase_taps(a, b)
    err = np.abs(y[clips].cpu().double().numpy() - ref)
    assert (err <= (K + 2) * EPS * absdot).all(), f"clips {clips}: max err {err.max():.3e}"
    del x, y
    torch.cuda.empty_cache()
    TIMES["resample batch"] = time.perf_counter() - t0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_encode_decode_5600_clips():
    """encode_audio and decode_audio of 5600 x 1 s on a context of their own.  Its workspace by workspace_ensure_clip's rule: per clip
    2 x 388 800 (x0, x1) + 388 800 (a) + 1 555 200 (h) + 64 800 (yi) floats = 58.1 GiB for 5600 clips; the audio, tokens and samples add 0.7 GiB:
    under the 64 GiB above which the issue asks for this test to be left out (asserted from l3ac_workspace_bytes below)."""
    _need(64)
    t0 = time.perf_counter()
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.to(device=DEV).eval()
    try:
        ctx = codec.network.context()
        ctx.reserve(BATCH, 16000)
        ws = ctx.workspace_bytes
        print(f"\n[large] workspace after l3ac_reserve({BATCH}, 16000): {ws / GIB:.2f} GiB")
        audio = ((torch.rand(BATCH, 16000, generator=torch.Generator().manual_seed(1234)) * 2 - 1) * 0.5).to(DEV)
        assert ws + 3 * audio.numel() * 4 < 64 * GIB
        q, ind = codec.encode_audio(audio)
        idx = ind["indices"]
        assert idx.shape == (BATCH, 60) and int(idx.min()) >= 0 and int(idx.max()) < codec.network.mc.codebook_size
        wave = codec.decode_audio(q)
        assert wave.shape == (BATCH, 16200) and bool(torch.isfinite(wave).all())
        for b in (0, 2796, 2797, 5592, 5593, 5599):  # any clip alone: identical tokens and samples
            q1, ind1 = codec.encode_audio(audio[b:b + 1])
            assert torch.equal(ind1["indices"], idx[b:b + 1]), b
            assert torch.equal(codec.decode_audio(q1), wave[b:b + 1]), b
    finally:
        codec.network.cpu()
        gc.collect()
        torch.cuda.empty_cache()
    TIMES["encode + decode 5600 x 1 s"] = time.perf_counter() - t0
