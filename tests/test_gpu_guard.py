"""Every compute entry point against the memory it was handed (needs an MI355X: `pytest -m gpu`): reads outside the caller's tensors,
writes outside the outputs or past the declared scratch size, and results that depend on what an output or the scratch held before.

tests/test_gpu_poison.py poisons a clip's batch neighbours; here the hostile values lie AROUND the call's tensors (tests/arena.py): before
the first clip, behind the last, in the gaps of strided rows, behind the scratch, and in every output and scratch byte before the call.
Batches are 1 and 3: with one clip — every streaming chunk — there is no neighbour at all, and what lies past the tensor would feed the
only clip there is.  Sections A and B run the C ABI through arena.embedded_check (the call on plain tensors, then once per fill Z, N, I,
B with every input and output a placement; bit equality and intact guards); section C runs the Python layer under arena.prefilled, which
stands in for its two allocators.  The launch profile must name the same kernels in every run of a case, and the form a case is meant
for.  The shapes are the smallest at which a tile tail exists; none is the workload's.

Measured on an MI355X: no finding.  Every output of every case is bit for bit the plain call's under all four fills, every guard and
stride gap is intact, no entry reads its scratch before writing it, and no *_scratch_bytes is too small for the scratch placed at
exactly that size.  62 tests, 7.3 s for the file alone, the slowest test 0.8 s (test_stem[split], which also builds the 1kbps context).

That the tests can fail was shown once with two local builds, each run against test_layer_stft_log_mel_and_friends alone:
* metrics.hip without the hipMemsetAsync of the STFT output (cells after a clip's own frames are left unwritten): "stft extra_scratch=0
  fill N out: 1254 of 4356 words differ from the plain call, the first at (0, 21, 0), the last at (1, 21, 65); the result is not finite"
  — frame 21 of clip 0 and frames 4 .. 21 of clip 1, the cells the header defines as zero.
* metrics_stage_kernel with `i < n` widened to `i < n + 1` (one sample past the clip, which for the clip that fills the last row is the
  first word behind the tensor): "stft extra_scratch=0 fill N out: 132 of 4356 words differ from the plain call, the first at (2, 20, 0),
  the last at (2, 21, 65); the result is not finite" — the last two frames of the last clip, the only ones whose window reaches sample n.
  Fill Z had passed before it in both builds: only a non-finite word shows what a zero hides.

Kernels the launch profile named, per family (`pytest -s` prints them per case):
* stem: first_block_kernel in both forms (by workgroup count), strided and padded; encode_audio lengths=: first_block_kernel<RAGGED>.
* ConvUnit: C = 24 conv_unit_split_kernel<24> (default, narrow_ring 0) / conv_unit_ring_kernel<24> (2), fp32 route conv_unit_fused_kernel<24>;
  C = 48 conv_unit_ring_kernel<48> (default, 2) / conv_unit_split_kernel<48> (0), fp32 conv_unit_fused_kernel<48>; C = 96
  wide_sliced_hidden + wide_sliced_out_kernel<96> (default, wide_sliced 2) / conv_unit_wide_kernel<96> (0), fp32 conv_unit_fused_kernel<96>;
  C = 128 / 192 / 256 dwconv_ln_split_kernel + the sliced pair (default, 2) or conv_unit_wide_kernel (0); C = 8 / 32 / 512, every in-place call
  and the wide widths' fp32 route: dwconv_ln_kernel + gemm_f32_kernel / gemm_split_kernel.  Large grids: C = 256 and 192 conv_unit_wide_kernel
  plus the sliced tail, C = 96 conv_unit_wide_kernel<96> with unit_counter 0 and 1, C = 48 both narrow kernels.
* down layers: down_exact_kernel<144,48>, <240,96> (1kbps), <192,96> (3kbps) with down_fused = 2 on both routes; GEMM + row_kernel<PLAIN,CN>
  with down_fused = 0 and for 96 -> 192.  conv_k3: gemm_f32_kernel<1,true,32,false>, gemm_split_conv_kernel (128 -> 512 on bf16x3).
* enhance: enhance_branches / enhance_stats / gate_flat kernels; up: GEMM + row_kernel<LERP,CN>; enhance_up: up_fused_kernel<256,96>, <96,48>,
  <48,24> on the bf16x3 route, the unfused chain (gate_flat + gemm_split_kernel, or the gated gemm_f32_kernel, + row_kernel<LERP,CN>) at
  512 -> 256 and on the fp32 route.
* output stage: legacy_unit_split_kernel / legacy_unit_kernel by route, head_fused_kernel.  LocalTrans: the stack kernel as cooperative and
  as one-workgroup form for 1kbps, 3kbps and win40, the layered route for refdefault and tiny.
* GEMMs: gemm_f32_kernel<1,false,32,false>, <1,false,32,true>, <4,false,32,false>; gemm_split_kernel in the forms the row counts select.
  snake_kernel; fsq_kernel (hot and generic forward, quantize_act, decode); vq_wave_kernel, vq_scan_kernel, and the screened form's
  vq_norms / vq_screen / vq_resolve kernels; pack_kernel, unpack_kernel; resample_poly_kernel with the input aligned and one element off.
* Python layer: resample_poly_kernel; encode_audio / decode_audio: the whole codec (trans_stack_kernel<coop>, the ragged_* kernels with
  lengths=); metrics_stage / scatter / mel / mean kernels with gemm_f32_kernel, signal_metrics_kernel, mfcc_dct_kernel, dtw_kernel; the six
  stoi_* kernels; loudness_pass<state> / <energy>, loudness_scan, loudness_gate, loudness_gain, apply_gain, loudness_series, loudness_range,
  true_peak_tile / true_peak_clip kernels; sos_matrix / sos_scan / sos_pass<state> / <output>; pitch_kernel, pitch_metrics_kernel;
  xcorr_kernel, xcorr_pick_kernel, align_apply_kernel; lpc_frame_kernel, lpc_pair_kernel; sdr_corr / solve / residual / final kernels;
  bands_frame_kernel, bands_pair_kernel; coh_chunk / class / energy / finish kernels; ragged_upload_kernel wherever lengths= is given.

Out of scope: the session state buffers (codec, IIR and resample streams), which their own tests guard, and the context's internal
workspace, which no caller can place."""
import gc

import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import arena as A
from tests import gpu_ops as G
from tests import quantiser_ref as R
from tests import test_gpu_local_trans as LT
from tests import test_gpu_output_stage as TO
from tests import test_gpu_poison as TP
from tests import test_gpu_trend_front as TF
from tests.test_gpu_poison import DOWN_OUT, K3_TS, LARGE, PAIRS, STEM_TS, UNIT_TS, UNITS, UP_TS, Option, Route, Run, codec_of, unit_forms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = (1, 3)
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _release():
    """the contexts of this file (and the CUs their cooperative launches claimed) go when it is done"""
    yield
    for m in LT._MODELS.values():
        m.release()
    LT._MODELS.clear()
    for codec, _, _ in TP._CODECS.values():
        codec.network.cpu()
    TP._CODECS.clear()
    gc.collect()


def rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def guard(family, call, inputs, out_specs, what, want=(), never=(), fills=A.FILLS):
    """arena.embedded_check of call(*inputs, *outputs) under the launch profile: every run of the case names the same kernels, every
    prefix in `want` and none in `never`."""
    run = Run(family, lambda args: (call(*args), None)[1], want, never)  # (what a call returns is its outputs again)
    ref = A.embedded_check(lambda *args: run(args), inputs, out_specs, what, fills=fills, device=DEV)
    run.check(what)
    return ref


def report(*prefixes):
    for f in sorted(TP.FORMS):
        if any(f.startswith(p) for p in prefixes):
            print(f"\n[guard forms] {f}: {sorted(TP.FORMS[f])}")


def block_call(ctx, fn, block, shape):
    return lambda x, y: G.op_block(ctx, fn, block, x, shape, out=y)


# ---- A. codec blocks through the C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["split", "batch"])
def test_stem(form):
    """first_block_at at STEM_TS with one and three clips (first_block_split_kernel), and at the batch sizes and lengths that take the
    batch form: many short clips, and one or three clips long enough for more than 1024 workgroups."""
    codec, mc, w, ctx = codec_of("1kbps")
    d0 = mc.encoder_dims[0]
    shapes = [(b, t) for t in STEM_TS for b in BATCHES] if form == "split" else \
        [(1024 // -(-t // 64) + 1, t) for t in STEM_TS] + [(1, 64 * 1024 + 1), (3, 64 * 342 + 1)]
    for b, t in shapes:
        assert TF.few(b, t) == (form == "split")
        x = (torch.rand((b, t), generator=torch.Generator().manual_seed(90 + t)) * 2 - 1).to(DEV)
        guard(f"guard stem {form}", lambda a, y: G.first_block_at(ctx, a, out=y), [x], [((b, t, d0), F32)], f"stem {form} B={b} T={t}",
              want=["first_block_kernel"])
    report(f"guard stem {form}")


def test_stem_strided_rows_and_padding():
    """audio_stride > samples with the fill between the rows, frames > samples (the zero right-padding folded into the load): the two
    shapes of test_stem_strided_rows_and_padding, both forms"""
    codec, mc, w, ctx = codec_of("1kbps")
    d0 = mc.encoder_dims[0]
    for s, f, stride in ((257, 257, 258), (300, 540, 1000)):
        for b in BATCHES + (1024 // -(-f // 64) + 1,):
            x = (torch.rand((b, s), generator=torch.Generator().manual_seed(s + b)) * 2 - 1).to(DEV)

            def call(a, y):
                # (one row has no stride of its own: the ABI is given the stride all the same)
                _capi.check(ctx.lib.l3ac_op_first_block_at(ctx.handle, a.data_ptr(), b, s, stride, f, y.data_ptr(), torch.cuda.current_stream().cuda_stream))

            guard("guard stem strided", call, [{"t": x, "stride0": stride}], [((b, f, d0), F32)], f"stem B={b} samples={s} frames={f} stride={stride}",
                  want=["first_block_kernel"])
    report("guard stem strided")


def unit_in_place(ctx, block):
    def call(x):  # x == y: one placement is input and output; the in-place call takes the unfused route
        b, t, c = x.shape
        _capi.check(ctx.lib.l3ac_op_conv_unit(ctx.handle, block.encode(), x.data_ptr(), b, t, x.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return call


UNFUSED_ONLY = ("conv_unit_wide_kernel", "conv_unit_ring_kernel", "conv_unit_split_kernel", "conv_unit_fused_kernel", "wide_sliced_out_kernel")


@pytest.mark.parametrize("c", sorted(UNITS))
def test_conv_unit_small(c):
    cfg, seed, block = UNITS[c]
    codec, mc, w, ctx = codec_of(cfg, seed)
    fam = f"guard conv_unit C={c}"
    for t in UNIT_TS:
        for b in BATCHES:
            x = rand((b, t, c), 1000 + c + t)
            for split in (True, False):
                route = "bf16x3" if split else "fp32"
                with Route(codec, split):
                    for opt, val, want, never in (unit_forms(c) if split else unit_forms(c)[:1]):
                        with Option(ctx, opt or "unit_counter", val):  # (the default form: nothing is set, the option is only restored)
                            guard(f"{fam} {route} {opt}={val}", block_call(ctx, "l3ac_op_conv_unit", block, (b, t, c)), [x], [((b, t, c), F32)],
                                  f"{block} C={c} B={b} T={t} split={split} {opt}={val}", want=want, never=never)
                    guard(f"{fam} in place {route}", unit_in_place(ctx, block), [{"t": x, "inout": True}], [], f"{block} C={c} B={b} T={t} split={split} in place",
                          never=UNFUSED_ONLY)
    report(fam + " ")


@pytest.mark.parametrize("c,block,b,t,extra,option,want", LARGE, ids=[f"C{r[0]}" for r in LARGE])
def test_conv_unit_large_grid(c, block, b, t, extra, option, want):
    """One large-grid case per family, fill N: the persistent kernels' last tile and the sliced tail end where the tensor ends."""
    codec, mc, w, ctx = codec_of("1kbps")
    x = rand((b, t, c), 2000 + c)
    name, values = option
    for v in values:
        with Option(ctx, name, v):
            ring = {0: ("conv_unit_split_kernel",), 2: ("conv_unit_ring_kernel",)}[v] if name == "narrow_ring" else ()
            guard(f"guard conv_unit C={c} large grid {name}={v}", block_call(ctx, "l3ac_op_conv_unit", block, (b, t, c)), [x], [((b, t, c), F32)],
                  f"{block} B={b} T={t} {name}={v}", want=want + ring, fills=("N",))
    report(f"guard conv_unit C={c} large")


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
def test_down_layers(tag):
    codec, mc, w, ctx = codec_of(tag)
    for i, s in enumerate(mc.compress_rates):
        block, ci, co = f"encoder.blocks.{2 * i + 2}", mc.encoder_dims[i], mc.encoder_dims[i + 1]
        exact = (ci * s, co) in ((144, 48), (240, 96), (192, 96))  # down_exact_supported
        for t_out in DOWN_OUT:
            for b in BATCHES:
                x = rand((b, s * t_out, ci), 3000 + ci + t_out)
                for split in (True, False):
                    for fused in (0, 2):
                        with Route(codec, split), Option(ctx, "down_fused", fused):
                            guard(f"guard down {tag} {ci}x{s}->{co} down_fused={fused} {'bf16x3' if split else 'fp32'}",
                                  block_call(ctx, "l3ac_op_down_layer", block, (b, t_out, co)), [x], [((b, t_out, co), F32)],
                                  f"{tag} {block} B={b} T_out={t_out} down_fused={fused} split={split}",
                                  want=("down_exact_kernel",) if fused == 2 and exact else (), never=() if fused == 2 and exact else ("down_exact_kernel",))
    report(f"guard down {tag}")


@pytest.mark.parametrize("block", ["encoder.blocks.8", "decoder.blocks.0"])
def test_conv_k3(block):
    codec, mc, w, ctx = codec_of("1kbps")
    co, ci = w[f"{block}.weight"].shape[:2]
    for t in K3_TS:
        for b in BATCHES:
            x = rand((b, t, ci), 4000 + t)
            for split in (True, False):
                with Route(codec, split):
                    guard(f"guard conv_k3 {ci}->{co} {'bf16x3' if split else 'fp32'}", block_call(ctx, "l3ac_op_conv_k3", block, (b, t, co)), [x],
                          [((b, t, co), F32)], f"{block} B={b} T={t} split={split}", want=("gemm_",))
    report(f"guard conv_k3 {ci}->")


@pytest.mark.parametrize("tag", ["1kbps", "3kbps"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}+{p[1]}")
def test_enhance_and_up_layers(tag, pair):
    codec, mc, w, ctx = codec_of(tag)
    k = PAIRS.index(pair)
    eb, ub = f"decoder.blocks.{pair[0]}", f"decoder.blocks.{pair[1]}"
    ci, co, s = mc.decoder_dims[k], mc.decoder_dims[k + 1], mc.decode_rates[k]
    fused = (ci, co) in TF.UP_FUSED
    for t in UP_TS:
        for b in BATCHES:
            x = rand((b, t, ci), 5000 + ci + t)
            for split in (True, False):
                with Route(codec, split):
                    route = "bf16x3" if split else "fp32"
                    calls = (("enhance", block_call(ctx, "l3ac_op_enhance", eb, (b, t, ci)), (b, t, ci), ("enhance_branches_kernel",)),
                             ("up", block_call(ctx, "l3ac_op_up_layer", ub, (b, t * s, co)), (b, t * s, co), ("row_kernel",)),
                             ("enhance_up", lambda a, y: G.op_block2(ctx, "l3ac_op_enhance_up", eb, ub, a, (b, t * s, co), out=y), (b, t * s, co),
                              ("up_fused_kernel",) if fused and split else ("enhance_stats_kernel", "row_kernel")))
                    for name, call, shape, want in calls:
                        guard(f"guard {name} {tag} {ci}->{co} x{s} {route}", call, [x], [(shape, F32)], f"{tag} {name} {eb}+{ub} B={b} T={t} split={split}", want=want)
    report(f"guard enhance {tag} {ci}->{co} ", f"guard up {tag} {ci}->{co} ", f"guard enhance_up {tag} {ci}->{co} ")


def test_output_stage():
    """LegacyUnits 0 .. 2, the head with pre-tanh on and off, and the whole last block, both routes."""
    st = TO.stage("1kbps")
    for split in (True, False):
        route = "bf16x3" if split else "fp32"
        with TO.Route(st, split):
            for b in BATCHES:
                for u, d in enumerate(TO.DILS):
                    for t in (1, 3 * d - 1, 3 * d + 1, 257):
                        x = G.to_frames(TO._x(b, st.c, t, seed=500 + t, loud=1))
                        guard(f"guard legacy_unit {route}", lambda a, y: G.legacy_unit(st.ctx, u, a, out=y), [x], [((b, t, st.c), F32)],
                              f"unit {u} B={b} T={t} split={split}", want=(TO.WANT[split],), never=(TO.WANT[not split],))
                for t in (1, 3, 4, 257):
                    x = G.to_frames(TO._x(b, st.c, t, seed=600 + t, loud=1))
                    for pre in (True, False):
                        st.ctx.set_head_pretanh(pre)
                        try:
                            guard(f"guard head {route}", lambda a, y: G.head(st.ctx, a, out=y), [x], [((b, t), F32)],
                                  f"head B={b} T={t} pretanh={pre} split={split}", want=("head_fused_kernel",))
                        finally:
                            st.ctx.set_head_pretanh(False)
                for t in (1, 26, 28, 257):
                    x = G.to_frames(TO._x(b, st.c, t, seed=700 + t, loud=1))
                    guard(f"guard last_block {route}", lambda a, y: G.op_plain(st.ctx, "l3ac_op_last_block", a, b, t, (b, t), out=y), [x], [((b, t), F32)],
                          f"last_block B={b} T={t} split={split}", want=(TO.WANT[split],))
    report("guard legacy_unit", "guard head", "guard last_block")


@pytest.mark.parametrize("name", list(LT.CONFIGS))
def test_local_trans(name, monkeypatch):
    """Each config's stacks at the first length of EXACT_LENGTHS, on every route that length takes.  LT.run asserts the route from its
    own launch profile; it calls G.op_block, which is handed the placement as its output here."""
    m = LT.model(name)
    real = G.op_block
    for stack, window, depth in m.stacks:
        t = LT.EXACT_LENGTHS[(name, window)][0]
        routes = ("coop", "single") if m.takes_stack_kernel(window, t) else ("layered",)
        for b in BATCHES:
            x = LT.inputs(t, m.dim, window, seed=31 * t + window)[:b].contiguous().to(DEV)
            for route in routes:
                def call(a, y):
                    with monkeypatch.context() as mp:
                        mp.setattr(G, "op_block", lambda *args, **kw: real(*args, out=y, **kw))
                        LT.run(m, stack, a, route)

                A.embedded_check(call, [x], [((b, t, m.dim), F32)], f"{m.label} {stack} W={window} B={b} T={t} {route}", device=DEV)
                TP.FORMS.setdefault(f"guard local_trans {m.label}", set()).add(route)
    report(f"guard local_trans {m.label}")


# ---- B. context-free numeric entries ------------------------------------------------------------------------------------------------------------------
GEMM_MS = (1, 60, 129, 180, 400)  # the row counts that select the launch forms of test_gemm_*_forms_return_the_same_bits


def gemm_cases(kind, shapes, fn):
    g = torch.Generator().manual_seed(41)
    for n, k in shapes:
        w = (torch.randn(n, k, generator=g) * 0.1).to(DEV)
        bias = torch.randn(n, generator=g).to(DEV)
        for m in GEMM_MS:
            a = torch.randn(m, k, generator=g).to(DEV)
            lda, ldc = k + 12, n + 4
            for with_bias in (True, False):
                def call(a_, w_, b_, c_):
                    fn(a_, w_, b_ if with_bias else None, out=c_, lda=lda, ldc=ldc)

                guard(f"guard {kind}", call, [{"t": a, "stride0": lda}, w, bias], [{"shape": (m, n), "dtype": F32, "stride0": ldc}],
                      f"{kind} m={m} n={n} k={k} lda={lda} ldc={ldc} bias={with_bias}", want=("gemm_",))
    report(f"guard {kind}")


def test_gemm_f32():
    gemm_cases("gemm_f32", ((32, 36), (100, 72), (128, 384)), G.gemm)


def test_gemm_split():
    gemm_cases("gemm_split", ((200, 40), (192, 96), (256, 544), (512, 2048)), G.gemm_split)


def test_snake():
    g = torch.Generator().manual_seed(3)
    for rows, c in ((1, 4), (3, 64), (257, 24), (33, 96)):
        x = (torch.randn(rows, c, generator=g) * 3).to(DEV)
        alpha = (torch.rand(c, generator=g) * 3 + 0.05).to(DEV)
        for mode in (0, 1, 4):
            guard("guard snake", lambda x_, al, y: G.snake(x_, al, mode, out=y), [x, alpha], [((rows, c), F32)], f"snake rows={rows} c={c} mode={mode}")
    report("guard snake")


def _quantiser():
    codec, mc, w, ctx = codec_of("1kbps")
    dev = [w[f"quantizer.{k}"].to(DEV) for k in ("project_in.weight", "project_in.bias", "project_out.weight", "project_out.bias")]
    return mc, dev


@pytest.mark.parametrize("want_latents", [False, True], ids=["hot", "generic"])
def test_fsq_forward(want_latents):
    mc, weights = _quantiser()
    d, feat = len(mc.levels), 128
    for n in (1, 1038):
        x = rand((n, feat), 90 + n, 2.0)
        specs = [((n, feat), F32), ((n,), torch.int32), ((n, d), F32)] + ([((n, d), F32)] if want_latents else [])

        def call(x_, wi, bi, wo, bo, *out):
            G.fsq_forward(x_, list(mc.levels), wi, bi, wo, bo, want_latents=want_latents, out=out)

        guard(f"guard fsq {'generic' if want_latents else 'hot'}", call, [x] + weights, specs, f"fsq_forward n={n} want_latents={want_latents}", want=("fsq_kernel",))
    report("guard fsq ")


def test_fsq_quantize_act_and_decode():
    mc, (w_in, b_in, w_out, b_out) = _quantiser()
    d, feat, levels = len(mc.levels), 128, list(mc.levels)
    for n in (1, 1038):
        act = torch.rand((n, d), generator=torch.Generator().manual_seed(n)).to(DEV)
        ref = guard("guard fsq_quantize_act", lambda a, wo, bo, *out: G.fsq_quantize_act(a, levels, wo, bo, out=out), [act, w_out, b_out],
                    [((n, feat), F32), ((n,), torch.int32), ((n, d), F32)], f"fsq_quantize_act n={n}")
        idx = ref["out1"]
        assert bool(((idx >= 0) & (idx < mc.codebook_size)).all())
        dec = guard("guard fsq_decode", lambda i, wo, bo, q: G.fsq_decode(i, levels, wo, bo, out=q), [idx, w_out, b_out], [((n, feat), F32)], f"fsq_decode n={n}")
        assert torch.equal(dec["out0"], ref["out0"])
    report("guard fsq_quantize_act", "guard fsq_decode")


@pytest.mark.parametrize("form,n", [(0, 700), (0, R.VQ_WAVE_MAX_N), (1, R.VQ_WAVE_MAX_N)], ids=["small", "screened", "scan"])
def test_vq_argmin(form, n):
    """the scan and the screened form, the scratch a placement of exactly l3ac_vq_argmin_scratch_bytes bytes"""
    dim = 4
    k = 513
    q, cb = (torch.as_tensor(v) for v in R.vq_grid_case(dim, k, n, seed=17))
    nbytes = _capi.load_library().l3ac_vq_argmin_scratch_bytes(n, cb.shape[0], form)
    guard(f"guard vq_argmin form={form} n={n}", lambda q_, cb_, out, scratch: G.vq_argmin(q_, cb_, form=form, out=out, scratch=scratch),
          [q.to(DEV), cb.to(DEV)], [((n,), torch.int32), {"shape": (nbytes,), "dtype": torch.uint8, "scratch": True}], f"vq_argmin form={form} n={n} k={k}")
    report("guard vq_argmin")


def test_pack_and_unpack_indices():
    lib = _capi.load_library()
    for bits in (17, 18):
        for b in BATCHES:
            for n_tok in (1, 31, 32, 33, 257):
                words = -(-n_tok * bits // 32)
                idx = torch.randint(0, 1 << bits, (b, n_tok), generator=torch.Generator().manual_seed(n_tok), dtype=torch.int32).to(DEV)
                what = f"bits={bits} B={b} n_tok={n_tok}"
                ref = guard("guard pack_indices", lambda i, out: _capi.check(lib.l3ac_pack_indices(i.data_ptr(), b, n_tok, bits, out.data_ptr(), words,
                                                                                                 torch.cuda.current_stream().cuda_stream)),
                            [idx], [((b, words), torch.int32)], f"pack_indices {what}")
                back = guard("guard unpack_indices", lambda p, out: _capi.check(lib.l3ac_unpack_indices(p.data_ptr(), b, n_tok, bits, words, out.data_ptr(),
                                                                                                      torch.cuda.current_stream().cuda_stream)),
                             [ref["out0"]], [((b, n_tok), torch.int32)], f"unpack_indices {what}")
                assert torch.equal(back["out0"], idx)
    report("guard pack_indices", "guard unpack_indices")


@pytest.mark.parametrize("a,b_rate", [(48000, 16000), (16000, 44100), (44100, 48000)])
def test_resample_direct(a, b_rate):
    """l3ac_resample itself: strided rows with the fill between them, the input 16-byte aligned and one element off (both branches of the
    kernel's `vec` test), 65 clips = two workgroups of 64 lanes"""
    lib = _capi.load_library()
    for n in (1, 7, 333):
        n_out = l3ac_amd.resample_length(a, b_rate, n)
        for b in (1, 3, 65):
            x = rand((b, n), 82 + n, 0.3)
            bank = l3ac_amd._resample_bank(torch.device(DEV), a, b_rate)
            for offset in (0, 1):
                def call(x_, bank_, y):
                    _capi.check(lib.l3ac_resample(x_.data_ptr(), b, n, n + 5, a, b_rate, bank_.data_ptr(), y.data_ptr(), n_out, torch.cuda.current_stream().cuda_stream))

                guard(f"guard resample {a}->{b_rate}", call, [{"t": x, "stride0": n + 5, "offset": offset}, bank], [((b, n_out), F32)],
                      f"l3ac_resample {a}->{b_rate} B={b} n={n} offset={offset}", want=("resample_poly_kernel",))
    report(f"guard resample {a}->{b_rate}")


# ---- C. the Python layer under arena.prefilled ----------------------------------------------------------------------------------------------------------
def layer(monkeypatch, family, fn, tensors, what=None, want=()):
    """fn(*tensors) unpatched, then under prefilled(fill) for every fill with the tensors as views into an arena of that fill: every
    returned tensor the same bits, every arena intact, the same kernels in every run."""
    what = what or family
    run = Run("guard " + family, lambda args: fn(*args), want)
    ref = run(tuple(tensors))
    for fill in A.FILLS:
        with A.prefilled(fill, monkeypatch) as arenas:
            got = run(tuple(arenas.view(t) for t in tensors))
        A.same_bits(ref, got, f"{what} fill {fill}")
        arenas.intact(what)
        assert arenas.arenas, f"{what}: the call allocated nothing through torch.empty or _metric.scratch"
    run.check(what)
    return ref


def both_scratch(monkeypatch, family, fn, tensors, want=()):
    """an entry that takes extra_scratch=: once with the minimum scratch, once with its default"""
    layer(monkeypatch, family, lambda *t: fn(*t, extra_scratch=0), tensors, f"{family} extra_scratch=0", want)
    return layer(monkeypatch, family, fn, tensors, f"{family} default scratch", want)


def tones(b, t, seed, fs=16000, level=0.3):
    """b voiced clips (harmonics of 110, 150, 190 Hz .. under a slow envelope, a little noise), fp32 on the GPU"""
    g = torch.Generator().manual_seed(seed)
    tt = torch.arange(t, dtype=torch.float64) / fs
    rows = [sum(torch.sin(2 * torch.pi * (110.0 + 40 * i) * h * tt + h) / h for h in range(1, 5)) * (1 + 0.5 * torch.sin(2 * torch.pi * 3 * tt)) for i in range(b)]
    return (level * torch.stack(rows).float() + 0.01 * torch.randn((b, t), generator=g)).to(DEV)


def pair_of(t, seed, fs=16000):
    ref = tones(3, t, seed, fs)
    return ref, (0.9 * ref + 0.02 * rand((3, t), seed + 1)).contiguous()


def ragged(t, short):
    """three lengths: clip 0 a little short of the row, clip 1 `short`, clip 2 the full row: its last frame ends where the tensor ends"""
    return [t - 7, short, t]


@pytest.mark.parametrize("a,b_rate", [(48000, 16000), (16000, 44100)])
def test_layer_resample(monkeypatch, a, b_rate):
    layer(monkeypatch, f"resample {a}->{b_rate}", lambda x: l3ac_amd.resample(x, a, b_rate), [rand((3, 333), 82, 0.3)], want=("resample_poly_kernel",))
    report("guard resample ")


def test_layer_encode_decode_audio(monkeypatch):
    codec, mc, w, ctx = codec_of("1kbps")
    hop = mc.hop_length
    t = 9 * hop + 3
    x = (torch.rand((3, t), generator=torch.Generator().manual_seed(77)) - 0.5).to(DEV)
    lens = [t - hop - 5, 2 * hop + 3, t]
    plain = layer(monkeypatch, "encode_audio", codec.encode_audio, [x], want=("first_block_kernel", "fsq_kernel"))
    rag = layer(monkeypatch, "encode_audio lengths=", lambda a: codec.encode_audio(a, lengths=lens), [x], want=("first_block_kernel<RAGGED>", "fsq_kernel"))
    before = ctx.bad_index_count()
    layer(monkeypatch, "decode_audio", lambda q: codec.decode_audio(q), [plain[0]])
    layer(monkeypatch, "decode_audio", lambda i: codec.decode_audio(indices=i), [plain[1]["indices"]], "decode_audio indices=")
    tok = rag[1]["lengths"].tolist()
    layer(monkeypatch, "decode_audio lengths=", lambda q: codec.decode_audio(q, lengths=tok), [rag[0]])
    layer(monkeypatch, "decode_audio lengths=", lambda i: codec.decode_audio(indices=i, lengths=tok), [rag[1]["indices"]], "decode_audio indices= lengths=")
    assert ctx.bad_index_count() == before
    report("guard encode_audio", "guard decode_audio")


def test_layer_stft_log_mel_and_friends(monkeypatch):
    n_fft, hop, n_mels = 64, 16, 8
    t = 21 * hop + 5
    lens = ragged(t, 3 * hop + 1)
    ref, est = pair_of(t, 128)
    both_scratch(monkeypatch, "stft", lambda a, **kw: l3ac_amd.stft(a, n_fft, hop, lengths=lens, **kw), [ref], want=("metrics_stage_kernel",))
    both_scratch(monkeypatch, "stft plain", lambda a, **kw: l3ac_amd.stft(a, n_fft, hop, **kw), [ref], want=("metrics_stage_kernel",))
    both_scratch(monkeypatch, "log_mel", lambda a, **kw: l3ac_amd.log_mel(a, 16000, n_fft, hop, n_mels, lengths=lens, **kw), [ref], want=("metrics_mel_kernel",))
    both_scratch(monkeypatch, "mel_distance", lambda r, e, **kw: l3ac_amd.mel_distance(r, e, 16000, scales=[(64, 16, 8), (32, 8, 24)], lengths=lens, **kw), [ref, est],
                 want=("metrics_mean_kernel",))
    layer(monkeypatch, "signal_metrics", lambda r, e: l3ac_amd.signal_metrics(r, e, lengths=lens), [ref, est], want=("signal_metrics_kernel",))
    report("guard stft", "guard log_mel", "guard mel_distance", "guard signal_metrics")


def test_layer_mfcc_dtw_and_mcd(monkeypatch):
    kw = dict(sample_rate=16000, n_fft=64, hop=16, n_mels=8, n_coeffs=5)
    t = 21 * 16 + 5
    lens = ragged(t, 3 * 16 + 1)
    ref, est = pair_of(t, 140)
    cep = both_scratch(monkeypatch, "mfcc", lambda a, **k: l3ac_amd.mfcc(a, lengths=lens, **kw, **k), [ref], want=("mfcc_dct_kernel",))
    frames = cep[1].tolist()
    a, b = cep[0], l3ac_amd.mfcc(est, lengths=lens, **kw)[0]
    both_scratch(monkeypatch, "dtw", lambda u, v, **k: l3ac_amd.dtw(u, v, lengths_a=frames, lengths_b=frames, return_path=True, return_cost_matrix=True, **k), [a, b],
                 want=("dtw_kernel",))
    both_scratch(monkeypatch, "mcd", lambda r, e, **k: l3ac_amd.mcd(r, e, lengths=lens, return_path=True, **kw, **k), [ref, est], want=("dtw_kernel",))
    both_scratch(monkeypatch, "mcd dtw=False", lambda r, e, **k: l3ac_amd.mcd(r, e, lengths=lens, dtw=False, **kw, **k), [ref, est])
    report("guard mfcc", "guard dtw", "guard mcd")


def test_layer_stoi(monkeypatch):
    t = 6000  # at 10 kHz: 45 analysis frames; clip 1 has too few for a segment
    lens = ragged(t, 3000)
    ref, est = pair_of(t, 150, fs=10000)
    both_scratch(monkeypatch, "stoi", lambda r, e, **k: l3ac_amd.stoi(r, e, 10000, lengths=lens, return_bands=True, **k), [ref, est],
                 want=("stoi_select_kernel", "stoi_segment_kernel"))
    report("guard stoi")


def test_layer_loudness(monkeypatch):
    fs, t = 8000, 8000
    lens = ragged(t, 3500)
    x = tones(3, t, 160, fs)
    stats = layer(monkeypatch, "loudness", lambda a: l3ac_amd.loudness(a, fs, lengths=lens, return_momentary=True), [x], want=("loudness_gate_kernel",))
    gain = layer(monkeypatch, "loudness_gain", lambda lufs, peak: l3ac_amd.loudness_gain({"lufs": lufs, "peak": peak}, -23.0, peak_limit_db=-1.0),
                 [stats["lufs"], stats["peak"]], want=("loudness_gain_kernel",))
    layer(monkeypatch, "apply_gain", lambda a, g: l3ac_amd.apply_gain(a, g, lengths=lens), [x, gain["gain"]], want=("apply_gain_kernel",))
    layer(monkeypatch, "normalize_loudness", lambda a: l3ac_amd.normalize_loudness(a, -23.0, fs, lengths=lens), [x], want=("loudness_gain_kernel", "apply_gain_kernel"))
    report("guard loudness", "guard apply_gain", "guard normalize_loudness")


def test_layer_r128(monkeypatch):
    fs, t = 8000, 28000  # 3.5 s: six short-term blocks
    lens = ragged(t, 9000)
    x = tones(3, t, 170, fs)
    layer(monkeypatch, "short_term_loudness", lambda a: l3ac_amd.short_term_loudness(a, fs, lengths=lens, window=3.0, return_parts=True), [x])
    layer(monkeypatch, "short_term_loudness", lambda a: l3ac_amd.short_term_loudness(a, fs, lengths=lens, window=0.4), [x], "momentary series")
    layer(monkeypatch, "loudness_range", lambda a: l3ac_amd.loudness_range(a, fs, lengths=lens), [x])
    layer(monkeypatch, "true_peak", lambda a: l3ac_amd.true_peak(a, fs), [x[:, :1000].contiguous()], "true_peak plain rows")
    layer(monkeypatch, "true_peak", lambda a: l3ac_amd.true_peak(a, fs, lengths=ragged(1000, 333)), [x[:, :1000].contiguous()], "true_peak ragged")
    report("guard short_term_loudness", "guard loudness_range", "guard true_peak")


def test_layer_sosfilt(monkeypatch):
    t = 700
    lens = ragged(t, 123)
    x = tones(3, t, 180)
    sos = l3ac_amd.butter_sos(4, 50.0, 16000)
    for dtype in (torch.float32, torch.float64):
        layer(monkeypatch, "sosfilt", lambda a: l3ac_amd.sosfilt(a, sos, lengths=lens, dtype=dtype), [x], f"sosfilt {dtype}")
        layer(monkeypatch, "sosfilt", lambda a: l3ac_amd.sosfilt(a, sos, dtype=dtype, extra_scratch=4096), [x], f"sosfilt {dtype} plain rows, extra scratch")
    report("guard sosfilt")


def test_layer_pitch(monkeypatch):
    fs = 8000
    span = l3ac_amd.pitch_lags(fs)["span"]
    t = span + 9 * (fs // 100) + 5
    lens = ragged(t, span - 1)  # clip 1 has no frame
    ref, est = pair_of(t, 190, fs)
    both_scratch(monkeypatch, "pitch", lambda a, **k: l3ac_amd.pitch(a, fs, lengths=lens, return_cmnd=True, **k), [ref])
    layer(monkeypatch, "pitch_metrics", lambda r, e: l3ac_amd.pitch_metrics(r, e, fs, lengths=lens), [ref, est])
    report("guard pitch")


def test_layer_delay_and_align(monkeypatch):
    t = 500
    lens = ragged(t, 123)
    ref = tones(3, t, 200)
    est = torch.roll(ref, 7, dims=1).contiguous()
    d = both_scratch(monkeypatch, "delay", lambda r, e, **k: l3ac_amd.delay(r, e, 40, lengths=lens, return_xcorr=True, **k), [ref, est])
    layer(monkeypatch, "apply_delay", lambda r, e, lag: l3ac_amd.apply_delay(r, e, lag, lengths=lens), [ref, est, d["lag"]])
    layer(monkeypatch, "align", lambda r, e: l3ac_amd.align(r, e, 40, lengths=lens), [ref, est])
    report("guard delay", "guard apply_delay", "guard align")


def test_layer_lpc(monkeypatch):
    kw = dict(sample_rate=16000, order=16, frame=100, hop=25)
    t = 100 + 25 * 25 + 8
    lens = ragged(t, 99)  # clip 1 has no frame
    ref, est = pair_of(t, 210)
    both_scratch(monkeypatch, "lpc", lambda a, **k: l3ac_amd.lpc(a, lengths=lens, **kw, **k), [ref], want=("lpc_frame_kernel",))
    both_scratch(monkeypatch, "lpc_metrics", lambda r, e, **k: l3ac_amd.lpc_metrics(r, e, lengths=lens, return_frames=True, **kw, **k), [ref, est],
                 want=("lpc_frame_kernel", "lpc_pair_kernel"))
    report("guard lpc")


def test_layer_sdr(monkeypatch):
    t, taps = 700, 37
    lens = ragged(t, 300)
    ref, est = pair_of(t, 220)
    both_scratch(monkeypatch, "correlate", lambda u, v, **k: l3ac_amd.correlate(u, v, taps, lengths=lens, **k), [ref, est])
    out = both_scratch(monkeypatch, "sdr", lambda r, e, **k: l3ac_amd.sdr(r, e, filter_length=taps, lengths=lens, return_filter=True, **k), [ref, est])
    layer(monkeypatch, "toeplitz_solve", l3ac_amd.toeplitz_solve, [out["autocorr"], out["crosscorr"]])
    report("guard correlate", "guard sdr", "guard toeplitz_solve")


def test_layer_bands(monkeypatch):
    kw = dict(sample_rate=16000, frame=100, hop=25, n_fft=256)
    t = 100 + 25 * 25 + 8
    lens = ragged(t, 99)
    ref, est = pair_of(t, 230)
    both_scratch(monkeypatch, "frame_spectrum", lambda a, **k: l3ac_amd.frame_spectrum(a, lengths=lens, detail=True, **kw, **k), [ref])
    both_scratch(monkeypatch, "band_energies", lambda a, **k: l3ac_amd.band_energies(a, lengths=lens, **kw, **k), [ref])
    both_scratch(monkeypatch, "band_metrics", lambda r, e, **k: l3ac_amd.band_metrics(r, e, lengths=lens, return_frames=True, **kw, **k), [ref, est])
    report("guard frame_spectrum", "guard band_")


def test_layer_coherence(monkeypatch):
    kw = dict(sample_rate=16000, frame=100, hop=25, n_fft=256)
    t = 100 + 25 * 25 + 8
    lens = ragged(t, 99)
    ref, est = pair_of(t, 240)
    both_scratch(monkeypatch, "coherence", lambda r, e, **k: l3ac_amd.coherence(r, e, lengths=lens, return_sums=True, **kw, **k), [ref, est])
    both_scratch(monkeypatch, "csii", lambda r, e, **k: l3ac_amd.csii(r, e, lengths=lens, return_bands=True, return_sums=True, **kw, **k), [ref, est])
    report("guard coherence", "guard csii")
