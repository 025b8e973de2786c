"""The GRN validation mode (network.grn_exact = True: dwconv_ln -> GEMM with EPI_SNAKE -> grn_sumsq_kernel -> grn_apply_kernel -> GEMM
with EPI_BIAS_RES) and its guard (network.min_grn_norm()) against the fp64 oracle.

Every ConvUnit kernel of the fast path takes the normaliser n = g / (g + 1e-8) as exactly 1 (true in fp32 for g >= 0.25, g = the clip's L2
norm over the whole hidden tensor) and the validation mode is the referee the documents name for that assumption, so it is tested here the
way a kernel is: every width on both GEMM routes, the guard's VALUE against the reference's per-clip norms, the literal formula where n is
far from 1 (a doctored model whose hidden tensor has g = 1e-2 .. 1e-9 and exactly 0), and clips that must not share a normaliser."""
import copy
import math

import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi, weights as W
from oracle import l3ac_oracle as O
from tests import gpu_ops as G
from tests.helpers import GOLDEN, assert_close, seeded_audio, seeded_randn as _rand

pytestmark = pytest.mark.gpu

ATOL_BLOCK = RTOL_BLOCK = 5e-5  # the ConvUnit tolerance of test_gpu_blocks.py (one block, activations O(1))

MODELS = {"1kbps": ("1kbps", 0), "tiny": (GOLDEN / "tiny.toml", 3), "refdefault": (GOLDEN / "refdefault.toml", 5)}
UNITS = [("1kbps", "encoder.blocks.1.0.module", 24), ("1kbps", "encoder.blocks.3.0.module", 48), ("1kbps", "encoder.blocks.5.0.module", 96),
         ("1kbps", "encoder.blocks.7.1.module", 192), ("1kbps", "decoder.blocks.4.1.module", 256), ("1kbps", "decoder.blocks.1.2.module", 512),
         ("tiny", "encoder.blocks.1.0.module", 8), ("tiny", "encoder.blocks.5.1.module", 24), ("tiny", "decoder.blocks.1.1.module", 32),
         ("refdefault", "decoder.blocks.4.0.module", 128)]
UNIT_IDS = [f"{m}-C{c}" for m, _, c in UNITS]


def _close(name, got, ref):
    assert_close(name, got, ref, ATOL_BLOCK, RTOL_BLOCK)


def _rms(e):
    return float(e.double().pow(2).mean().sqrt())


def guard_rtol(c):
    """A priori bound on the guard's relative error at width C: a K = C fp32 dot product per hidden element plus fewer than 64 fp32 additions
    per partial sum of squares, halved by the square root, doubled for margin (6.9e-5 at C = 512)."""
    return 2 * (c + 64) * 2.0 ** -24


class GrnRecorder:
    """Wraps oracle.grn (conv_unit looks it up at call time): per call the per-clip norms, the rms of the hidden tensor and the output."""

    def __init__(self, monkeypatch):
        self.norms, self.rms, self.out = [], [], []
        original = O.grn

        def recorder(x, gamma, beta):
            self.norms.append(torch.norm(x, dim=[1, 2]).double())
            self.rms.append(x.double().pow(2).mean(dim=[1, 2]).sqrt())
            y = original(x, gamma, beta)
            self.out.append(y)
            return y

        monkeypatch.setattr(O, "grn", recorder)

    def minimum(self):
        """(smallest norm over every call and clip, rms of the hidden tensor it was taken over)"""
        norms, rms = torch.cat(self.norms), torch.cat(self.rms)
        i = int(norms.argmin())
        return float(norms[i]), float(rms[i])


def _w64(w, block):
    return {k: v.double() for k, v in w.items() if k.startswith(block)}


def _unit_ref64(monkeypatch, w, block, x):
    """fp64 oracle of one ConvUnit on x (B, C, T): (output, per-clip GRN norms, GRN output (B, T, 4C))."""
    with monkeypatch.context() as mp:
        rec = GrnRecorder(mp)
        y = O.conv_unit(_w64(w, block), block, x.double())
    return y, rec.norms[0], rec.out[0]


@pytest.fixture(scope="module")
def models():
    """models(tag) -> (validation-mode codec, default codec, folded fp32 weights) of one of MODELS, each made on first use."""
    made = {}

    def get(tag):
        if tag not in made:
            cfg, seed = MODELS[tag]
            exact = l3ac_amd.get_model(cfg, synthetic_seed=seed)
            exact.network.grn_exact = True
            exact.network.to(device="cuda").eval()
            fast = l3ac_amd.get_model(cfg, synthetic_seed=seed)
            fast.network.to(device="cuda").eval()
            made[tag] = (exact, fast, W.folded_weights(exact.network.state_dicts()))
        return made[tag]

    yield get
    made.clear()


def _run(ctx, block, x_bct, in_place=False):
    """l3ac_op_conv_unit on x (B, C, T) -> ((B, C, T) on the CPU, names of the kernels that ran)."""
    xf = G.to_frames(x_bct)
    b, c, t = x_bct.shape
    with _capi.profile() as prof:
        y = G.op_block(ctx, "l3ac_op_conv_unit", block, xf, (b, t, c), out=xf if in_place else None)
    return G.from_frames(y), [e["name"] for e in prof.entries]


def _fused_names(names):
    return [n for n in names if n.startswith("conv_unit") or n.startswith("wide_sliced")]


def _assert_validation_route(names, what):
    assert "grn_sumsq_kernel" in names and "grn_apply_kernel" in names, f"{what}: the two-pass GRN did not run: {names}"
    assert not _fused_names(names), f"{what}: a fused ConvUnit kernel ran on the validation route: {names}"


RMS_MIN_ELEMENTS = 64  # below this an output's rms error is not compared on its own (test_single_frame_rms_relation_at_the_narrow_widths)


def _both_forms(exact, fast, block, x, split):
    """The block on the validation-mode context and on the default one, on one GEMM route: (output, kernel names, guard after the call) of
    the first, (output, kernel names) of the second."""
    ctx_x, ctx_f = exact.network.context(), fast.network.context()
    try:
        ctx_x.set_gemm_split(split)
        ctx_f.set_gemm_split(split)
        exact.network.min_grn_norm(reset=True)
        got_x, names_x = _run(ctx_x, block, x)
        guard = exact.network.min_grn_norm()
        got_f, names_f = _run(ctx_f, block, x)
    finally:
        ctx_x.set_gemm_split(True)
        ctx_f.set_gemm_split(True)
    return got_x, names_x, guard, got_f, names_f


def _rms_relation(what, err_x, err_f, check=True):
    """The project's relation between two GPU forms of one function, on their errors against fp64: neither rms may exceed 1.5 x the other's + 1e-9."""
    e_x, e_f = _rms(err_x), _rms(err_f)
    print(f"[rms vs fp64 {what}] validation route {e_x:.3e} | fast form {e_f:.3e} | ratio {e_x / e_f:.3f}{'' if check else ' (printed only)'}")
    if check:
        assert e_x <= 1.5 * e_f + 1e-9, f"{what}: validation route rms {e_x:.3e} > 1.5 x fast form's {e_f:.3e}"
        assert e_f <= 1.5 * e_x + 1e-9, f"{what}: fast form rms {e_f:.3e} > 1.5 x validation route's {e_x:.3e}"


def _shapes(c):
    t_star = 2048 * 4 // c + 1  # the smallest T with T * C > 2048 * 4: several blocks per clip in both GRN kernels
    return [(1, 1), (3, 7), (2, 33), (5, t_star)]


# ---------------------------------------------------------------------------------------------------
# 1. the validation route against fp64, every width, both GEMM routes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,block,c", UNITS, ids=UNIT_IDS)
def test_validation_route_against_fp64(tag, block, c, models, monkeypatch):
    """l3ac_op_conv_unit on a grn_exact context against the fp64 oracle at the block tolerance, at one frame, odd clip lengths and a clip
    long enough for several blocks per clip in grn_sumsq_kernel / grn_apply_kernel (atomics, the channel index across blocks); the profile
    shows the two GRN kernels and no fused one, and the guard reports the reference's smallest norm (n == 1.0f here whatever the sum, so
    the guard is what sees a clip's partial or misattributed sum at these shapes).  The fast form of the same block (default context, same
    input; g >= 0.25 here, so the same function) is held to the same reference: at every shape and route neither one's rms error may
    exceed 1.5 x the other's + 1e-9.  Outputs of fewer than RMS_MIN_ELEMENTS numbers — the (1, 1) shape at C = 8, 24, 32 and 48 — are only
    printed here and asserted together in test_single_frame_rms_relation_at_the_narrow_widths."""
    exact, fast, w = models(tag)
    for b, t in _shapes(c):
        x = _rand((b, c, t), 7000 + 13 * c + t)
        ref, norms, _ = _unit_ref64(monkeypatch, w, block, x)
        assert float(norms.min()) >= 0.25, f"input condition: the reference's norms {norms.tolist()} must keep n == 1.0f"
        for split in (True, False):
            what = f"{tag} {block} C={c} B={b} T={t} {'bf16x3' if split else 'fp32'}"
            got_x, names_x, guard, got_f, names_f = _both_forms(exact, fast, block, x, split)
            _assert_validation_route(names_x, what)
            assert "grn_sumsq_kernel" not in names_f and "grn_apply_kernel" not in names_f, f"{what}: default context: {names_f}"
            _guard_matches(what, guard, float(norms.min()), guard_rtol(c))  # with several blocks per clip: a partial sum falls short by far more
            _close(f"exact {what}", got_x, ref)
            _close(f"fast  {what}", got_f, ref)
            _rms_relation(f"{what} ({', '.join(sorted(set(names_f)))})", got_x.double() - ref, got_f.double() - ref, check=ref.numel() >= RMS_MIN_ELEMENTS)


def test_single_frame_rms_relation_at_the_narrow_widths(models, monkeypatch):
    """The 1.5 x rms relation of test_validation_route_against_fp64 for the outputs it only prints: one frame of one clip at C = 8, 24, 24, 32
    and 48 is 8 .. 48 numbers, and the rms of so few scatters by more than the margin between two correct evaluations (24 numbers: about
    14 % each; measured at 1kbps C = 24, bf16x3: validation route 1.02e-7, fast form 1.61e-7, a ratio of 1.57, and 1.33 on the fp32 route,
    where every output of 64 numbers or more stayed below 1.22).  Their errors, of one size at these widths (1e-7 .. 2.3e-7 rms), are taken
    together per GEMM route, 136 numbers."""
    for split in (True, False):
        e_x, e_f = [], []
        for tag, block, c in UNITS:
            if c >= RMS_MIN_ELEMENTS:
                continue
            exact, fast, w = models(tag)
            x = _rand((1, c, 1), 7000 + 13 * c + 1)  # the (1, 1) input of test_validation_route_against_fp64
            ref, _, _ = _unit_ref64(monkeypatch, w, block, x)
            got_x, names_x, _, got_f, _ = _both_forms(exact, fast, block, x, split)
            _assert_validation_route(names_x, f"{tag} C={c}")
            e_x.append((got_x.double() - ref).flatten())
            e_f.append((got_f.double() - ref).flatten())
        _rms_relation(f"one frame, C < {RMS_MIN_ELEMENTS}, {'bf16x3' if split else 'fp32'}, {sum(e.numel() for e in e_x)} numbers", torch.cat(e_x), torch.cat(e_f))


# ---------------------------------------------------------------------------------------------------
# 2. the in-place route on default contexts (the same row route with EPI_SNAKE_GRN)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,block,c", [u for u in UNITS if u[0] == "1kbps" and u[2] != 256], ids=lambda v: str(v).split(".module")[0])
def test_in_place_route_on_default_contexts(tag, block, c, models, monkeypatch):
    """l3ac_op_conv_unit with x == y on a default context: no fused kernel may run (they cannot work in place), the unit takes the row route
    with the GRN folded into the first product's epilogue, and meets the block tolerance against fp64 on both GEMM routes (C = 256 is in
    test_gpu_blocks.py::test_conv_units_wide_fused)."""
    _, fast, w = models(tag)
    ctx = fast.network.context()
    for b, t in ((3, 7), (2, 33)):
        x = _rand((b, c, t), 8000 + 13 * c + t)
        ref, _, _ = _unit_ref64(monkeypatch, w, block, x)
        for split in (True, False):
            what = f"in place {block} C={c} B={b} T={t} {'bf16x3' if split else 'fp32'}"
            try:
                ctx.set_gemm_split(split)
                got, names = _run(ctx, block, x, in_place=True)
            finally:
                ctx.set_gemm_split(True)
            assert not _fused_names(names), f"{what}: a fused kernel ran on an in-place call: {names}"
            assert "dwconv_ln_kernel" in names and "grn_apply_kernel" not in names, f"{what}: not the row route with EPI_SNAKE_GRN: {names}"
            _close(what, got, ref)


# ---------------------------------------------------------------------------------------------------
# 3. the guard's value
# ---------------------------------------------------------------------------------------------------
def _three_clips(monkeypatch, w, block, c, seed):
    """B = 3, T = 3 input whose reference norms differ pairwise by at least 10 x the guard tolerance (asserted: a condition on the input)."""
    x = _rand((3, c, 3), seed)
    _, norms, _ = _unit_ref64(monkeypatch, w, block, x)
    tol = guard_rtol(c)
    for i in range(3):
        for j in range(i):
            gap = abs(float(norms[i] - norms[j])) / float(norms.min())
            assert gap >= 10 * tol, f"input condition: reference norms {norms.tolist()} too close for C={c} (gap {gap:.2e} < {10 * tol:.2e})"
    return x, norms


def _guard_matches(what, got, want, tol):
    rel = abs(got - want) / want
    print(f"[guard {what}] min_grn_norm {got:.9e} | reference {want:.9e} | relative difference {rel:.3e} (bound {tol:.3e})")
    assert math.isfinite(got) and rel <= tol, f"{what}: guard {got!r} != reference's smallest norm {want!r} (relative {rel:.3e} > {tol:.3e})"


@pytest.mark.parametrize("tag,block,c", UNITS, ids=UNIT_IDS)
def test_guard_equals_the_smallest_clip_norm_wherever_it_sits(tag, block, c, models, monkeypatch):
    """One call with three clips of different norms: min_grn_norm() is the reference's smallest per-clip norm within 2 (C + 64) 2^-24,
    with the smallest clip first, in the middle and last (the guard is taken by one thread per clip: one that looks at only some clips,
    or at another clip's sum, reports a value percents away)."""
    exact, _, w = models(tag)
    ctx = exact.network.context()
    x, norms = _three_clips(monkeypatch, w, block, c, 9000 + c)
    order = torch.argsort(norms).tolist()  # ascending: order[0] is the smallest clip
    print(f"[guard {tag} C={c}] reference norms {[f'{v:.6f}' for v in norms.tolist()]}")
    values = []
    for pos, perm in (("first", [order[0], order[1], order[2]]), ("middle", [order[2], order[0], order[1]]), ("last", [order[1], order[2], order[0]])):
        exact.network.min_grn_norm(reset=True)
        got, names = _run(ctx, block, x[perm])
        _assert_validation_route(names, f"{tag} C={c}")
        values.append(exact.network.min_grn_norm())
        _guard_matches(f"{tag} C={c} smallest clip {pos}", values[-1], float(norms.min()), guard_rtol(c))
    assert max(values) - min(values) <= 2 * 2.0 ** -24 * max(values), f"the guard moves with the clip's position: {values}"


def test_guard_across_calls_layers_and_reset(models, monkeypatch):
    """Two calls on different blocks without a reset give the smaller of the two reference minima; min_grn_norm(reset=True) returns that
    value and the next read, with no call in between, is +inf."""
    exact, _, w = models("1kbps")
    ctx = exact.network.context()
    (_, block_a, c_a), (_, block_b, c_b) = UNITS[0], UNITS[2]
    x_a, norms_a = _three_clips(monkeypatch, w, block_a, c_a, 9000 + c_a)
    x_b, norms_b = _three_clips(monkeypatch, w, block_b, c_b, 9000 + c_b)
    minima = {block_a: (float(norms_a.min()), c_a), block_b: (float(norms_b.min()), c_b)}
    want, c_min = min(minima.values())
    assert abs(minima[block_a][0] - minima[block_b][0]) / want >= 10 * guard_rtol(max(c_a, c_b)), "input condition: the two layers' minima must differ"
    for first, second in (((block_a, x_a), (block_b, x_b)), ((block_b, x_b), (block_a, x_a))):  # the smaller one first, then last
        exact.network.min_grn_norm(reset=True)
        _run(ctx, first[0], first[1])
        _guard_matches("after the first call", exact.network.min_grn_norm(), minima[first[0]][0], guard_rtol(minima[first[0]][1]))
        _run(ctx, second[0], second[1])
        _guard_matches("after both calls", exact.network.min_grn_norm(), want, guard_rtol(c_min))
        got = exact.network.min_grn_norm(reset=True)
        _guard_matches("returned by the reset", got, want, guard_rtol(c_min))
        after = exact.network.min_grn_norm()
        print(f"[guard] first read after the reset: {after}")
        assert after == float("inf")


@pytest.mark.parametrize("tag", ["tiny", "1kbps"])
@pytest.mark.parametrize("kind", ["noise", "silence"])
def test_guard_over_the_whole_network(tag, kind, models, monkeypatch):
    """encode_audio then decode_audio on 2 clips of 2 hops: the guard equals the smallest norm any GRN of the fp64 oracle's encoder and
    decoder saw.  The oracle decodes the features the GPU encoder returned (what the GPU decoder was given), so a token that falls the other
    way in fp64 cannot move the decoder's norms.  Relative tolerance: the block tolerance over the rms of the hidden tensor at the
    minimising layer (upstream activations carry the block-level error e per element: |dg| <= e sqrt(N), g = rms sqrt(N))."""
    exact, _, w = models(tag)
    mc = exact.network.mc
    audio = seeded_audio(2, 2 * mc.hop_length, seed=77) if kind == "noise" else torch.zeros(2, 2 * mc.hop_length)
    exact.network.min_grn_norm(reset=True)
    q, _ = exact.encode_audio(audio.cuda())
    g_enc = exact.network.min_grn_norm()
    exact.decode_audio(q)
    got = exact.network.min_grn_norm(reset=True)
    exact.decode_audio(q)
    g_dec = exact.network.min_grn_norm()  # the decoder's layers alone, wherever the minimum of both sits
    w64 = {k: v.double() for k, v in w.items()}
    rec = GrnRecorder(monkeypatch)
    O.encode_audio(w64, mc, audio.double())
    want_enc, rms_enc = rec.minimum()
    n_enc = len(rec.norms)
    O.decode_audio(w64, mc, audio_feature=q.cpu().double())
    want, rms_min = rec.minimum()
    print(f"[guard {tag} {kind}] {n_enc} encoder + {len(rec.norms) - n_enc} decoder GRN layers; hidden rms at the minimising layer {rms_min:.3e}")
    _guard_matches(f"{tag} {kind} encoder", g_enc, want_enc, ATOL_BLOCK / rms_enc)
    _guard_matches(f"{tag} {kind} encoder + decoder", got, want, ATOL_BLOCK / rms_min)
    del rec.norms[:n_enc], rec.rms[:n_enc]
    want_dec, rms_dec = rec.minimum()
    _guard_matches(f"{tag} {kind} decoder", g_dec, want_dec, ATOL_BLOCK / rms_dec)


# ---------------------------------------------------------------------------------------------------
# 4. the literal formula where it differs from 1: a doctored 1kbps model
# ---------------------------------------------------------------------------------------------------
# (block, C, target norm of the hidden tensor on x = 0, (B, T) = (2, 8)): the model's seven ConvUnits of widths 24, 96 and 256, every target once
DOCTORED = [("encoder.blocks.1.0.module", 24, 1e-8),
            ("encoder.blocks.5.0.module", 96, 1e-9), ("decoder.blocks.7.0.module", 96, 1e-6), ("decoder.blocks.7.1.module", 96, 0.0),
            ("decoder.blocks.4.0.module", 256, 1e-7), ("decoder.blocks.4.1.module", 256, 1e-2), ("decoder.blocks.4.2.module", 256, 1e-8)]
DOCTORED_IDS = [f"C{c}-g{g:g}" for _, c, g in DOCTORED]
DOCTORED_B, DOCTORED_T = 2, 8


def _doctor(sds, block, s):
    module, key = block.split(".", 1)
    sd = sds[module]
    sd[f"{key}.grn.gamma"] = torch.ones_like(sd[f"{key}.grn.gamma"])
    sd[f"{key}.grn.beta"] = torch.zeros_like(sd[f"{key}.grn.beta"])
    sd[f"{key}.pw_conv2.bias"] = torch.zeros_like(sd[f"{key}.pw_conv2.bias"])
    g = f"{key}.pw_conv1.parametrizations.weight.original0"  # weight-normed: the gain carries the scale
    sd[g] = (sd[g].double() * s).float()
    sd[f"{key}.pw_conv1.bias"] = (sd[f"{key}.pw_conv1.bias"].double() * s).float()


@pytest.fixture(scope="module")
def doctored():
    """One 1kbps state dict with seven doctored ConvUnits (gamma = 1, beta = 0, pw_conv2.bias = 0, pw_conv1 scaled by s), loaded on a
    validation-mode and on a default context.  s comes from the fp64 reference alone: the norm at s = 1 on x = 0, then one correction
    for the activation's quadratic term."""
    base = l3ac_amd.get_model("1kbps", synthetic_seed=0).network.state_dicts()

    def ref_norm(sds, block, c):
        with pytest.MonkeyPatch.context() as mp:
            _, norms, _ = _unit_ref64(mp, W.folded_weights(sds), block, torch.zeros(DOCTORED_B, c, DOCTORED_T))
        return float(norms[0])

    scales = {}
    for block, c, target in DOCTORED:
        s = 0.0
        if target > 0:
            trial = copy.deepcopy(base)
            _doctor(trial, block, 1.0)
            s = target / ref_norm(trial, block, c)
            trial = copy.deepcopy(base)
            _doctor(trial, block, s)
            s *= target / ref_norm(trial, block, c)
        scales[block] = s
    sds = copy.deepcopy(base)
    for block, _, _ in DOCTORED:
        _doctor(sds, block, scales[block])
    codecs = []
    for grn_exact in (True, False):
        codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
        codec.network.load_state_dicts(copy.deepcopy(sds))
        codec.network.grn_exact = grn_exact
        codec.network.to(device="cuda").eval()
        codecs.append(codec)
    return codecs[0], codecs[1], W.folded_weights(sds), scales


def _magnitude_metric(w, block, y, y_ref, h_ref):
    """|y - y_ref| / (|W2| @ |h'_ref|) per output element, (B, C, T): the error against the rows' magnitude sum of the second product."""
    mag = (h_ref.double().abs() @ w[f"{block}.pw_conv2.weight"].double().abs().T).permute(0, 2, 1)
    return (y.double() - y_ref).abs() / mag


SIN2_ABS = 2e-7  # the kernels' sin^2 against fp64: the bound test_gpu_blocks.py::test_sin_squared_range asserts for both of its forms


def _activation_term(w, block, x, norms, h_ref):
    """What the activation's absolute accuracy may add to the magnitude metric, per output element (B, C, T).  snake(v) = v + sin^2(alpha v)
    / alpha is evaluated with a sin^2 that is accurate to SIN2_ABS absolutely, not relatively (the packed form takes it as (1 - cos 2u) / 2),
    and that errs by at most sin^2(u) <= u^2 itself where sin^2 is below that granularity (it returns 0 there).  So a hidden element may be
    off by min(SIN2_ABS, u^2) / alpha, u = alpha v from the fp64 reference: nothing at O(1) activations or at g <= 1e-6, far more than the
    fp32 rounding of the products where the hidden elements are of order 1e-4 (g = 1e-2).

    Measured at C = 256, g = 1e-2, without this term: the validation route's max error was 172 x (bf16x3) and 170 x (fp32 route) the fp32
    CPU oracle's, its rms 180 x; the fast path's 170 x and 169 x (8.4e-6 .. 8.6e-6 of the magnitude sum against the oracle's 5.0e-8) — all
    four evaluations, since both GEMM families' epilogues use the packed form.  The term is a worst case over signs, 1.5e-4 there, 17 x the
    measured error, so after the subtraction nothing is left (ratios 0.00): at that norm the comparison bounds the error at 1.5e-4 of the
    magnitude sum and no tighter.  At every other norm the term is below the oracle's own error (at most 2.4e-8 against 7.9e-8, at g = 1e-6)
    and the GPU met the margins without it (max 0.71 .. 2.97 x, _margins), so _doctored_case leaves it out there: it returns zeros unless
    the term's largest element exceeds the fp32 oracle's largest error."""
    wb = _w64(w, block)
    c = x.shape[1]
    v = torch.nn.functional.conv1d(x.double(), wb[f"{block}.dw_conv.weight"], wb[f"{block}.dw_conv.bias"], padding=3, groups=c).permute(0, 2, 1)
    v = O.channel_norm_last(v, wb[f"{block}.norm.weight"], wb[f"{block}.norm.bias"])
    v = torch.nn.functional.linear(v, wb[f"{block}.pw_conv1.weight"], wb[f"{block}.pw_conv1.bias"])
    alpha = wb[f"{block}.act.alpha"]
    n = (norms / (norms + 1e-8)).view(-1, 1, 1)
    e = (alpha * v).pow(2).clamp_max(SIN2_ABS) * (alpha + O.EPS).reciprocal().abs() * (1 + n)
    w2 = wb[f"{block}.pw_conv2.weight"].abs()
    return ((e @ w2.T) / (h_ref.double().abs() @ w2.T)).permute(0, 2, 1)


def _doctored_case(monkeypatch, w, block, x):
    """fp64 reference of a doctored unit, the fp32 CPU oracle's error against it in the magnitude metric and the activation's term in that
    metric: (y64, norms, h'64, metric32, activation term)."""
    y64, norms, h64 = _unit_ref64(monkeypatch, w, block, x)
    y32 = O.conv_unit({k: v for k, v in w.items() if k.startswith(block)}, block, x.float())
    m32 = _magnitude_metric(w, block, y32, y64, h64)
    act = None
    if float(norms.min()) > 0:
        act = _activation_term(w, block, x, norms, h64)
        if float(act.max()) <= float(m32.max()):  # below the reference's own rounding: the margins hold without it
            act = torch.zeros_like(act)
    return y64, norms, h64, m32, act


def _margins(c):
    """(max, rms) factors over the fp32 CPU oracle's error.  The project's margins between two evaluations of one function (test_sin_squared_range,
    the form comparisons) are 2 x on the max and 1.5 x on the rms, and they hold at C = 24 and 96 (measured ratios: max 0.71 .. 1.52, rms
    0.76 .. 1.40).  At C = 256 the GPU measured max 1.73 .. 2.97 x and rms 1.44 .. 1.96 x the oracle's, with no bug: the second product sums
    K = 1024 terms, which the CPU's BLAS spreads over many partial sums (vector lanes times unrolling) where the matrix cores run one fp32
    chain per output, so the oracle's own error (0.5e-7 of the magnitude sum, under one ulp) is no longer the size of a correct fp32
    product's (the GPU's 0.9e-7 .. 1.5e-7 is well inside the 4e-7 test_gemm_against_fp64 allows in this metric).  There the margins are
    doubled, to 4 x and 3 x."""
    return (2.0, 1.5) if c < 256 else (4.0, 3.0)


def _allowance(what, c, m_gpu, m_32, act):
    """The GPU's error against fp64 in the magnitude metric, less the activation's term, within _margins of the fp32 CPU oracle's."""
    f_max, f_rms = _margins(c)
    rest = (m_gpu - act).clamp_min(0.0)
    print(f"[{what}] err / magnitude sum vs fp64: GPU max {float(m_gpu.max()):.3e} rms {_rms(m_gpu):.3e} | fp32 oracle max {float(m_32.max()):.3e} rms {_rms(m_32):.3e}"
          f" | ratios max {float(m_gpu.max() / m_32.max()):.2f} rms {_rms(m_gpu) / _rms(m_32):.2f} | activation term max {float(act.max()):.3e};"
          f" without it: ratios max {float(rest.max() / m_32.max()):.2f} rms {_rms(rest) / _rms(m_32):.2f} (allowed {f_max:g}, {f_rms:g})")
    return float(rest.max()) <= f_max * float(m_32.max()) and _rms(rest) <= f_rms * _rms(m_32)


@pytest.mark.parametrize("block,c,target", DOCTORED, ids=DOCTORED_IDS)
def test_literal_formula_at_small_norms(block, c, target, doctored, monkeypatch):
    """x = 0 removes the O(1) residual, so the output is W2 . h (1 + n), of the hidden tensor's order, and n = g / (g + 1e-8) moves it by a
    factor between 1 and 2.  The validation route must follow the fp64 oracle as closely as the fp32 CPU oracle does (max <= 2 x, rms
    <= 1.5 x its error over the second product's magnitude sum; the docstrings of _margins and _activation_term say where and why the GPU
    is given more, each with the ratios measured), on both GEMM routes, and the guard must report the reference's norm; at
    g = 0 the guard is exactly 0.0 and the output exactly the reference's (0 / (0 + 1e-8) = 0: no NaN).  The comparison can see n: the
    fast path on the same weights misses the reference by more than 10 x the allowance at g = 1e-8 and 1e-9 — its documented assumption,
    not a defect — and passes it at g = 1e-2, where n differs from 1 by 1e-6."""
    exact, fast, w, scales = doctored
    x = torch.zeros(DOCTORED_B, c, DOCTORED_T)
    y64, norms, h64, m32, act = _doctored_case(monkeypatch, w, block, x)
    g_ref = float(norms.min())
    print(f"[doctored {block} C={c}] s = {scales[block]:.6e}; reference norms {norms.tolist()} (target {target:g}); max|y_ref| {float(y64.abs().max()):.3e}")
    if target == 0.0:
        assert g_ref == 0.0 and float(y64.abs().max()) == 0.0
    else:
        assert target / 2 <= g_ref <= target * 2 and g_ref >= 1e-10, f"input condition: reference norm {g_ref:.3e} is not within a factor 2 of {target:g}"
    for split in (True, False):
        what = f"doctored C={c} g={target:g} {'bf16x3' if split else 'fp32'}"
        ctx = exact.network.context()
        exact.network.min_grn_norm(reset=True)
        try:
            ctx.set_gemm_split(split)
            got, names = _run(ctx, block, x)
        finally:
            ctx.set_gemm_split(True)
        guard = exact.network.min_grn_norm()
        _assert_validation_route(names, what)
        assert torch.isfinite(got).all(), f"{what}: non-finite output"
        if target == 0.0:
            print(f"[{what}] guard {guard!r}; max|y| {float(got.abs().max())!r}")
            assert guard == 0.0 and torch.equal(got.double(), y64)
            continue
        _guard_matches(what, guard, g_ref, guard_rtol(c))
        assert _allowance(f"exact {what}", c, _magnitude_metric(w, block, got, y64, h64), m32, act), f"{what}: the validation route misses the fp32 oracle's allowance"
        if target in (1e-8, 1e-9, 1e-2):
            ctx_f = fast.network.context()
            try:
                ctx_f.set_gemm_split(split)
                got_f, names_f = _run(ctx_f, block, x)
            finally:
                ctx_f.set_gemm_split(True)
            assert "grn_apply_kernel" not in names_f
            m_f = _magnitude_metric(w, block, got_f, y64, h64)
            if target == 1e-2:
                assert _allowance(f"fast  {what}", c, m_f, m32, act), f"{what}: the fast path misses the allowance where n = 1 - 1e-6"
            else:
                print(f"[fast  {what}] err / magnitude sum: max {float(m_f.max()):.3e} = {float(m_f.max() / m32.max()):.0f} x the fp32 oracle's max (n = {g_ref / (g_ref + 1e-8):.3f} taken as 1)")
                assert float(m_f.max()) > 10 * (_margins(c)[0] * float(m32.max()) + float(act.max())), f"{what}: the comparison cannot see the normaliser"


# ---------------------------------------------------------------------------------------------------
# 5. clips do not share a normaliser
# ---------------------------------------------------------------------------------------------------
def test_a_clip_alone_equals_the_same_clip_in_a_batch(models, monkeypatch):
    """The validation route at C = 96 on the shipped gamma: each clip run alone equals the same clip inside a batch of three (clip 1 drawn from
    another seed, three times as loud) within 2 x 2^-24 relative (the atomics leave the order of a clip's partial sums free, so bits are not
    required).  With g far above 0.25 the normaliser is 1.0f whatever sum a clip is given, so the OUTPUTS here show only that the rows of
    different clips do not mix; a shared or swapped sum is seen by the guard, which must report each clip's own reference norm when it runs
    alone and the smallest of the three for the batch, and by test_a_tiny_clip_between_two_others_keeps_its_own_normaliser."""
    exact, _, w = models("1kbps")
    ctx = exact.network.context()
    _, block, c = UNITS[2]
    for t in (33, 2048 * 4 // c + 1):  # one block per clip, several
        x = _rand((3, c, t), 5100 + t)
        x[1] = _rand((c, t), 5200 + t, 3.0)
        _, norms, _ = _unit_ref64(monkeypatch, w, block, x)
        exact.network.min_grn_norm(reset=True)
        batch, names = _run(ctx, block, x)
        _assert_validation_route(names, f"C={c} T={t}")
        _guard_matches(f"batch of three, C={c} T={t}", exact.network.min_grn_norm(reset=True), float(norms.min()), guard_rtol(c))
        for i in range(3):
            alone, _ = _run(ctx, block, x[i:i + 1])
            _guard_matches(f"clip {i} alone, C={c} T={t}", exact.network.min_grn_norm(reset=True), float(norms[i]), guard_rtol(c))
            rel = float(((alone[0] - batch[i]).abs() / batch[i].abs().clamp_min(1e-30)).max())
            print(f"[clip {i} alone vs in the batch, C={c} T={t}] max relative difference {rel:.3e}")
            assert rel <= 2 * 2.0 ** -24, f"clip {i} alone differs from the same clip in the batch (T={t}): {rel:.3e}"


@pytest.mark.parametrize("block,c,target", [d for d in DOCTORED if d[2] == 1e-8], ids=[i for i, d in zip(DOCTORED_IDS, DOCTORED) if d[2] == 1e-8])
def test_a_tiny_clip_between_two_others_keeps_its_own_normaliser(block, c, target, doctored, monkeypatch):
    """The doctored unit at g = 1e-8, B = 3: clip 1 is x = 0, clips 0 and 2 seeded noise, whose hidden tensors have other norms.  Clip 1 must
    meet the allowance of test_literal_formula_at_small_norms with its own n = 0.5 (a shared or swapped sum gives it another clip's), the
    guard reports the batch's smallest reference norm, and the noise clips meet the block tolerance."""
    exact, _, w, _ = doctored
    x = _rand((3, c, DOCTORED_T), 6100 + c)
    x[1] = 0.0
    y64, norms, h64, m32, act = _doctored_case(monkeypatch, w, block, x)
    n_ref = norms / (norms + 1e-8)
    print(f"[doctored batch C={c}] reference norms {norms.tolist()} -> n {n_ref.tolist()}")
    assert target / 2 <= float(norms[1]) <= target * 2
    assert min(abs(float(n_ref[1] - n_ref[0])), abs(float(n_ref[1] - n_ref[2]))) >= 1e-3, "input condition: the clips' normalisers must differ by far more than the allowance"
    for split in (True, False):
        what = f"doctored batch C={c} {'bf16x3' if split else 'fp32'}"
        ctx = exact.network.context()
        exact.network.min_grn_norm(reset=True)
        try:
            ctx.set_gemm_split(split)
            got, names = _run(ctx, block, x)
        finally:
            ctx.set_gemm_split(True)
        _assert_validation_route(names, what)
        _guard_matches(what, exact.network.min_grn_norm(), float(norms.min()), guard_rtol(c))
        m = _magnitude_metric(w, block, got, y64, h64)
        assert _allowance(f"clip 1 of the {what}", c, m[1], m32[1], act[1]), f"{what}: clip 1 misses the allowance: another clip's normaliser?"
        _close(f"noise clips of the {what}", got[[0, 2]], y64[[0, 2]])
