"""Which kernels a call launches, and how often: the profiler's entries of a fixed table of calls, as (name, launches) pairs in the order
of each name's first launch, against tests/golden/dispatch_launches.json (needs an MI355X: `pytest -m gpu`).

The host code that turns a call into launches (csrc/network.hip, the context entries of csrc/capi.hip, launch_wide in
csrc/kernels/conv_unit_wide.hip) decides a form per block from the shape, the context's options and the device's CU count.  This file
pins those decisions: a change to that host code that is meant to leave every launch alone leaves this file green, and one that is
meant to move a launch re-records the fixture (`python -m tests.test_gpu_dispatch --record`, on the commit BEFORE the change when the
change is a refactor) and shows the move in the fixture's diff.  Names and launch counts only, never times.

The table:
* codec calls -- encode_audio and decode_audio of the 1kbps and 3kbps synthetic models on one clip of one second and on a ragged batch
  of three clips of unequal length, with every option at its default and then with one option changed at a time (OPTIONS).
* the wide ConvUnit's forms (wide_plan in conv_unit_wide.hip) through l3ac_op_conv_unit, see wide_table.
* the block entries whose workspace is sized by workspace_ensure_op, at (B, T) = (2, 64), see block_table.

The fixture holds the device's CU count it was recorded on (256): wide_plan's half-tile rule reads it, so on another count the wide
table is not comparable and the test says so instead of reporting moved launches.
"""
import gc
import json
import sys

import pytest
import torch

import l3ac_amd
from l3ac_amd import _capi
from tests import gpu_ops as G
from tests.helpers import GOLDEN, seeded_audio

pytestmark = pytest.mark.gpu

FIXTURE = GOLDEN / "dispatch_launches.json"
MODELS = ("1kbps", "3kbps")
OPTIONS = ((None, None), ("gemm_split", 0), ("narrow_ring", 0), ("narrow_ring", 2), ("wide_sliced", 0), ("wide_sliced", 2),
           ("unit_counter", 0), ("unit_counter", 2), ("unit_counter", 3), ("down_fused", 0), ("trans_coop", 0))
RAGGED_SAMPLES = (16000, 11111, 5000)


def profiled(fn):
    torch.cuda.synchronize()
    with _capi.profile() as p:
        fn()
        torch.cuda.synchronize()
    return [[e["name"], e["launches"]] for e in p.entries]


class option:
    """one option of the context changed for the duration of a block (None: every option at its default)"""

    def __init__(self, ctx, name, value):
        self.ctx, self.name, self.value = ctx, name, value

    def __enter__(self):
        if self.name is not None:
            self.before = self.ctx.get_option(self.name)
            self.ctx.set_option(self.name, self.value)
        return "defaults" if self.name is None else f"{self.name}={self.value}"

    def __exit__(self, *exc):
        if self.name is not None:
            self.ctx.set_option(self.name, self.before)
        return False


def model_on_gpu(name):
    """The model with the only live context of this file (and, after gc, of the process): a context keeps the CUs its cooperative
    transformer launches claimed until it is closed, and a launch whose claim no longer fits the device takes the one-workgroup form,
    under another profiler name."""
    gc.collect()
    codec = l3ac_amd.get_model(name, synthetic_seed=0)
    codec.network.to(device="cuda").eval()
    return codec


def codec_table(name, emit):
    codec = model_on_gpu(name)
    try:
        ctx = codec.network.context()
        audio = seeded_audio(3, max(RAGGED_SAMPLES)).cuda()
        one, lens = audio[:1].contiguous(), list(RAGGED_SAMPLES)
        ind_one = codec.encode_audio(one)[1]["indices"]
        ragged = codec.encode_audio(audio, lengths=lens)[1]
        for opt, value in OPTIONS:
            with option(ctx, opt, value) as tag:
                emit(f"{name}/{tag}/encode 1x1s", lambda: codec.encode_audio(one))
                emit(f"{name}/{tag}/decode 1x1s", lambda: codec.decode_audio(indices=ind_one))
                emit(f"{name}/{tag}/encode ragged", lambda: codec.encode_audio(audio, lengths=lens))
                emit(f"{name}/{tag}/decode ragged", lambda: codec.decode_audio(indices=ragged["indices"], lengths=ragged["lengths"]))
    finally:
        codec.network.cpu()  # closes the context


def wide_table(emit):
    """l3ac_op_conv_unit on the wide fused kernel's widths, one call per form of wide_plan.  On 256 CUs, with T = 900 and C = 256
    (one workgroup per CU, passes of 4 x 256 = 1024 tiles of 32 frames, the sliced form up to 256 tiles of 16 frames), re-derived
    from wide_plan:
      B =  1:    900 rows,   57 tiles16 <= 256                            -> all sliced  (wide_sliced 0: 29 tiles, 8 blocks: half tiles)
      B =  5:  4 500 rows,  282 tiles16 > 256; 141 tiles, 36 blocks, 72 <= 256 -> half tiles
      B = 20: 18 000 rows,  563 tiles, 141 blocks, 282 > 256; no full pass      -> one partial pass, 141 workgroups
      B = 40: 36 000 rows, 1125 tiles = 1024 + 101, 2 x 101 <= 256              -> passes + sliced tail
      B = 44: 39 600 rows, 1238 tiles = 1024 + 214, 428 > 256, 428 <= 1024      -> passes + half-tile tail
      B = 56: 50 400 rows, 1575 tiles = 1024 + 551, 1102 > 1024                 -> passes, the remainder as a second pass
    Only B = 1 changes with wide_sliced: 0 never takes the sliced form for a whole call and 2 equals 1 below 256 tiles16.  The sliced
    TAIL at B = 40 does not read the option, so it is the same under all three.
    C = 96 (two workgroups per CU, front end inside the kernel, units by counter where the context hands counters in), T = 2700:
      B = 31: 83 700 rows, 2616 tiles, 512 workgroups, 2616 > 4 x 512 -> passes by counter (unit_counter 1), lock-step passes (0)
      B =  1:  2 700 rows,  169 tiles16                              -> all sliced"""
    codec = model_on_gpu("1kbps")
    try:
        ctx = codec.network.context()
        x = torch.zeros((56, 900, 256), dtype=torch.float32, device="cuda")
        for sliced in (1, 0, 2):
            with option(ctx, "wide_sliced", sliced) as tag:
                for b in (1, 5, 20, 40, 44, 56):
                    emit(f"wide/C=256 {b}x900 {tag}", lambda: G.op_block(ctx, "l3ac_op_conv_unit", "decoder.blocks.4.1.module", x[:b], (b, 900, 256)))
        x = torch.zeros((31, 2700, 96), dtype=torch.float32, device="cuda")
        for counter in (0, 1):
            with option(ctx, "unit_counter", counter) as tag:
                emit(f"wide/C=96 31x2700 {tag}", lambda: G.op_block(ctx, "l3ac_op_conv_unit", "decoder.blocks.7.0.module", x, (31, 2700, 96)))
        emit("wide/C=96 1x2700", lambda: G.op_block(ctx, "l3ac_op_conv_unit", "decoder.blocks.7.0.module", x[:1], (1, 2700, 96)))
    finally:
        codec.network.cpu()


def block_table(emit):
    """every EnhanceBlock, up layer and pair of the two of the 1kbps decoder, its three LegacyUnits, its head and its last block"""
    codec = model_on_gpu("1kbps")
    try:
        ctx = codec.network.context()
        b, t = 2, 64
        zeros = lambda c: torch.zeros((b, t, c), dtype=torch.float32, device="cuda")
        dims, rates = codec.network.mc.decoder_dims, codec.network.mc.decode_rates
        for i in range(len(dims) - 1):
            eb, ub, ci, co, s = f"decoder.blocks.{2 + 3 * i}", f"decoder.blocks.{3 + 3 * i}", dims[i], dims[i + 1], rates[i]
            emit(f"block/l3ac_op_enhance {eb}", lambda: G.op_block(ctx, "l3ac_op_enhance", eb, zeros(ci), (b, t, ci)))
            emit(f"block/l3ac_op_up_layer {ub}", lambda: G.op_block(ctx, "l3ac_op_up_layer", ub, zeros(ci), (b, t * s, co)))
            emit(f"block/l3ac_op_enhance_up {eb} {ub}", lambda: G.op_block2(ctx, "l3ac_op_enhance_up", eb, ub, zeros(ci), (b, t * s, co)))
        for unit in range(3):
            emit(f"block/l3ac_op_legacy_unit {unit}", lambda: G.legacy_unit(ctx, unit, zeros(dims[-1])))
        emit("block/l3ac_op_head", lambda: G.head(ctx, zeros(dims[-1])))
        emit("block/l3ac_op_last_block", lambda: G.op_plain(ctx, "l3ac_op_last_block", zeros(dims[-1]), b, t, (b, t)))
    finally:
        codec.network.cpu()


TABLES = {**{f"{name}/": (lambda emit, name=name: codec_table(name, emit)) for name in MODELS}, "wide/": wide_table, "block/": block_table}


def run(prefix):
    got = {}

    def emit(call, fn):
        assert call.startswith(prefix) and call not in got, call
        got[call] = profiled(fn)

    TABLES[prefix](emit)
    return got


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("prefix", list(TABLES))
def test_launches_equal_the_recorded_ones(prefix):
    golden = json.loads(FIXTURE.read_text())
    assert cu_count() == golden["cu_count"], f"the fixture was recorded on {golden['cu_count']} CUs, this device has {cu_count()}"
    want = {k: v for k, v in golden["calls"].items() if k.startswith(prefix)}
    got = run(prefix)
    assert sorted(got) == sorted(want), f"the table's calls and the fixture's differ: {sorted(set(got) ^ set(want))}"
    moved = {k: {"launched": got[k], "recorded": want[k]} for k in want if got[k] != want[k]}
    assert not moved, f"{len(moved)} of {len(want)} calls launch something else than recorded:\n{json.dumps(moved, indent=1)}"


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit(f"usage: python -m tests.test_gpu_dispatch --record [PATH]   (default {FIXTURE})")
    calls = {}
    for prefix in TABLES:
        calls.update(run(prefix))
    out = FIXTURE if len(sys.argv) < 3 else sys.argv[2]
    with open(out, "w") as f:
        json.dump({"cu_count": cu_count(), "calls": calls}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(calls)} calls on {cu_count()} CUs into {out}")
