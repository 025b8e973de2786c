#!/usr/bin/env python3
"""Batches of long recordings: B recordings with seeded lengths uniform in --min-s .. --max-s seconds, encoded
and decoded (from indices) two ways, on the same recordings:
  long   one encode_long + one decode_long for the batch (chunks of all recordings as rows of ragged calls)
  loop   extract_unit + decode_unit per recording, one recording after the other (the only way before encode_long)
and the cut / merge kernels alone against a device-to-device copy of the same bytes in the same run:
  audio     l3ac_chunk_cut of every chunk of the batch's audio (c = 1, chunk starts only 4-byte aligned)
  features  l3ac_chunk_merge of every chunk's token features (c = feature_dim, 16-byte accesses)
`long` and `loop` are checked bit-equal before anything is timed.  Timings: device events around one pass, --reps passes per
variant after --warm, the variants alternating pass by pass; the JSON line gives each variant's median and its min .. max."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import l3ac_amd
from l3ac_amd import _capi
from l3ac_amd.chunking import ChunkData


def alternate(fns, reps, warm):
    """{name: [ms per pass]}: every variant `warm` times untimed, then `reps` rounds of one timed pass of each in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "passes": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="1kbps")
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=10.0)
    ap.add_argument("--max-s", type=float, default=120.0)
    ap.add_argument("--window", type=int, default=5 * 16000)
    ap.add_argument("--prefix-tokens", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    codec = l3ac_amd.get_model(args.config, synthetic_seed=0)
    codec.network.to(device="cuda").eval()
    mc = codec.network.mc
    hop, sr = mc.hop_length, codec.config.sample_rate
    rng = np.random.default_rng(args.seed)
    lengths = [int(v) for v in rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, size=args.recordings)]
    t = max(lengths)
    g = torch.Generator().manual_seed(args.seed)
    audio = (torch.rand(args.recordings, t, generator=g) - 0.5).cuda()
    for i, n in enumerate(lengths):
        audio[i, n:] = 0
    kw = dict(process_window=args.window, prefix_tokens=args.prefix_tokens)
    chunk_len, prefix_tokens, per_call = codec._long_plan(args.window, args.prefix_tokens, None)
    row_samples = chunk_len + prefix_tokens * hop
    codec.network.context().reserve(per_call, row_samples)
    clips = [audio[i:i + 1, :n] for i, n in enumerate(lengths)]

    def long():
        _, ind = codec.encode_long(audio, lengths=lengths, **kw)
        return ind, codec.decode_long(indices=ind["indices"], lengths=ind["lengths"], **kw)

    def loop():
        for clip in clips:
            idx, _ = codec.extract_unit(clip, **kw)
            codec.decode_unit(chunk_indices=idx)

    # bit-equality first: each row of `long` against the recording alone
    ind, wave = long()
    for i, clip in enumerate(clips):
        idx, _ = codec.extract_unit(clip, **kw)
        k = int(ind["lengths"][i])
        assert torch.equal(ind["indices"][i, :k], idx.data), f"recording {i}: indices differ"
        alone = codec.decode_unit(chunk_indices=ChunkData(chunk_len // hop, prefix_tokens, original_data=ind["indices"][i, :k]))
        assert torch.equal(wave[i, :k * hop], alone[0]), f"recording {i}: waveform differs"
    n_tok = ind["indices"].shape[1]
    del wave

    cut = l3ac_amd.chunk_plan(lengths, chunk_len, prefix_tokens * hop, hop)
    merge = l3ac_amd.chunk_plan(ind["lengths"].tolist(), chunk_len // hop, prefix_tokens, 1)
    n = len(cut)
    out = {"config": args.config, "recordings": args.recordings, "seconds": round(sum(lengths) / sr, 1), "chunks": n,
           "chunk_row_seconds": round(sum(d.frames for d in cut) / sr, 1), "process_window": args.window, "prefix_tokens": prefix_tokens,
           "chunks_per_call": per_call, "bit_equal": True}

    ms = alternate({"long": long, "loop": loop}, args.reps, args.warm)
    for name, v in ms.items():
        out[name] = summary(v)
    out["loop_over_long"] = round(out["loop"]["median_ms"] / out["long"]["median_ms"], 2)

    # the kernels alone against a device-to-device copy of the same bytes
    lib = _capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    rows = torch.empty((n, -(-row_samples // 4) * 4), dtype=torch.float32, device="cuda")
    moved = sum(d.frames for d in cut)
    flat_src, flat_dst = torch.rand(moved, device="cuda"), torch.empty(moved, device="cuda")
    feat = mc.feature_dim
    row_tok = row_samples // hop
    q_rows = torch.rand((n, row_tok, feat), device="cuda")
    q_out = torch.empty((args.recordings, n_tok, feat), device="cuda")
    own = sum(d.frames - d.prefix for d in merge) * feat            # elements copied: read and written
    zeroed = args.recordings * n_tok * feat - own                    # elements of the tails: written only
    f_elems = own + zeroed // 2                                      # a copy that moves the same bytes
    f_src, f_dst = torch.rand(f_elems, device="cuda"), torch.empty(f_elems, device="cuda")
    inner = 20  # launches per timed pass: one launch is a fraction of a millisecond

    def times(fn):
        def run():
            for _ in range(inner):
                fn()
        return run

    k = alternate({name: times(fn) for name, fn in {
        "audio_cut": lambda: _capi.check(lib.l3ac_chunk_cut(audio.data_ptr(), args.recordings, audio.stride(0), 1, cut, n, rows.data_ptr(), n,
                                                            rows.stride(0), stream)),
        "audio_copy": lambda: flat_dst.copy_(flat_src),
        "feature_merge": lambda: _capi.check(lib.l3ac_chunk_merge(q_rows.data_ptr(), n, row_tok, feat, merge, n, q_out.data_ptr(),
                                                                  args.recordings, n_tok, n_tok, stream)),
        "feature_copy": lambda: f_dst.copy_(f_src),
    }.items()}, max(args.reps, 10), 2)
    k = {name: [v / inner for v in ms] for name, ms in k.items()}
    for name, elements in (("audio_cut", moved), ("audio_copy", moved), ("feature_merge", f_elems), ("feature_copy", f_elems)):
        s = summary(k[name])
        s["bytes"] = 8 * elements  # 4 read + 4 written per element moved (feature_merge: its zero tails count as written only)
        s["gb_per_s"] = round(8.0 * elements / (s["median_ms"] * 1e-3) / 1e9, 1)
        out[name] = s
    out["audio_cut_over_copy"] = round(out["audio_cut"]["gb_per_s"] / out["audio_copy"]["gb_per_s"], 3)
    out["feature_merge_over_copy"] = round(out["feature_merge"]["gb_per_s"] / out["feature_copy"]["gb_per_s"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
