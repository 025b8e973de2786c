#!/usr/bin/env python3
"""Ragged batches: 256 clips with seeded lengths uniform in 0.5 - 2 s, encoded and decoded (from indices)
three ways, on the same clips:
  ragged   one encode_audio / decode_audio call with lengths=
  padded   one plain call on the batch zero-padded to its longest clip (what padding costs; its tokens near a clip's end are wrong)
  grouped  one plain call per distinct length, the clips of that length as a batch (the correct way without lengths=)
Every timing is device events around `reps` repetitions after `warm`; ms per repetition of the whole 256-clip encode + decode.
Prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import l3ac_amd


def time_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="1kbps")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    codec = l3ac_amd.get_model(args.config, synthetic_seed=0)
    codec.network.to(device="cuda").eval()
    sr = codec.config.sample_rate
    rng = np.random.default_rng(args.seed)
    lengths = [int(v) for v in rng.integers(sr // 2, 2 * sr + 1, size=args.clips)]
    t = max(lengths)
    g = torch.Generator().manual_seed(args.seed)
    audio = (torch.rand(args.clips, t, generator=g) - 0.5).cuda()
    for i, n in enumerate(lengths):
        audio[i, n:] = 0
    codec.network.context().reserve(args.clips, t)

    def ragged():
        _, ind = codec.encode_audio(audio, lengths=lengths)
        codec.decode_audio(indices=ind["indices"], lengths=ind["lengths"])

    def padded():
        _, ind = codec.encode_audio(audio)
        codec.decode_audio(indices=ind["indices"])

    groups = {}
    for i, n in enumerate(lengths):
        groups.setdefault(n, []).append(i)
    batches = [(n, audio[idx, :n].contiguous()) for n, idx in groups.items()]

    def grouped():
        for _, a in batches:
            _, ind = codec.encode_audio(a)
            codec.decode_audio(indices=ind["indices"])

    out = {"config": args.config, "clips": args.clips, "seconds": round(sum(lengths) / sr, 2), "distinct_lengths": len(groups)}
    for name, fn in (("ragged", ragged), ("padded", padded), ("grouped", grouped)):
        out[f"{name}_ms"] = round(time_ms(fn, args.reps if name != "grouped" else max(1, args.reps // 2), args.warm), 3)
    out["ragged_over_padded"] = round(out["ragged_ms"] / out["padded_ms"], 3)
    out["grouped_over_ragged"] = round(out["grouped_ms"] / out["ragged_ms"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
