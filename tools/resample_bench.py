#!/usr/bin/env python3
"""Micro-benchmark of the sample-rate conversion kernel (kernels/resample.hip) on 256 clips x 1 s, next to a device copy of the
same bytes measured in the same run; the 1kbps encode + decode step with 48 kHz in and out against the plain 16 kHz step
(alternated); and scipy.signal.resample_poly on the CPU for the same input, when scipy is present.

Every timing is device events around `reps` launches after `warm` launches.  "cold": each launch reads a different one of a set of
input buffers that together exceed the 256 MiB Infinity Cache (and writes a different output); "warm": the same buffers every time.
Kernel-only times: run with --kernels-only under `rocprofv3 --kernel-trace --stats` (resample_poly_kernel)."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import l3ac_amd

PAIRS = [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 48000)]
CLIPS = 256
ROTATE_BYTES = 512 << 20  # > the 256 MiB Infinity Cache


def time_ms(fn, n_bufs, reps, warm):
    for i in range(warm):
        fn(i % n_bufs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fn(i % n_bufs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_pairs(dev, reps, warm, out):
    g = torch.Generator(device=dev).manual_seed(0)
    for a, b in PAIRS:
        n_out = l3ac_amd.resample_length(a, b, a)
        nbytes = 4 * CLIPS * (a + n_out)  # algorithmic: every input read once, every output written once
        n_bufs = max(2, -(-ROTATE_BYTES // nbytes))
        xs = [torch.randn(CLIPS, a, device=dev, generator=g) * 0.3 for _ in range(n_bufs)]
        ys = [torch.empty(CLIPS, n_out, device=dev) for _ in range(n_bufs)]
        half = nbytes // 8  # a copy of nbytes / 2 reads and writes nbytes in all
        cs = [torch.empty(half, device=dev) for _ in range(n_bufs)]
        cd = [torch.empty(half, device=dev) for _ in range(n_bufs)]
        lib = l3ac_amd._capi.load_library()
        bank = l3ac_amd._resample_bank(torch.device(dev), a, b)
        stream = torch.cuda.current_stream().cuda_stream

        def run(i):  # the kernel alone, as resample() launches it, without the output allocation
            lib.l3ac_resample(xs[i].data_ptr(), CLIPS, a, a, a, b, bank.data_ptr(), ys[i].data_ptr(), n_out, stream)

        res = {"pair": f"{a}->{b}", "bytes": nbytes, "buffers_cold": n_bufs}
        for mode, nb in (("cold", n_bufs), ("warm", 1)):
            for rnd in range(2):  # interleaved with the copy, twice
                k = time_ms(run, nb, reps, warm)
                c = time_ms(lambda i: cd[i].copy_(cs[i]), nb, reps, warm)
                res.setdefault(f"{mode}_kernel_us", []).append(round(k * 1e3, 2))
                res.setdefault(f"{mode}_copy_us", []).append(round(c * 1e3, 2))
            kmin, cmin = min(res[f"{mode}_kernel_us"]), min(res[f"{mode}_copy_us"])
            res[f"{mode}_kernel_GBps"] = round(nbytes / kmin / 1e3, 1)
            res[f"{mode}_copy_GBps"] = round(nbytes / cmin / 1e3, 1)
            res[f"{mode}_ratio_to_copy"] = round(cmin / kmin, 3)
        print(json.dumps(res), flush=True)
        out.append(res)
        del xs, ys, cs, cd


def bench_step(dev, reps, warm, rounds, out):
    codec = l3ac_amd.get_model("1kbps", synthetic_seed=0)
    codec.network.to(device=dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    x16 = torch.randn(CLIPS, 16000, device=dev, generator=g) * 0.1
    x48 = torch.randn(CLIPS, 48000, device=dev, generator=g) * 0.1

    def plain(_):
        q, _ = codec.encode_audio(x16)
        codec.decode_audio(q)

    def at48(_):
        q, _ = codec.encode_audio(x48, sample_rate=48000)
        codec.decode_audio(q, sample_rate=48000)

    t_plain, t_48 = [], []
    for _ in range(rounds):  # alternated
        t_plain.append(time_ms(plain, 1, reps, warm))
        t_48.append(time_ms(at48, 1, reps, warm))
    res = {"step": "1kbps encode+decode, 256 x 1 s", "plain_16k_ms": [round(t, 3) for t in t_plain],
           "in_out_48k_ms": [round(t, 3) for t in t_48],
           "added_ms_median": round(sorted(b - a for a, b in zip(t_plain, t_48))[len(t_plain) // 2], 3)}
    print(json.dumps(res), flush=True)
    out.append(res)


def bench_scipy(out):
    try:
        from scipy import signal
    except ImportError:
        print(json.dumps({"scipy": "not installed"}), flush=True)
        return
    import numpy as np
    x = np.random.default_rng(0).standard_normal((CLIPS, 48000)).astype(np.float32)
    for a, b, up, down in ((48000, 16000, 1, 3), (44100, 16000, 160, 441)):
        xa = x[:, :a]
        t0 = time.perf_counter()
        signal.resample_poly(xa, up, down, axis=-1)
        dt = time.perf_counter() - t0
        res = {"scipy_resample_poly": f"{a}->{b}", "clips": CLIPS, "ms": round(dt * 1e3, 1)}
        print(json.dumps(res), flush=True)
        out.append(res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="alternated rounds of the step comparison")
    ap.add_argument("--kernels-only", action="store_true", help="only the kernel / copy timings (for a rocprofv3 run)")
    ap.add_argument("--json", help="also write the results here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    dev = "cuda:0"
    results = []
    bench_pairs(dev, args.reps, args.warm, results)
    if not args.kernels_only:
        bench_step(dev, max(5, args.reps // 10), 3, args.rounds, results)
        bench_scipy(results)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(results, indent=1) + "\n")
