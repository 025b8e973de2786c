#!/usr/bin/env python3
"""Streaming sessions: S live streams at 1kbps, a step of one second, the default look-back (the attention
window), in the steady state.  One push of every stream, encoder and decoder timed separately, three ways on the same audio:
  eager   StreamEncoder.push / StreamDecoder.push
  graph   the same steady push captured once and replayed
  cat     what a caller had to write before sessions: keep the look-back in a tensor, torch.cat it in front of the new frames, run
          encode_audio / decode_audio on the rows, slice the look-back off again and keep the rows' tail for the next step
  conv    the eager sessions with sample-rate conversion on both sides: a --in-rate (48 kHz) stream_resampler in
          front of the encoder, fed packets that convert to one step, and a --out-rate (44.1 kHz) one behind the decoder; `rs_in` /
          `rs_out` time those resampler pushes alone, `resample_in` / `resample_out` the offline l3ac_amd.resample on the same packet
`eager`, `graph` and `cat` are checked bit-equal before anything is timed, and the resampler's pushes against resample of what it was fed.  Timings: device events around --inner pushes, --reps passes
per variant after --warm, the variants alternating pass by pass; the JSON line (one per S) gives each variant's median and its
min .. max in ms PER PUSH."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import l3ac_amd


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


def summary(ms, inner):
    ms = [v / inner for v in ms]
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "passes": len(ms)}


def run(codec, streams, args):
    mc = codec.network.mc
    hop = mc.hop_length
    cl_tok = args.window // hop
    cl = cl_tok * hop
    p_tok = mc.en_coder_window_size
    p = p_tok * hop
    fill = -(-p_tok // cl_tok)  # pushes until the look-back is full
    codec.network.context().reserve(streams, p + cl)
    g = torch.Generator().manual_seed(args.seed)
    steps = [((torch.rand(streams, cl, generator=g) - 0.5)).cuda() for _ in range(fill + 3)]

    # ---- the three ways, fed the same steps; bit-equality first ------------------------------------------------------------
    enc, dec = codec.stream_encoder(streams=streams, process_window=args.window), codec.stream_decoder(streams=streams, process_window=args.window)
    g_enc, g_dec = codec.stream_encoder(streams=streams, process_window=args.window), codec.stream_decoder(streams=streams, process_window=args.window)
    cat = {"audio": torch.zeros((streams, 0), device="cuda"), "idx": torch.zeros((streams, 0), dtype=torch.int32, device="cuda")}

    def cat_encode(x):
        rows = torch.cat([cat["audio"], x], dim=1)
        q, ind = codec.encode_audio(rows)
        drop = cat["audio"].shape[1] // hop
        cat["audio"] = rows[:, -p:] if p else rows[:, :0]
        return q[:, drop:].contiguous(), ind["indices"][:, drop:].contiguous(), ind["level_indices"][:, drop:].contiguous()

    def cat_decode(idx):
        rows = torch.cat([cat["idx"], idx], dim=1)
        wave = codec.decode_audio(indices=rows)
        drop = cat["idx"].shape[1] * hop
        cat["idx"] = rows[:, -p_tok:] if p_tok else rows[:, :0]
        return wave[:, drop:].contiguous()

    tokens = []
    for j in range(fill + 1):  # fills the look-back; the last one is the eager steady push
        q, ind = enc.push(steps[j])
        wave, _ = dec.push(indices=ind["indices"])
        g_enc.push(steps[j])
        g_dec.push(indices=ind["indices"])
        qc, ic, lc = cat_encode(steps[j])
        wc = cat_decode(ic)
        assert torch.equal(q, qc) and torch.equal(ind["indices"], ic) and torch.equal(ind["level_indices"], lc), f"step {j}: cat encodes other bits"
        assert torch.equal(wave, wc), f"step {j}: cat decodes other bits"
        tokens.append(ind["indices"])
    static_audio, static_idx = steps[fill + 1].clone(), tokens[-1].clone()
    torch.cuda.synchronize()
    graph_enc, graph_dec = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_enc):
        qg, ig = g_enc.push(static_audio)
    with torch.cuda.graph(graph_dec):
        wg, _ = g_dec.push(indices=static_idx)
    for j in (fill + 1, fill + 2):
        q, ind = enc.push(steps[j])
        wave, _ = dec.push(indices=ind["indices"])
        static_audio.copy_(steps[j])
        static_idx.copy_(ind["indices"])
        graph_enc.replay()
        graph_dec.replay()
        torch.cuda.synchronize()
        assert torch.equal(qg, q) and torch.equal(ig["indices"], ind["indices"]) and torch.equal(wg, wave), f"step {j}: the graph gives other bits"
        qc, ic, lc = cat_encode(steps[j])
        assert torch.equal(q, qc) and torch.equal(cat_decode(ic), wave), f"step {j}: cat gives other bits"
    new_idx = ind["indices"]

    # ---- conversion on both sides: sessions of their own behind / in front of resamplers, brought to the steady state ---------------------
    sr = codec.config.sample_rate
    ratio_num, ratio_den = args.in_rate, sr
    n_in = cl * ratio_num // ratio_den  # a packet at the input rate that converts to one step
    x_in = (torch.rand(streams, n_in, generator=g) - 0.5).cuda()
    rs_in, rs_out = l3ac_amd.stream_resampler(streams, args.in_rate, sr), l3ac_amd.stream_resampler(streams, sr, args.out_rate)
    rs_in_alone, rs_out_alone = l3ac_amd.stream_resampler(streams, args.in_rate, sr), l3ac_amd.stream_resampler(streams, sr, args.out_rate)
    c_enc, c_dec = codec.stream_encoder(streams=streams, process_window=args.window), codec.stream_decoder(streams=streams, process_window=args.window)

    def conv_encode():
        y, n = rs_in.push(x_in)
        return c_enc.push(y, lengths=n)

    def conv_decode():
        w, n_tok = c_dec.push(indices=new_idx)
        return rs_out.push(w, lengths=n_tok * hop)

    got_in, got_out = [], []
    for j in range(fill + 2):
        conv_encode()
        conv_decode()
        got_in.append(rs_in_alone.push(x_in)[0])
        got_out.append(rs_out_alone.push(wave)[0])
    for got, piece, rates in ((got_in, x_in, (args.in_rate, sr)), (got_out, wave, (sr, args.out_rate))):
        got = torch.cat(got, dim=1)
        want = l3ac_amd.resample(torch.cat([piece] * (fill + 2), dim=1), *rates)
        assert torch.equal(got, want[:, :got.shape[1]]), "the streaming resampler gives other bits than resample"

    # ---- timing: every variant stays in the steady state, so any step serves as the next push ----------------------------------
    inner = args.inner
    x = steps[-1]

    def times(fn):
        def go():
            for _ in range(inner):
                fn()
        return go

    ms = alternate({name: times(fn) for name, fn in {
        "enc_eager": lambda: enc.push(x),
        "enc_graph": graph_enc.replay,
        "enc_cat": lambda: cat_encode(x),
        "dec_eager": lambda: dec.push(indices=new_idx),
        "dec_graph": graph_dec.replay,
        "dec_cat": lambda: cat_decode(new_idx),
        "enc_conv": conv_encode,
        "dec_conv": conv_decode,
        "rs_in": lambda: rs_in_alone.push(x_in),
        "rs_out": lambda: rs_out_alone.push(wave),
        "resample_in": lambda: l3ac_amd.resample(x_in, args.in_rate, sr),
        "resample_out": lambda: l3ac_amd.resample(wave, sr, args.out_rate),
    }.items()}, args.reps, args.warm)
    out = {"config": args.config, "streams": streams, "step_samples": cl, "step_tokens": cl_tok, "lookback_tokens": p_tok,
           "row_tokens": p_tok + cl_tok, "bit_equal": True, "inner": inner, "in_rate": args.in_rate, "out_rate": args.out_rate,
           "in_packet_samples": n_in}
    for name, v in ms.items():
        out[name] = summary(v, inner)
    for side in ("enc", "dec"):
        out[f"{side}_eager_over_cat"] = round(out[f"{side}_eager"]["median_ms"] / out[f"{side}_cat"]["median_ms"], 3)
        out[f"{side}_graph_over_eager"] = round(out[f"{side}_graph"]["median_ms"] / out[f"{side}_eager"]["median_ms"], 3)
        out[f"{side}_conv_added_ms"] = round(out[f"{side}_conv"]["median_ms"] - out[f"{side}_eager"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="1kbps")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--window", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--in-rate", type=int, default=48000, help="rate of the live input of the `conv` variant")
    ap.add_argument("--out-rate", type=int, default=44100, help="rate of the audio the `conv` variant returns")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a GPU: a timing taken anywhere else says nothing")
    codec = l3ac_amd.get_model(args.config, synthetic_seed=0)
    codec.network.to(device="cuda").eval()
    for streams in args.streams:
        run(codec, streams, args)


if __name__ == "__main__":
    main()
