#!/usr/bin/env python3
"""Record ``metric_contract.json``: what the metric entries of a built library return on the host, for tests/test_metric_contract_host.py.

Run it ONCE against a library built from the commit whose behaviour is to be pinned (``L3AC_LIB_PATH=<that build's libl3ac_hip.so>
python tests/golden/make_metric_contract.py``); no GPU is needed.  It records
  * ``host``    every ``*_scratch_bytes``, ``*_frames``, ``*_blocks``, ``*_lags``, ``*_defaults`` value and the length of every host table over
                a grid of arguments: batch 1, 2, 65535 and the first values outside; samples 1, just below / at / above one frame, a few
                thousand and the ends of the range; every family's parameter extremes.  A refused call records its message.
  * ``launch``  for each launch entry a valid call on fake pointers (never made as it stands) and calls with one of its arguments wrong, then
                with two: the return code and the message, i.e. which check comes first.  Every one must be refused by the host-side
                validation — the script fails on a call that is not.
A family added later is recorded after the earlier ones (the SDR family, from the commit before its entries moved out of capi.hip into
kernels/sdr.hip): the earlier records must come out as they are in the file, the new records and messages behind them.
"""
import itertools
import json
import sys
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from l3ac_amd import _capi  # noqa: E402
from tests.test_metric_contract_host import FIXTURE, mutated, run_call  # noqa: E402

BATCH = ([1, 2, 65535], [0, 65536])
TOP = 1 << 31
BIG = 1 << 40  # scratch_bytes of the base calls: above every minimum


def sweep(*axes):
    """Argument lists over axes of (supported values, unsupported values); an axis may hold tuples, which are spliced in.  Every
    combination of supported values, then each unsupported value on its own beside the first supported value of the other axes."""
    flat = lambda combo: [v for part in combo for v in (part if isinstance(part, (list, tuple)) else [part])]  # noqa: E731
    calls = [flat(c) for c in itertools.product(*(good for good, _ in axes))]
    for i, (_, bad) in enumerate(axes):
        calls += [flat([b if j == i else good[0] for j, (good, _) in enumerate(axes)]) for b in bad]
    return calls


def host_calls() -> dict:
    mel = ([(64, 16, 8), (16, 4, 1), (2048, 2048, 256), (2048, 4, 80)], [(24, 4, 8), (64, 6, 8), (64, 16, 257)])
    pitch = ([(16000, 60.0, 500.0, -1, -1), (8000, 60.0, 500.0, -1, -1), (192000, 200.0, 1000.0, -1, -1), (16000, 60.0, 500.0, 1, 1),
              (16000, 8.0, 4000.0, 1, 7), (16000, 60.0, 500.0, 3000, 4000)],
             [(16000, 60.0, 500.0, 0, -1), (16000, 60.0, 500.0, -1, 0), (7999, 60.0, 500.0, -1, -1), (16000, 500.0, 60.0, -1, -1),
              (16000, 60.0, 4001.0, -1, -1), (16000, 1.0, 500.0, -1, -1), (16000, 60.0, 500.0, 3733, -1), (16000, 3999.0, 4000.0, -1, -1),
              (16000, 60.0, "inf", -1, -1)])
    lpc = ([(16000, 16, 480, 120), (8000, 10, 240, 60), (16000, 1, 2, 1), (192000, 32, 8192, 8192), (16000, 32, 33, 9000)],
           [(16000, 16, 480, 0), (16000, 16, 16, 4), (16000, 33, 480, 120), (16000, 0, 480, 120), (16000, 16, 8193, 120), (7999, 16, 480, 120),
            (192001, 16, 480, 120)])
    table = [(None, 0)], []  # the size query of a host table
    return {
        "l3ac_stft_frames": sweep(([1, 3, 4, 5, 5000, 1 << 40], [0, -1]), ([4, 1, 512], [0, -4])),
        "l3ac_stft_basis": sweep(([16, 64, 512, 2048], [8, 24, 2064, 0, -64]), table),
        "l3ac_mel_weights": sweep(([(16000, 64, 8), (16000, 2048, 256), (44100, 1024, 128), (1, 16, 1)],
                                   [(0, 64, 8), (16000, 24, 8), (16000, 64, 0), (16000, 64, 257)]), table),
        "l3ac_mel_scratch_bytes": sweep(BATCH, ([1, 63, 64, 65, 5000, TOP - 4097], [0, TOP - 4096]), mel) + [[65535, TOP - 4097, 16, 4, 1]],
        "l3ac_stoi_frames": sweep(([1, 255, 256, 257, 384, 385, 5000], [0, -5])),
        "l3ac_stoi_basis": sweep(table),
        "l3ac_stoi_window": sweep(table),
        "l3ac_stoi_bands": [[{"out": 30}], [None]],
        "l3ac_stoi_scratch_bytes": sweep(BATCH, ([1, 256, 257, 385, 4097, 5000, TOP - 4097], [0, TOP - 4096])),
        "l3ac_loudness_coeffs": sweep(([8000, 16000, 44100, 48000, 192000], [7990, 16001, 192010, 0]), table),
        "l3ac_loudness_blocks": sweep(([1, 4799, 4800, 19199, 19200, 19201, 500000], [0, -1]), ([8000, 48000, 192000], [16001])),
        "l3ac_loudness_scratch_bytes": sweep(BATCH, ([1, 799, 800, 3199, 3200, 3201, 5000, TOP - 1], [0, TOP]), ([8000, 48000, 192000], [7990])),
        "l3ac_pitch_lags": sweep(pitch, ([{"out": 5}], [None])),
        "l3ac_pitch_frames": sweep(([0, 1, 534, 535, 536, 5000], [-1]), pitch),  # span of the default geometry at 16 kHz: 267 + 268
        "l3ac_pitch_scratch_bytes": sweep(BATCH, ([1, 535, 5000, TOP - 1], [0, TOP]), pitch),
        "l3ac_xcorr_scratch_bytes": sweep(BATCH, ([1, 4095, 4096, 4097, 5000, TOP - 1], [0, TOP]), ([0, 1, 100, 16384], [-1, 16385])),
        "l3ac_dct_table": sweep(([(40, 13), (2, 1), (256, 64), (65, 64)], [(64, 64), (1, 1), (40, 40), (257, 13), (40, 0), (0, 1)]), table),
        "l3ac_mfcc_scratch_bytes": sweep(BATCH, ([1, 159, 160, 161, 5000], [0, TOP - 4096]),
                                         ([(512, 160, 40), (16, 4, 2), (2048, 2048, 256)], [(24, 4, 8)]), ([13, 1], [0, 64])),
        "l3ac_dtw_scratch_bytes": sweep(BATCH, ([1, 2, 4096], [0, 4097]), ([1, 3, 4096], [0, 4097])),
        "l3ac_lpc_window": sweep(([2, 3, 480, 8192], [1, 8193, 0]), table),
        "l3ac_lpc_defaults": sweep(([8000, 9999, 10000, 16000, 44100, 192000], [7999, 192001]), ([{"out": 3}], [None])),
        "l3ac_lpc_frames": sweep(([0, 1, 479, 480, 481, 5000, TOP], [-1]), ([480, 2, 8192], [1, 8193]), ([120, 1, 9000], [0])),
        "l3ac_lpc_scratch_bytes": sweep(BATCH, ([1, 479, 480, 481, 5000, TOP - 1], [0, TOP]), lpc),
        "l3ac_lpc_metrics_scratch_bytes": sweep(BATCH, ([1, 479, 480, 481, 5000, 16385, 16386], [0, TOP, 2000000, TOP - 1]), lpc),
    }


# ---- the launch entries: (parameter names, a call that would be valid on real buffers, wrong values by parameter) ------------------------------
F, F4 = "fake", "fake+4"
SCRATCH = [("scratch", None), ("scratch", F4), ("scratch_bytes", 0), ("scratch_bytes", 255)]
LENS = [("samples", [0, 100]), ("samples", [50, 101]), ("samples", [50, -3])]


def shape(batch="batch", samples="max_samples"):
    return [(batch, 0), (batch, 65536), (batch, -1), (samples, 0), (samples, TOP), (samples, TOP - 4096)]


LAUNCH = {
    "l3ac_stft": (
        "audio batch max_samples audio_stride samples n_fft hop basis spec scratch scratch_bytes stream",
        [F, 2, 100, 100, [50, 100], 64, 16, F, F, F, BIG, None],
        shape() + LENS + SCRATCH + [("audio", None), ("audio_stride", 99), ("n_fft", 24), ("n_fft", 4096), ("hop", 6), ("hop", 128), ("basis", None),
                                    ("basis", F4), ("spec", None)]),
    "l3ac_log_mel": (
        "audio batch max_samples audio_stride samples n_fft hop basis weights n_mels out scratch scratch_bytes stream",
        [F, 2, 100, 100, [50, 100], 64, 16, F, F, 8, F, F, BIG, None],
        shape() + LENS + SCRATCH + [("audio", None), ("audio_stride", 99), ("n_fft", 24), ("hop", 6), ("basis", None), ("basis", F4), ("weights", None),
                                    ("n_mels", 0), ("n_mels", 257), ("out", None)]),
    "l3ac_mel_distance": (
        "ref ref_stride est est_stride batch max_samples samples n_fft hop n_mels basis weights out scratch scratch_bytes stream",
        [F, 100, F, 100, 2, 100, [50, 100], 64, 16, 8, F, F, F, F, BIG, None],
        shape() + LENS + SCRATCH + [("ref", None), ("est", None), ("ref_stride", 99), ("est_stride", 99), ("n_fft", 24), ("hop", 6), ("n_mels", 257),
                                    ("basis", None), ("basis", F4), ("weights", None), ("out", None)]),
    "l3ac_signal_metrics": (
        "ref ref_stride est est_stride batch max_samples samples out scratch scratch_bytes stream",
        [F, 100, F, 100, 2, 100, [50, 100], F, F, BIG, None],
        # (this entry takes any positive batch: 65536 would walk past the two lengths)
        [("batch", 0), ("batch", -1), ("max_samples", 0), ("max_samples", TOP)] + LENS
        + [("ref", None), ("est", None), ("out", None), ("ref_stride", 99), ("est_stride", 99), ("scratch", None), ("scratch", "fake+2"),
           ("scratch_bytes", 7)]),
    "l3ac_stoi": (
        "ref ref_stride est est_stride batch max_samples samples basis out frames_out bands_out scratch scratch_bytes stream",
        [F, 5000, F, 5000, 2, 5000, [4000, 5000], F, F, F, None, F, BIG, None],
        shape() + [("samples", [0, 5000]), ("samples", [4000, 5001])] + SCRATCH
        + [("ref", None), ("est", None), ("out", None), ("frames_out", None), ("basis", None), ("basis", F4), ("ref_stride", 4999), ("est_stride", 4999)]),
    "l3ac_loudness": (
        "audio audio_stride batch max_samples samples sample_rate stats counts momentary scratch scratch_bytes stream",
        [F, 100, 2, 100, [50, 100], 16000, F, F, None, F, BIG, None],
        shape() + LENS + SCRATCH + [("audio", None), ("stats", None), ("counts", None), ("audio_stride", 99), ("sample_rate", 16001),
                                    ("sample_rate", 7990)]),
    "l3ac_loudness_gain": (
        "stats batch target_lufs peak_limit_db gain stream",
        [F, 2, -23.0, -1.0, F, None],
        [("batch", 0), ("batch", 65536), ("target_lufs", "nan"), ("target_lufs", "inf"), ("stats", None), ("gain", None)]),
    "l3ac_apply_gain": (
        "audio audio_stride out out_stride batch max_samples samples gain gain_stride stream",
        [F, 100, F, 100, 2, 100, [50, 100], F, 1, None],
        shape()[:5] + LENS + [("audio", None), ("out", None), ("gain", None), ("audio_stride", 99), ("out_stride", 99), ("gain_stride", 0)]),
    "l3ac_pitch": (
        "audio audio_stride batch max_samples samples sample_rate fmin fmax window hop threshold f0 voiced aperiodicity cmnd frames scratch scratch_bytes "
        "stream",
        [F, 1000, 2, 1000, [600, 1000], 16000, 60.0, 500.0, -1, -1, 0.1, F, F, F, None, F, F, BIG, None],
        shape()[:5] + [("samples", [0, 1000]), ("samples", [600, 1001])] + SCRATCH
        + [("audio", None), ("f0", None), ("voiced", None), ("aperiodicity", None), ("audio_stride", 999), ("sample_rate", 7999), ("fmin", 0.0),
           ("fmax", 4001.0), ("window", 0), ("hop", 0), ("window", 3733), ("threshold", 0.0), ("threshold", 1.0), ("threshold", "nan")]),
    "l3ac_pitch_metrics": (
        "f0_ref voiced_ref f0_est voiced_est batch max_frames frames out counts stream",
        [F, F, F, F, 2, 40, [10, 40], F, F, None],
        [("batch", 0), ("batch", 65536), ("max_frames", -1), ("max_frames", TOP), ("out", None), ("counts", None), ("f0_ref", None), ("voiced_est", None),
         ("frames", [-1, 40]), ("frames", [10, 41])]),
    "l3ac_xcorr": (
        "ref ref_stride est est_stride batch max_samples samples max_lag lag polarity delay correlation xcorr scratch scratch_bytes stream",
        [F, 100, F, 100, 2, 100, [50, 100], 8, F, F, F, F, None, F, BIG, None],
        shape()[:5] + LENS + SCRATCH + [("ref", None), ("est", None), ("lag", None), ("correlation", None), ("ref_stride", 99), ("est_stride", 99),
                                        ("max_lag", -1), ("max_lag", 16385)]),
    "l3ac_align_apply": (
        "ref ref_stride est est_stride batch max_samples samples lag out_ref out_ref_stride out_est out_est_stride out_samples scratch scratch_bytes stream",
        [F, 100, F, 100, 2, 100, [50, 100], F, F, 100, F, 100, F, F, BIG, None],
        shape()[:5] + LENS + SCRATCH + [("ref", None), ("est", None), ("lag", None), ("out_ref", None), ("out_samples", None), ("ref_stride", 99),
                                        ("out_est_stride", 99)]),
    "l3ac_mfcc": (
        "audio batch max_samples audio_stride samples n_fft hop basis weights n_mels dct n_coeffs out scratch scratch_bytes stream",
        [F, 2, 100, 100, [50, 100], 64, 16, F, F, 8, F, 4, F, F, BIG, None],
        shape() + LENS + SCRATCH + [("audio", None), ("out", None), ("basis", None), ("weights", None), ("dct", None), ("audio_stride", 99), ("n_fft", 24),
                                    ("hop", 6), ("n_mels", 257), ("n_coeffs", 0), ("n_coeffs", 8)]),
    "l3ac_dtw": (
        "a a_frame_stride a_row_stride b b_frame_stride b_row_stride batch dim max_frames_a max_frames_b frames_a frames_b diagonal_only cost path_len path "
        "delta scratch scratch_bytes stream",
        [F, 12, 120, F, 12, 96, 2, 12, 10, 8, [5, 10], [8, 3], 0, F, F, None, None, F, BIG, None],
        [("batch", 0), ("batch", 65536), ("max_frames_a", 0), ("max_frames_a", 4097), ("max_frames_b", 0), ("max_frames_b", 4097), ("dim", 0), ("dim", 65),
         ("a", None), ("b", None), ("cost", None), ("path_len", None), ("a_frame_stride", 11), ("b_frame_stride", 11), ("a_row_stride", 119),
         ("b_row_stride", 95), ("a_frame_stride", -12), ("frames_a", [0, 10]), ("frames_a", [5, 11]), ("frames_b", [9, 3]), ("frames_b", [8, 0]),
         ("diagonal_only", 1)] + SCRATCH),
    "l3ac_lpc": (
        "audio audio_stride batch max_samples samples sample_rate order frame hop window a reflection error autocorr valid frames scratch scratch_bytes "
        "stream",
        [F, 1000, 2, 1000, [600, 1000], 16000, 16, 480, 120, F, F, F, F, F, F, F, F, BIG, None],
        shape()[:5] + [("samples", [0, 1000]), ("samples", [600, 1001])] + SCRATCH
        + [("audio", None), ("a", None), ("valid", None), ("audio_stride", 999), ("sample_rate", 7999), ("order", 0), ("order", 33), ("frame", 16),
           ("frame", 8193), ("hop", 0)]),
    "l3ac_lpc_metrics": (
        "ref ref_stride est est_stride batch max_samples samples sample_rate order frame hop window trim llr_max is_max cd_max out counts frame_values forms "
        "scratch scratch_bytes stream",
        [F, 1000, F, 1000, 2, 1000, [600, 1000], 16000, 16, 480, 120, F, 0.95, 2.0, 100.0, 10.0, F, F, None, None, F, BIG, None],
        shape()[:5] + [("samples", [0, 1000]), ("samples", [600, 1001])] + SCRATCH
        + [("ref", None), ("est", None), ("out", None), ("counts", None), ("ref_stride", 999), ("est_stride", 999), ("sample_rate", 192001), ("order", 33),
           ("frame", 16), ("hop", 0), ("trim", 0.0), ("trim", 1.5), ("llr_max", -1.0), ("is_max", "inf"), ("cd_max", "nan"), ("max_samples", 2000000)]),
}


# ---- the SDR family, recorded later than the rest: its records and messages are APPENDED, the earlier ones keep their place and index --------
def sdr_host_calls() -> dict:
    taps = ([8, 1, 2, 512, 1024], [0, 1025, -1])
    extent = [[1, TOP - 1, 1], [1, TOP - 1, 2], [65535, TOP - 1024, 1024], [1, TOP - 1023, 1024]]  # max_samples + taps - 1 at and past 2^31 - 1
    return {
        "l3ac_correlate_scratch_bytes": sweep(BATCH, ([1, 4096, 5000, TOP - 8], [0, TOP]), taps) + extent,
        "l3ac_toeplitz_solve_scratch_bytes": sweep(BATCH, taps),
        "l3ac_sdr_scratch_bytes": sweep(BATCH, ([1, 4088, 4089, 4090, 5000, TOP - 8], [0, TOP]), taps) + extent,  # 4089 + 8 - 1: one segment
    }


SDR_LAUNCH = {
    "l3ac_correlate": (
        "u u_stride v v_stride batch max_samples samples lags out scratch scratch_bytes stream",
        [F, 100, F, 100, 2, 100, [50, 100], 8, F, F, BIG, None],
        shape()[:5] + LENS + SCRATCH + [("u", None), ("v", None), ("out", None), ("u_stride", 99), ("v_stride", 99), ("lags", 0), ("lags", 1025),
                                        ("max_samples", TOP - 4)]),
    "l3ac_toeplitz_solve": (
        "r b batch length x error valid scratch scratch_bytes stream",
        [F, F, 2, 8, F, F, F, F, BIG, None],
        [("batch", 0), ("batch", 65536), ("batch", -1), ("length", 0), ("length", 1025), ("r", None), ("b", None), ("x", None), ("error", None),
         ("valid", None)] + SCRATCH),
    "l3ac_sdr": (
        "ref ref_stride est est_stride batch max_samples samples filter_length load out valid filter corr scratch scratch_bytes stream",
        [F, 100, F, 100, 2, 100, [50, 100], 8, 0.001, F, F, None, None, F, BIG, None],
        shape()[:5] + LENS + SCRATCH + [("ref", None), ("est", None), ("out", None), ("valid", None), ("ref_stride", 99), ("est_stride", 99),
                                        ("filter_length", 0), ("filter_length", 1025), ("load", -1.0), ("load", "inf"), ("load", "nan"),
                                        ("max_samples", TOP - 4)]),
}


def launch_cases(lib, fn: str, spec) -> dict:
    names, base, wrong = spec
    params = names.split()
    assert len(params) == len(base) == len(_capi.SIGNATURES[fn][1]), fn
    singles = [{str(params.index(p)): v} for p, v in wrong]
    firsts = list({next(iter(s)): s for s in reversed(singles)}.values())[::-1]  # pairs: the first wrong value of each parameter
    pairs = [dict(a, **b) for a, b in itertools.combinations(firsts, 2)]
    cases = []
    for changes in singles + pairs:
        ret, err, _ = run_call(lib, fn, mutated(base, changes))
        assert ret == -1, f"{fn} {changes}: not refused by the host-side validation: {ret} {err}"  # (L3AC_EINVAL; anything else launched)
        cases.append([changes, message(err)])
    return {"params": params, "base": base, "ret": -1, "cases": cases}


MESSAGES = []  # every distinct message once; the records hold its index


def message(err):
    if err is not None and err not in MESSAGES:
        MESSAGES.append(err)
    return None if err is None else MESSAGES.index(err)


def main() -> None:
    lib = _capi.load_library()
    host, launch = {}, {}
    for host_part, launch_part in ((host_calls(), LAUNCH), (sdr_host_calls(), SDR_LAUNCH)):  # in the order recorded: messages keep their index
        for fn, calls in host_part.items():
            host[fn] = []
            for args in calls:
                ret, err, out = run_call(lib, fn, args)
                host[fn].append([args, ret, message(err), out])
        launch.update({fn: launch_cases(lib, fn, spec) for fn, spec in launch_part.items()})
    # one line per entry: "messages" [text], "host" {entry: [[args, return value, message or null, output buffers or null]]},
    # "launch" {entry: {"params", "base" (the valid call), "ret", "cases": [[{index of the parameter: wrong value}, message]]}}
    text = json.dumps({"messages": MESSAGES, "host": host, "launch": launch}, separators=(",", ":"))
    FIXTURE.write_text(text.replace('"],"host":{', '"],\n"host":{\n').replace(']],"l3ac_', ']],\n"l3ac_').replace(']]},"l3ac_', ']]},\n"l3ac_')
                       .replace('},"launch":{', '},\n"launch":{\n') + "\n")
    n_host, n_launch = sum(map(len, host.values())), sum(len(e["cases"]) for e in launch.values())
    print(f"wrote {FIXTURE} ({FIXTURE.stat().st_size} bytes): {n_host} host calls, {n_launch} refused launch calls, {len(MESSAGES)} messages; "
          f"library {_capi.LIB_PATH}")


if __name__ == "__main__":
    main()
