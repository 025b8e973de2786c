"""The host-side contract of the metric entries, pinned without a GPU: tests/golden/metric_contract.json holds what the library built from
the commit before the metric families got their shared base (csrc/kernels/metric_common.hpp, l3ac_amd/_metric.py) returned — every
``*_scratch_bytes``, ``*_frames``, ``*_blocks``, ``*_lags``, ``*_defaults`` value and table length over a grid of arguments, and for every
launch entry the return code and the message of calls with one wrong argument and with two (which error wins).  The replay requires
equality of every value and every string.  tests/golden/make_metric_contract.py wrote the file and states its layout.  The SDR family's
records were appended from the commit before every context-free entry became one definition in its family's file."""
import json
from pathlib import Path

import pytest

from l3ac_amd import _capi

C = _capi.C
FIXTURE = Path(__file__).resolve().parent / "golden" / "metric_contract.json"
CONTRACT = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {"host": {}, "launch": {}}  # (absent only while it is being recorded)
FAKE = 4096  # a non-null, 256-byte aligned "pointer": every recorded launch call is refused before anything is dereferenced or launched


def _decode(v):
    """One JSON argument as the binding takes it -> (the ctypes argument, the int32 output buffer it is or None)."""
    if isinstance(v, str):
        if v.startswith("fake"):  # "fake", "fake+4": the second is aligned to 4 bytes only
            return FAKE + int(v[4:] or 0), None
        return float(v), None  # "nan", "inf"
    if isinstance(v, list):
        return (C.c_int32 * len(v))(*v), None
    if isinstance(v, dict):
        buf = (C.c_int32 * v["out"])()
        return buf, buf
    return v, None


def run_call(lib, fn: str, args: list) -> list:
    """Calls ``fn`` -> [the return value, the library's message when that is negative else None, what int32 output buffers hold else None]."""
    assert len(args) == len(_capi.SIGNATURES[fn][1]), fn
    decoded = [_decode(v) for v in args]
    ret = int(getattr(lib, fn)(*(a for a, _ in decoded)))
    outs = [list(buf) for _, buf in decoded if buf is not None]
    return [ret, lib.l3ac_last_error().decode() if ret < 0 else None, outs if outs and ret >= 0 else None]


def mutated(base: list, changes: dict) -> list:
    args = list(base)
    for index, value in changes.items():
        args[int(index)] = value
    return args


def _message(index):
    return None if index is None else CONTRACT["messages"][index]


@pytest.mark.parametrize("fn", sorted(CONTRACT["host"]))
def test_host_values_and_messages_are_the_recorded_ones(fn):
    lib = _capi.load_library()
    records = CONTRACT["host"][fn]
    assert records
    for args, ret, msg, out in records:
        assert run_call(lib, fn, args) == [ret, _message(msg), out], (fn, args)


@pytest.mark.parametrize("fn", sorted(CONTRACT["launch"]))
def test_refused_launch_calls_fail_with_the_recorded_code_and_message(fn):
    lib = _capi.load_library()
    entry = CONTRACT["launch"][fn]
    assert len(entry["params"]) == len(entry["base"]) and entry["cases"]
    assert entry["ret"] < 0  # host-side validation refused every recorded call: nothing was launched
    for changes, msg in entry["cases"]:
        assert run_call(lib, fn, mutated(entry["base"], changes)) == [entry["ret"], _message(msg), None], (fn, changes)


def test_the_fixture_covers_every_metric_entry():
    names = [n for n in _capi.SIGNATURES
             if n.split("_")[1] in ("stft", "mel", "log", "signal", "stoi", "loudness", "apply", "pitch", "xcorr", "align", "dct", "mfcc", "dtw", "lpc",
                                    "correlate", "toeplitz", "sdr")]
    assert sorted(names) == sorted(set(CONTRACT["host"]) | set(CONTRACT["launch"]))
