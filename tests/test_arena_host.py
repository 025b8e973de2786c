"""tests/arena.py has teeth: small "kernels" in torch on CPU tensors, one clean and one for each defect the guarded arena is there to
report — a write one element past an output, a write into a stride gap, a result that adds 0 * x[-1] from before its input, one that
adds 0 * x[n] from after it, an output cell nobody writes, a scratch word read before it is written — and the fills' own properties.
No GPU."""
import numpy as np
import pytest
import torch

from tests import arena as A

N = 37


def _x(n=N, seed=5):
    return torch.randn((n,), generator=torch.Generator().manual_seed(seed))


def _raw(t, k):
    """What a kernel finds k elements from t's first one, whoever owns it: the storage's word there (0 where the storage ends, as a
    plain tensor has nothing around it)."""
    at = t.storage_offset() + k
    whole = t.untyped_storage().nbytes() // t.element_size()
    return torch.as_strided(t, (1,), (1,), at)[0].clone() if 0 <= at < whole else torch.zeros((), dtype=t.dtype)


def _poke(t, k, value):
    at = t.storage_offset() + k
    if 0 <= at < t.untyped_storage().nbytes() // t.element_size():
        torch.as_strided(t, (1,), (1,), at)[0] = value


def copy(x, y):
    y.copy_(x)


def log(x, y):
    y.copy_(torch.log(x))


def clean(x, y):
    y.copy_(2 * x + 1)


def writes_past_output(x, y):
    clean(x, y)
    _poke(y, y.numel(), 7.0)


def reads_before_input(x, y):
    clean(x, y)
    y[0] += 0 * _raw(x, -1)  # the halo before the first clip, "masked" by a product


def reads_after_input(x, y):
    clean(x, y)
    y[-1] += 0 * _raw(x, x.numel())  # the tile tail after the last clip


def leaves_a_cell(x, y):
    y[:-1].copy_((2 * x + 1)[:-1])


def reads_scratch_first(x, y, scratch):
    y.copy_(2 * x + 1 + 0 * scratch[3])
    scratch.copy_(x[:scratch.numel()])


def scratch_then_read(x, y, scratch):
    scratch.copy_(x[:scratch.numel()])
    y.copy_(2 * x + 1 + 0 * scratch[3])


def test_clean_function_passes_under_every_fill():
    ref = A.embedded_check(clean, [_x()], [((N,), torch.float32)], "clean")
    assert torch.equal(ref["out0"], 2 * _x() + 1)
    A.embedded_check(scratch_then_read, [_x()], [((N,), torch.float32), {"shape": (8,), "dtype": torch.float32, "scratch": True}], "scratch written first")
    A.embedded_check(clean, [{"t": _x(), "offset": 1}], [{"shape": (N,), "dtype": torch.float32, "offset": 1}], "offset 1")
    # in place: one placement is input and output
    A.embedded_check(lambda x: x.mul_(3), [{"t": _x(), "inout": True}], [], "in place")


@pytest.mark.parametrize("fill", A.FILLS)
def test_a_write_one_element_past_an_output_is_reported(fill):
    with pytest.raises(A.Touched, match=rf"output 0 \({N},\).*first changed offset {N}(\.\d+)?, last {N}\.75 elements from its start \(behind it\)"):
        A.embedded_check(writes_past_output, [_x()], [((N,), torch.float32)], "past", fills=(fill,))


@pytest.mark.parametrize("fill", A.FILLS)
def test_a_write_into_a_stride_gap_is_reported(fill):
    x = torch.randn((3, 5), generator=torch.Generator().manual_seed(6))

    def into_gap(x, y):
        y.copy_(x)
        if y.stride(0) > 5:
            _poke(y, 5, 7.0)  # row 0 has 5 elements, row 1 starts at 8

    with pytest.raises(A.Touched, match=r"output 0 \(3, 5\).*first changed offset 5(\.\d+)?, .*\(in a stride gap\)"):
        A.embedded_check(into_gap, [x], [{"shape": (3, 5), "dtype": torch.float32, "stride0": 8}], "gap", fills=(fill,))
    A.embedded_check(copy, [{"t": x, "stride0": 7}], [{"shape": (3, 5), "dtype": torch.float32, "stride0": 8}], "strided, clean",
                     fills=(fill,))


@pytest.mark.parametrize("kernel", [reads_before_input, reads_after_input], ids=["before", "after"])
@pytest.mark.parametrize("fill", A.FILLS)
def test_a_masked_read_outside_the_input_is_reported(kernel, fill):
    spec = [((N,), torch.float32)]
    if fill in ("Z", "B"):  # 0 * 0 and 0 * 3e38 are 0: only a non-finite word shows a read that a zero weight hides
        A.embedded_check(kernel, [_x()], spec, kernel.__name__, fills=(fill,))
    else:
        with pytest.raises(A.Differs, match=r"out0: 1 of 37 words differ from the plain call, the first at \((0|36),\).*not finite"):
            A.embedded_check(kernel, [_x()], spec, kernel.__name__, fills=(fill,))


@pytest.mark.parametrize("fill", A.FILLS)
def test_an_unwritten_cell_and_a_scratch_word_read_too_early_are_reported(fill):
    if fill == "Z":  # the baseline cannot tell: the plain run's outputs and scratch are zero as well
        A.embedded_check(leaves_a_cell, [_x()], [((N,), torch.float32)], "unwritten", fills=(fill,))
        return
    with pytest.raises(A.Differs, match=r"out0: 1 of 37 words differ from the plain call, the first at \(36,\)"):
        A.embedded_check(leaves_a_cell, [_x()], [((N,), torch.float32)], "unwritten", fills=(fill,))
    specs = [((N,), torch.float32), {"shape": (8,), "dtype": torch.float32, "scratch": True}]
    if fill == "B":
        A.embedded_check(reads_scratch_first, [_x()], specs, "scratch", fills=(fill,))
    else:
        with pytest.raises(A.Differs, match="out0: 37 of 37 words differ"):
            A.embedded_check(reads_scratch_first, [_x()], specs, "scratch", fills=(fill,))


def test_bits_not_values_are_compared():
    sign = {"k": 0}

    def flips_a_zero(x, y):  # -0 in every run after the first: equal as a value, not as bits
        y.copy_(x * 0 * (1.0 if sign["k"] == 0 else -1.0))
        sign["k"] += 1

    with pytest.raises(A.Differs):
        A.embedded_check(flips_a_zero, [_x().abs() + 1], [((N,), torch.float32)], "-0", fills=("Z",))
    A.embedded_check(log, [_x()], [((N,), torch.float32)], "NaN == NaN")  # log of negatives


def test_fills_reach_every_dtype_and_placements_are_where_they_should_be():
    for fill in A.FILLS:
        a = A.Arena(fill, "cpu", A.Arena.words_for([((6,), torch.float32, None), ((4,), torch.float64, None), ((5,), torch.int32, None), ((7,), torch.uint8, None)]))
        f, d, i, u = a.place((6,)), a.place((4,), torch.float64), a.place((5,), torch.int32), a.place((7,), torch.uint8)
        even, odd = A.fill_words(fill)
        assert i.tolist() == [even, odd, even, odd, even]
        assert np.array_equal(f.numpy().view(np.int32), np.array([even, odd] * 3, dtype=np.int64).astype(np.int32))
        assert np.array_equal(d.numpy().view(np.int32), np.array([even, odd] * 4, dtype=np.int64).astype(np.int32))
        assert bytes(u.numpy().tobytes()) == np.array([even, odd], dtype=np.int64).astype(np.int32).tobytes()[:7]
        for v in (f, d, i, u):
            assert v.data_ptr() % 16 == 0 and v.is_contiguous()
        if fill == "N":
            assert torch.isnan(f).all() and i[0] == 0x7FC0BEEF and (d.abs() > 1e300).all() and torch.isinf(d * d).all()
        if fill == "I":
            assert torch.isinf(f).all() and f[0] > 0 > f[1]
        if fill == "B":
            assert torch.isfinite(f).all() and torch.isinf(f * 2).all() and f[0] > 0 > f[1]
        if fill == "Z":
            assert not f.any() and not d.any() and not u.any()
        # GUARD elements lie between neighbours and before the first, whatever the type
        starts = [p.start for p in a.placements]
        assert starts[0] >= 4 * A.GUARD and starts[1] - (starts[0] + 24) >= 8 * A.GUARD and starts[3] - (starts[2] + 20) >= 4 * A.GUARD
        assert starts[3] + 7 + 4 * A.GUARD <= a.buf.numel() * 4
        a.intact("untouched")
        for v in (f, d, i, u):
            v.fill_(1)
        a.intact("own elements only")
    a = A.Arena("N", "cpu")
    v = a.place((3, 5), stride0=9, offset=1)
    assert v.data_ptr() % 16 == 4 and v.stride() == (9, 1) and torch.isnan(v).all()
    assert A.GUARD > 256 * 512


def test_prefilled_stands_in_for_the_two_allocators_and_restores_them(monkeypatch):
    from l3ac_amd import _metric
    real_empty, real_scratch = torch.empty, _metric.scratch
    with pytest.raises(RuntimeError, match="boom"):
        with A.prefilled("N", monkeypatch) as arenas:
            s = _metric.scratch("cpu", 100)  # exactly 100 bytes, the fill in them, a guard behind them
            assert s.shape == (100,) and s.dtype == torch.uint8 and s.data_ptr() % 512 == 0 and s[:4].tolist() == [0xEF, 0xBE, 0xC0, 0x7F]
            assert _metric.scratch("cpu", 100, 28).shape == (128,)
            assert _metric.mel_scratch("cpu", 10, 1, 64, 64, 16, None).shape == (10 + 2 * 10 * 68 * 4,)  # resolved at call time: the same stand-in
            assert torch.empty(3).shape == (3,) and len(arenas.arenas) == 1  # CPU allocations are torch's own
            x = arenas.view(_x())
            assert torch.equal(x, _x()) and torch.isnan(_raw(x, -1))
            arenas.intact("before")
            s.fill_(0)
            arenas.intact("the scratch's own bytes")
            _poke(s, 100, 1)
            with pytest.raises(A.Touched, match=r"scratch of 100 bytes.*first changed offset 100, last 100 .*\(behind it\)"):
                arenas.intact("one byte past the scratch")
            raise RuntimeError("boom")
    assert torch.empty is real_empty and _metric.scratch is real_scratch
