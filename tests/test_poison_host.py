"""tests/poison.py has teeth: three toy batched ops in torch on concatenated clips — a conv whose clip-edge padding is a multiplicative
mask (leaks 0 * NaN), the same conv with a select (does not), an op that divides by a batch-wide maximum (leaks) — and the patterns'
own properties.  No GPU."""
import pytest
import torch

from tests import poison as P

K, HALF = 7, 3
B, T = 3, 20


def _weights():
    return torch.linspace(-1.0, 1.0, K, dtype=torch.float32) + 0.25


def _conv_rows(batch, select):
    """y[b, t] = sum_j w[j] x[b, t + j - 3], zero padding at each clip's edges, computed over the CONCATENATED rows [B * T] as the
    frame-major kernels do: a tap that falls outside the clip reads the neighbour's sample and is then zeroed — by a product with a 0 / 1
    mask, or by a select."""
    b, t = batch.shape
    flat = batch.reshape(-1)
    w = _weights()
    pos = torch.arange(b * t)
    y = torch.zeros(b * t)
    for j in range(K):
        src = pos + j - HALF
        inside = (src // t == pos // t) & (src >= 0) & (src < b * t)
        v = flat[src.clamp(0, b * t - 1)]
        v = torch.where(inside, v, torch.zeros(())) if select else v * inside.to(v.dtype)
        y = y + w[j] * v
    return y.reshape(b, t)


def _normalised(batch):
    return batch / batch.abs().max()


def _batch():
    return torch.randn((B, T), generator=torch.Generator().manual_seed(11))


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_masked_conv_leaks_and_select_conv_does_not(pattern):
    x = _batch()
    assert torch.equal(_conv_rows(x, True), _conv_rows(x, False))  # the same op on finite data: only poison tells them apart
    ref = torch.nn.functional.conv1d(x[:, None], _weights()[None, None], padding=HALF)[:, 0]
    assert torch.allclose(_conv_rows(x, True), ref, atol=1e-6)
    if pattern == "P4":  # 0 * 3e38 = 0: a finite value behind a zero mask does not leak, and the taps themselves do not overflow here
        P.twin_check(lambda b: _conv_rows(b, False), x, [0, 2], pattern)
    else:
        with pytest.raises(P.Leak, match="clean row 1 beside poisoned rows"):
            P.twin_check(lambda b: _conv_rows(b, False), x, [0, 2], pattern)
    clean, bad = P.twin_check(lambda b: _conv_rows(b, True), x, [0, 2], pattern)
    assert torch.equal(clean[1], bad[1])
    if pattern != "P2":
        assert not torch.isfinite(bad[0]).all() or pattern == "P4"


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_batch_wide_max_leaks(pattern):
    with pytest.raises(P.Leak, match="clean row 1 beside poisoned rows"):
        P.twin_check(_normalised, _batch(), [0, 2], pattern)
    P.twin_check(lambda b: b / b.abs().amax(dim=1, keepdim=True), _batch(), [0, 2], pattern)  # the maximum kept inside the clip


def test_state_that_sticks_is_caught_by_the_third_run():
    seen = {"nan": False}

    def run(b):  # a "workspace" that keeps a NaN it saw in the call BEFORE: the poisoned run itself is clean beside its poisoned row
        y = b + (1.0 if seen["nan"] else 0.0)
        seen["nan"] = seen["nan"] or bool(torch.isnan(b).any())
        return y

    with pytest.raises(P.Leak, match="clean row 0 in the clean run after the poisoned one"):
        P.twin_check(run, _batch(), [1], "P1")


def test_outputs_may_be_dicts_tuples_and_lists_and_integers_compare_as_they_are():
    def run(b):
        return {"y": _conv_rows(b, True), "idx": (b.nan_to_num().abs() * 7).to(torch.int32), "n": 3}, [r * 2 for r in b]

    P.twin_check(run, _batch(), [0], "P1")
    with pytest.raises(P.Leak, match="not finite"):  # a clean row of the clean twin must be finite too
        P.twin_check(lambda b: torch.log(b), _batch(), [0], "P1")
    P.twin_check(lambda b: torch.log(b), _batch(), [0], "P1", finite=False)  # NaN == NaN by bits
    with pytest.raises(AssertionError):  # every row poisoned checks nothing
        P.twin_check(lambda b: b, _batch(), [0, 1, 2], "P1")


@pytest.mark.parametrize("shape", [(20,), (5, 8), (1, 8), (4, 3, 2)])
def test_pattern_properties(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    pats = P.patterns(x)
    assert set(pats) == set(P.PATTERNS)
    for name, p in pats.items():
        assert p.shape == x.shape and p.dtype == x.dtype, name
    assert torch.isnan(pats["P1"]).all()
    nan = torch.isnan(pats["P2"])
    assert int(nan.sum()) == 2  # exactly two positions: the first element of the first frame, the last of the last
    assert bool(nan.reshape(-1)[0]) and bool(nan.reshape(-1)[-1])
    assert torch.equal(pats["P2"][~nan], x[~nan])
    assert nan[0].any() and nan[-1].any()
    p3 = pats["P3"].reshape(-1)
    assert torch.isinf(p3).all() and (p3[0::2] > 0).all() and (p3[1::2] < 0).all()
    p4 = pats["P4"].reshape(-1)
    assert torch.isfinite(p4).all() and (p4.abs() == torch.tensor(3e38)).all()  # finite on entry ...
    assert (p4[0::2] > 0).all() and (p4[1::2] < 0).all()
    assert torch.isinf(p4 * 2).all() and torch.isinf(p4[0] - p4[1])              # ... and overflows at the first sum or product
    assert torch.equal(x, torch.randn(shape, generator=torch.Generator().manual_seed(3)))  # the clip itself is not written


def test_poison_rows_respects_a_ragged_extent():
    x = _batch()
    bad = P.poison_rows(x, [1], "P1", extent=[T, 7, T])
    assert torch.isnan(bad[1, :7]).all() and torch.equal(bad[1, 7:], x[1, 7:]) and torch.equal(bad[0], x[0]) and torch.equal(bad[2], x[2])
    clips = [x[0], x[1, :9], x[2]]
    bad = P.poison_rows(clips, [1], "P3")
    assert torch.isinf(bad[1]).all() and bad[1].shape == (9,) and torch.equal(bad[0], clips[0])
