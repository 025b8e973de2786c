"""Clip isolation against non-finite neighbours: the poison patterns and the three-run twin check (tests only; no GPU import here).

A batched entry point promises that a clip's bits do not depend on its neighbours.  A finite neighbour only shows a read that carries
non-zero weight; a NaN, an Inf or a sample that overflows inside the kernel also shows a value that was read and then multiplied by a
zero mask or weight (0 * NaN), and a wave- or workgroup-wide max, vote or reduction that spans rows of two clips.

twin_check runs the same call three times — the clean batch, the batch with some rows replaced by a pattern, the clean batch again — and
asks that every other row of every output be the same bits in all three and finite.  The reference is the call itself (same shapes, same
launch forms): there is no tolerance.  The third run catches what sticks to a context: counters, tickets, stale NaN in a workspace."""
import numpy as np
import torch

PATTERNS = ("P1", "P2", "P3", "P4")
BIG = 3e38  # finite in fp32 (max 3.4028e38); 2 * BIG, BIG * BIG and BIG - (-BIG) are not


class Leak(AssertionError):
    """A row that was not poisoned changed, or is not finite."""


def _alternating(x_clip, value):
    flat = torch.full((x_clip.numel(),), value, dtype=x_clip.dtype)
    flat[1::2] = -value
    return flat.reshape(x_clip.shape).to(x_clip.device)


def patterns(x_clip):
    """The poisoned versions of one clip (any layout whose axis 0 is the clip's frames or samples), by name:
    P1 every element NaN; P2 the clip as it is but for one NaN in its first frame / sample and one in its last (the two positions nearest
    the clip's edges: the only way out is a halo or a shared tile); P3 alternating +inf / -inf; P4 alternating +-3e38 (finite on entry,
    overflows inside the kernels)."""
    assert x_clip.is_floating_point() and x_clip.numel() > 0
    flat = x_clip.reshape(-1).clone()
    flat[0] = float("nan")
    flat[-1] = float("nan")
    p2 = flat.reshape(x_clip.shape)
    return {"P1": torch.full_like(x_clip, float("nan")), "P2": p2, "P3": _alternating(x_clip, float("inf")),
            "P4": _alternating(x_clip, BIG)}


def poison_rows(batch, rows, pattern, extent=None):
    """A copy of `batch` (a tensor [B, ...], or a list of per-clip tensors) whose `rows` hold `pattern`; extent[i]: only the clip's
    first extent[i] positions of axis 0 are the clip (a padded ragged batch: the padding stays as it is)."""
    out = [c.clone() for c in batch] if isinstance(batch, (list, tuple)) else batch.clone()
    for r in rows:
        n = out[r].shape[0] if extent is None else int(extent[r])
        if n > 0:
            out[r][:n] = patterns(out[r][:n])[pattern]
    return out


def _as_outputs(result):
    """Flatten a call's result into [(name, output)]: a tensor [B, ...], a LIST of per-clip tensors (ragged results), or a dict / tuple
    of those, nested at will."""
    if isinstance(result, torch.Tensor) or (isinstance(result, list) and result and all(isinstance(t, torch.Tensor) for t in result)):
        return [("out", result)]
    if isinstance(result, dict):
        items = [(str(k), v) for k, v in result.items()]
    elif isinstance(result, (list, tuple)):
        items = [(str(i), v) for i, v in enumerate(result)]
    else:
        return []  # counts, None, ...: compared by the caller where they matter
    out = []
    for k, v in items:
        if isinstance(v, torch.Tensor) or (isinstance(v, list) and v and all(isinstance(t, torch.Tensor) for t in v)):
            out.append((k, v))
        elif isinstance(v, (int, float, bool)) or v is None:
            continue
        else:
            out += [(f"{k}.{n}", t) for n, t in _as_outputs(v)]
    return out


def _bits(t):
    """One row of an output as integers: floats by their bit pattern (so NaN == NaN and -0 != +0), the rest as they are."""
    a = t.detach().cpu().contiguous().numpy()
    if a.dtype.kind == "f":
        return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    if a.dtype.kind == "c":
        return a.view({8: np.int32, 16: np.int64}[a.dtype.itemsize])
    return a


def _finite(t):
    return bool(torch.isfinite(t).all()) if (t.is_floating_point() or t.is_complex()) else True


def twin_check(run, batch, poisoned_rows, pattern, extent=None, finite=True, what="", bad=None):
    """run(batch) -> output tensor(s) whose axis 0 (or list position) is the clip.  Runs the clean twin, the poisoned batch and the clean
    twin again; raises Leak unless every row outside `poisoned_rows` is bit for bit the same in all three and finite (finite=False: a
    result that is legitimately NaN or +-inf for a clean clip, e.g. a measure with no valid frame, is only compared).  `bad`: the
    poisoned batch where it is not `batch` with whole rows replaced (one packet of a stream, one side of a pair, what an encoder made of
    a poisoned clip); `pattern` then only names it.  Returns (clean outputs, poisoned outputs) as run returned them, for the checks a
    case adds about the poisoned rows themselves."""
    poisoned_rows = sorted(set(int(r) for r in poisoned_rows))
    n_rows = len(batch)
    assert poisoned_rows and all(0 <= r < n_rows for r in poisoned_rows) and len(poisoned_rows) < n_rows
    if bad is None:
        bad = poison_rows(batch, poisoned_rows, pattern, extent)
        host = [v.detach().cpu() if isinstance(v, torch.Tensor) else v for v in (batch, bad)]
        for r in range(n_rows):  # the poison is where it was meant to be, and nowhere else
            assert np.array_equal(_bits(host[0][r]), _bits(host[1][r])) == (r not in poisoned_rows), f"{what}: row {r} of the poisoned batch"
    assert len(bad) == n_rows
    res = [run(batch), run(bad), run(batch)]
    outs = [_as_outputs(r) for r in res]
    assert outs[0], "twin_check: run() returned no tensor"
    assert [n for n, _ in outs[0]] == [n for n, _ in outs[1]] == [n for n, _ in outs[2]], "twin_check: the runs' outputs differ in kind"
    for k, (name, first) in enumerate(outs[0]):
        runs = [first, outs[1][k][1], outs[2][k][1]]
        runs = [r.detach().cpu() if isinstance(r, torch.Tensor) else r for r in runs]  # one copy per output, not one per row
        assert all(len(r) == n_rows for r in runs), f"{what} {name}: axis 0 is not the clip ({[len(r) for r in runs]} vs {n_rows} clips)"
        for row in range(n_rows):
            if row in poisoned_rows:
                continue
            a = runs[0][row]
            if finite and not _finite(a):
                raise Leak(f"{what} {pattern} {name}: clean row {row} of the clean twin is not finite")
            for which, other in (("beside poisoned rows " + str(poisoned_rows), runs[1][row]), ("in the clean run after the poisoned one", runs[2][row])):
                if other.shape != a.shape or other.dtype != a.dtype:
                    raise Leak(f"{what} {pattern} {name}: clean row {row} {which} has another shape or type")
                ba, bo = _bits(a), _bits(other)
                if not np.array_equal(ba, bo):
                    n_diff = int((ba != bo).sum())
                    nonfinite = not _finite(other)
                    raise Leak(f"{what} {pattern} {name}: clean row {row} {which} differs from the clean twin in {n_diff} of {ba.size} "
                               f"words{' and is not finite' if nonfinite else ''}")
    return res[0], res[1]
