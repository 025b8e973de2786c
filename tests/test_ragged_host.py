"""Host side of ragged batches: length validation and the C entries' bindings.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from l3ac_amd import _capi, ragged_lengths

HEADER = Path(__file__).resolve().parents[1] / "include" / "l3ac_hip.h"


def test_lengths_accept_sequences_arrays_and_tensors():
    assert ragged_lengths([3, 1, 10], 3, 10) == [3, 1, 10]
    assert ragged_lengths(np.array([4, 5], dtype=np.int64), 2, 5) == [4, 5]
    assert ragged_lengths(torch.tensor([7, 2], dtype=torch.int32), 2, 7) == [7, 2]
    assert ragged_lengths((2.0, 3.0), 2, 3) == [2, 3]
    assert all(type(v) is int for v in ragged_lengths(np.array([1, 2]), 2, 2))


@pytest.mark.parametrize("bad,batch,limit,what", [
    ([0, 3], 2, 5, "outside"),          # empty clip
    ([6, 3], 2, 5, "outside"),          # longer than the tensor
    ([-1, 3], 2, 5, "outside"),
    ([3], 2, 5, "1 entries for a batch of 2"),
    ([3, 3, 3], 2, 5, "3 entries"),
    ([2.5, 3], 2, 5, "integers"),
    (None, 2, 5, "sequence"),
    (["a", 3], 2, 5, "sequence"),
])
def test_bad_lengths_raise(bad, batch, limit, what):
    with pytest.raises(ValueError, match=what):
        ragged_lengths(bad, batch, limit)


def test_ragged_entries_are_declared_and_bound():
    header = HEADER.read_text()
    for name, n_args in (("l3ac_encode_ragged", 10), ("l3ac_decode_ragged", 8)):
        m = re.search(rf"int {name}\(([^;]*)\);", header)
        assert m, f"{name} missing from the header"
        assert len(m.group(1).split(",")) == n_args  # (that the binding has as many, of the header's types: tests/test_host.py)
    assert "#define L3AC_ABI_VERSION 5" in header  # additive entries: the ABI stays at 5
