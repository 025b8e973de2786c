"""tests/quantiser_ref.py on the CPU alone: the inputs of tests/test_gpu_quantiser.py have the properties its assertions rest on, and
the references agree with oracle/l3ac_oracle.py."""
import numpy as np
import pytest
import torch

from oracle import l3ac_oracle as O
from tests import quantiser_ref as R


@pytest.mark.parametrize("feat", R.FEATS)
def test_ambiguous_share_is_capped_and_oracle_obeys_the_margin(feat):
    """For every (feat, D): at most 3 % of the tokens have a dimension inside its tau; and the fp32 CPU oracle — another fp32
    evaluation, entitled to the same error — keeps its latents within e_lat and its level indices within the margin's rule."""
    for d in range(1, 9):
        c = R.fsq_case(feat, d)
        ref = R.fsq_forward_ref(c["x"], c["w_in"], c["b_in"], c["levels"])
        share = ref["ambiguous"].any(1).double().mean().item()
        w = {"quantizer.project_in.weight": c["w_in"], "quantizer.project_in.bias": c["b_in"],
             "quantizer.project_out.weight": c["w_out"], "quantizer.project_out.bias": c["b_out"]}

        class MC:
            levels = c["levels"]

        q_feat, ind, lat = O.quantizer(w, MC, c["x"])
        ratio = ((lat.double() - ref["lat"]).abs() / ref["e_lat"]).max().item()
        n_diff, _ = R.check_level_indices(ind["level_indices"], ref, c["levels"])
        print(f"[host feat {feat} D {d}] ambiguous share {share:.4f}, oracle latents err/bound {ratio:.3f}, oracle level indices off {n_diff}")
        assert share <= R.AMBIGUOUS_CAP
        assert ratio <= 1.0
        basis = R.fsq_basis(c["levels"])
        assert torch.equal((ind["level_indices"].long() * basis).sum(-1).int(), ind["indices"])
        out, bound = R.project_out_ref(R.dequantise(ind["level_indices"], c["levels"]), c["w_out"], c["b_out"])
        assert ((q_feat.double() - out).abs() <= bound).all()


def test_geometry_restates_the_launch_rule():
    assert [R.fsq_geometry(f) for f in R.FEATS] == [(2, 1, 256), (2, 2, 128), (2, 4, 64), (2, 8, 32), (4, 8, 32), (4, 16, 16), (4, 32, 8)]


@pytest.mark.parametrize("d", range(1, 9))
def test_half_activations_land_on_every_half(d):
    levels = R.fsq_levels(d)
    act, ties = R.half_activations(levels)
    assert ties == [L - 1 for L in levels], "some k has no fp32 activation whose product is exactly k + 0.5"
    lm1 = torch.tensor(levels, dtype=torch.float32) - 1
    prod = act * lm1
    for j, L in enumerate(levels):
        col, p = act[:, j], prod[:, j]
        for k in range(L - 1):
            on = col[p == k + 0.5]
            assert on.numel() > 0
            # both sides of the half are present within two ulp of it
            below = torch.nextafter(on.min(), torch.tensor(-1.0))
            above = torch.nextafter(on.max(), torch.tensor(2.0))
            assert (col == below).any() and (col == above).any()
            assert (col == torch.nextafter(below, torch.tensor(-1.0))).any() and (col == torch.nextafter(above, torch.tensor(2.0))).any()
        for v in (0.0, 1.0, 2.0 ** -30):
            assert (col == v).any()
    # the oracle rounds the exact halves to even
    _, _, li = O.fsq_quantize_act(act, levels)
    tie = (prod - prod.floor()) == 0.5
    assert tie.any() and (li[tie] % 2 == 0).all()


@pytest.mark.parametrize("dim", range(1, 9))
def test_grid_data_is_exact_and_mixed(dim):
    cases = R.vq_cases(dim)
    assert set(k for k, _ in cases) == set(R.VQ_KS) and len(cases) <= 11
    assert any(k == 2049 and n >= R.VQ_WAVE_MAX_N for k, n in cases)
    assert set(n for _, n in cases) == set(R.VQ_NS_WAVE) | set(R.VQ_NS_MANY)
    for k, n in cases:
        q, cb = R.vq_grid_case(dim, k, n, seed=100 * dim + len(str(k)) + k)
        for what, ok in R.vq_exactness(q, cb).items():
            assert ok, f"dim {dim} k {k} n {n}: {what}"
        idx, across = R.vq_argmin_ref(q, cb)
        # fp64 distances are exact here too: the same argmin from another instrument
        d64 = torch.cdist(q.double(), cb.double()) ** 2 if dim > 1 else (q.double() - cb.double().T) ** 2
        assert torch.equal(d64.argmin(1).int()[~across], idx[~across])
        assert ((d64.gather(1, idx.long()[:, None])[:, 0] - d64.min(1).values).abs() < 1e-9).all()
        if n >= R.VQ_WAVE_MAX_N:
            assert k >= 31 and 0 < int(across.sum()) < n, f"dim {dim} k {k} n {n}: {int(across.sum())} of {n} across blocks"
    q, cb = R.vq_bisector_case(dim, 513, 5120, seed=dim)
    for what, ok in R.vq_exactness(q, cb).items():
        assert ok, what
    idx, across = R.vq_argmin_ref(q, cb)
    assert across.all()
    d2 = ((q[:, None, :] - cb[None, :, :]) ** 2).sum(-1)
    assert (d2.min(1).values == 1).all()
    for i in range(0, 5120, 97):  # the minimum is shared by two codes that differ
        tied = cb[d2[i] == 1]
        assert len({tuple(r.tolist()) for r in tied}) == 2


def test_block_of_follows_the_accumulator_layout():
    got = R.vq_block_of(np.arange(64)).tolist()
    assert got[:12] == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0] and got[28:36] == [1, 1, 1, 1, 2, 2, 2, 2]


def test_grid_reference_agrees_with_the_oracle_codebook():
    """On an FSQ grid whose codes are multiples of 0.5 the search is the closed form: every code is its own nearest neighbour, and a
    query beside a code returns the closed form's index."""
    levels = [5, 3, 5, 3]
    cb = O.codebook(levels)
    perm = torch.randperm(cb.shape[0], generator=torch.Generator().manual_seed(1))
    idx, across = R.vq_argmin_ref(cb[perm], cb)
    assert torch.equal(idx.long(), perm) and not across.any()
    codes = O.fsq_indices_to_codes(idx, levels)
    assert torch.equal(codes, cb[perm])


def test_out_of_domain_rule_is_torch_argmin():
    for row in (torch.full((7,), float("nan")), torch.full((7,), float("inf"))):
        assert int(torch.argmin(row)) == 0
