"""The quantiser kernels (kernels/fsq.hip) on the MI355X at every feature width, depth and exact tie, against the plain references of
tests/quantiser_ref.py (needs an MI355X: `pytest -m gpu`).

1. FSQ forward, feat = 8 .. 512 x D = 1 .. 8 (levels [9, 7, 5, 3, 2, 4, 6, 8][:D]), both kernels (fsq_kernel whenever the latents are
   tapped, fsq_forward128_kernel at feat = 128 otherwise), against fp64 with a DERIVED margin.  With u = 2^-24 and gamma_n = n u / (1 - n u):
   a latent is an fmaf chain over the lane's channels, at most six lane-sum additions and the bias — at most feat + 8 roundings in
   whatever order — so it lies within e_lat = gamma_{feat+8} (|x| . |W_in|^T + |b_in|) of the fp64 value.  What is rounded is
   s = (tanh(lat) + 1) / 2 (L - 1); tanh' <= 1 and the halving pass on 0.5 e_lat, tanhf is documented at 2 ulp (2^-22 below 1), the
   "+ 1" and "x 0.5" round once each (4 u covers both), the last product once at a value below L - 1:
       tau = (L - 1) (0.5 e_lat + 2^-22 + 4 u) + u (L - 1).
   A level index may differ from round_half_even(s) only where s is within tau of a half, and then by one step; everywhere else it
   must be equal.  The share of tokens with a dimension inside its tau is a property of the inputs (capped at 3 %, asserted here and
   in tests/test_quantiser_host.py).  Everything after the rounding is exact up to the output projection, which must lie within
   gamma_{D+1} (|b_out| + |q| . |W_out|^T) of the fp64 projection of the kernel's own dequantised levels.  No exclusions between the
   entries: the tapped latents fed back through latents_in, and fsq_decode of the indices, return the forward call's bits; the two
   kernels return each other's.  Token counts 1, tpb - 1, tpb, tpb + 1 (tpb = tokens per block) and one count at which a block walks
   three token groups, the last one partial, for D = 6 and D = 3.
2. The rounding half bit for bit: activations whose product with L - 1 is exactly k + 0.5 for every k, their +-1 / +-2 ulp
   neighbours, 0, 1 and 2^-30, for D = 1 .. 8 at feat = 8 and 256 against O.fsq_quantize_act (IEEE multiply and torch.round: exact).
3. The explicit-codebook search on integer-grid data, where every difference, square, running sum, code norm and matrix-core score is
   exact in fp32: the defined result is np.argmin of an int64 distance, lowest index first, whichever form runs.  dim = 1 .. 8, every
   k of {1, 31, 32, 33, 63, 65, 511, 513, 1025, 2049} and every n of {1, 3, 4, 5, 255, 5119 | 5120, 5121, 6200} once per dim, every
   form the n admits; past 5 120 the number of queries the screened form lists for the full search must be the number whose minimum
   is shared by more than one of its 16-code blocks (tol = 2^-17 Qd ~ 0.02 is below the smallest non-zero gap 0.25); one case per dim
   has every query on a bisector of two different codes (all of them listed).
4. A query with no code below +inf (NaN or Inf coordinate, |q| ~ 1e30) gets index 0, in the three forms, its neighbours unchanged.

Observed on the MI355X (each test prints its figures); no test failed on the kernels as they were, except 4:
* worst latents err/bound per feat, D = 1 .. 8 at 4096 tokens: 8: 0.221, 16: 0.110, 32: 0.052, 64: 0.021, 128: 0.009, 256: 0.003,
  512: 0.001 (a worst-case bound that grows like feat against an error that grows like sqrt(feat)); three-group counts the same
  (0.239 at feat 8).  q_feature err/bound 0.35 .. 0.64.
* ambiguous share of the tokens, maximum over D: 8: 0.0002, 16: 0.0002, 32: 0.0005, 64: 0.0012, 128: 0.0027, 256: 0.0063,
  512: 0.0210 (D = 8); in the three-group cases 0.0001 .. 0.0132.  Level indices that differ from round_half_even(s): none in the 56
  cases of 4096 tokens, one each at feat 8 D 3 (of 1 048 705 tokens) and feat 16 D 6 (of 524 353), both inside tau.
* three-group token counts on 256 CUs: 1 048 705 (feat 8), 524 353, 262 177, 131 089 (feat 64 and 128), 65 545, 32 773 (feat 512).
* listed counts of the screened form on mixed grid data = the number of queries whose minimum is shared across blocks, every case:
  dim 1: 2993 / 5120 (k 511) .. 3644 / 6200 (k 1025); dim 2: 1510 (k 65) .. 4339 / 6200 (k 513); dim 3: 620 .. 2140; dim 4: 463 ..
  954; dim 5: 776 .. 968; dim 6: 646 .. 967; dim 7: 844 .. 1430; dim 8: 754 .. 852; bisector cases: 5120 of 5120 for every dim.
* 4, on the kernels as they were: the wavefront-form call returned 2147483647 for the NaN, the Inf and the 1e30 query (the search
  kernels' "none yet" marker, which vq_argmin_combine_kernel passed on); with the rule in that kernel: 0, neighbours unchanged.
* one-line changes tried on a scratch build, each alone: level indices exchanged from lane group_base + d + 1 in fsq_kernel's shuffle
  path -> 10 tests of this file fail (every width but the DPP ones, 64 and 128); the lower-index term dropped from vq_wave_kernel's
  butterfly -> all 8 grid tests fail; vq_resolve_kernel's tol at 2^-9 Qd -> 7 grid tests fail on the listed count (863 for 828).
* wall time: 8 s for the file's 25 tests; the slowest is test_fsq_forward_token_counts[8] at 1.1 s (1 048 705 tokens drawn and
  checked in fp64 on the CPU), every grid test about a second at the most (the int64 reference of its eleven cases).
"""
import pytest
import torch

from oracle import l3ac_oracle as O
from tests import gpu_ops as G
from tests import quantiser_ref as R

pytestmark = pytest.mark.gpu


def _forward_checks(tag, c, ref=None, check_cap=True):
    """One forward case through both kernels and the other entries; returns (worst latent err/bound, ambiguous share, entries off)."""
    levels, d, n = c["levels"], c["d"], c["n"]
    dev = {k: c[k].cuda() for k in ("w_in", "b_in", "w_out", "b_out")}
    x = c["x"].cuda()
    q, idx, li, lat = G.fsq_forward(x, levels, dev["w_in"], dev["b_in"], dev["w_out"], dev["b_out"], want_latents=True)
    q2, idx2, li2, _ = G.fsq_forward(x, levels, dev["w_in"], dev["b_in"], dev["w_out"], dev["b_out"])  # feat = 128: the hot kernel
    assert torch.equal(idx2, idx) and torch.equal(li2, li) and torch.equal(q2, q), f"{tag}: with and without the latents tap differ"
    q3, idx3, li3, _ = G.fsq_forward(None, levels, None, None, dev["w_out"], dev["b_out"], latents_in=lat)
    assert torch.equal(idx3, idx) and torch.equal(li3, li) and torch.equal(q3, q), f"{tag}: latents_in of the tapped latents differs"
    assert torch.equal(G.fsq_decode(idx, levels, dev["w_out"], dev["b_out"]), q), f"{tag}: fsq_decode(indices) != q_feature"
    ref = R.fsq_forward_ref(c["x"], c["w_in"], c["b_in"], levels) if ref is None else ref
    lat, li, idx, q = lat.cpu(), li.cpu(), idx.cpu(), q.cpu()
    ratio = ((lat.double() - ref["lat"]).abs() / ref["e_lat"]).max().item()
    assert ratio <= 1.0, f"{tag}: latents outside e_lat (worst err/bound {ratio:.3f})"
    n_off, share = R.check_level_indices(li, ref, levels)
    assert torch.equal((li.long() * R.fsq_basis(levels)).sum(-1).int(), idx), f"{tag}: indices != sum li_d basis_d"
    out, bound = R.project_out_ref(R.dequantise(li, levels), c["w_out"], c["b_out"])
    qr = ((q.double() - out).abs() / bound).max().item()
    assert torch.isfinite(q).all() and qr <= 1.0, f"{tag}: q_feature outside its bound (worst err/bound {qr:.3f})"
    if check_cap:
        assert share <= R.AMBIGUOUS_CAP, f"{tag}: ambiguous share {share:.4f}"
    print(f"[{tag}] n {n}: latents err/bound {ratio:.3f}, q_feature err/bound {qr:.3f}, ambiguous share {share:.4f}, level indices off {n_off}")
    return ratio, share, n_off


@pytest.mark.parametrize("feat", R.FEATS)
def test_fsq_forward_every_depth(feat):
    worst, shares, off = 0.0, [], 0
    for d in range(1, 9):
        ratio, share, n_off = _forward_checks(f"fsq feat {feat} D {d}", R.fsq_case(feat, d))
        worst, off = max(worst, ratio), off + n_off
        shares.append(share)
    print(f"[fsq feat {feat}] worst latents err/bound {worst:.3f}; ambiguous share max {max(shares):.4f}; level indices off (all inside tau) {off}")


@pytest.mark.parametrize("feat", R.FEATS)
def test_fsq_forward_token_counts(feat):
    """Block edges, and a block that walks three token groups with the last one partial (8 = the residency cap of fsq_resident, so at
    least one block of the resident grid takes a third group whatever the kernel's occupancy)."""
    tpb = R.fsq_geometry(feat)[2]
    places = torch.cuda.get_device_properties(0).multi_processor_count * 8
    multi = 2 * places * tpb + tpb // 2 + 1
    assert multi * feat * 4 <= 72e6
    for d in (6, 3):
        for n in (1, tpb - 1, tpb, tpb + 1):
            _forward_checks(f"fsq feat {feat} D {d}", R.fsq_case(feat, d, n), check_cap=False)  # (a share of 1 .. 257 tokens says nothing)
        _forward_checks(f"fsq feat {feat} D {d} three groups", R.fsq_case(feat, d, multi))


@pytest.mark.parametrize("feat", (8, 256))
def test_fsq_rounding_halves_bit_for_bit(feat):
    for d in range(1, 9):
        levels = R.fsq_levels(d)
        act, ties = R.half_activations(levels)
        assert ties == [L - 1 for L in levels]
        g = torch.Generator().manual_seed(7000 + 10 * feat + d)
        w_out = torch.rand(feat, d, generator=g) - 0.5
        b_out = torch.rand(feat, generator=g) - 0.5
        q_ref, idx_ref, li_ref = O.fsq_quantize_act(act, levels)
        q, idx, li = G.fsq_quantize_act(act.cuda(), levels, w_out.cuda(), b_out.cuda())
        assert torch.equal(li.cpu(), li_ref), f"feat {feat} D {d}: {(li.cpu() != li_ref).sum().item()} level indices differ at the halves"
        assert torch.equal(idx.cpu(), idx_ref)
        out, bound = R.project_out_ref(q_ref, w_out, b_out)
        assert ((q.cpu().double() - out).abs() <= bound).all()
        prod = act * (torch.tensor(levels, dtype=torch.float32) - 1)
        print(f"[fsq halves feat {feat} D {d}] {act.shape[0]} rows, {int(((prod - prod.floor()) == 0.5).sum())} exact halves")


def _search_all_forms(tag, q, cb, ref):
    """Every form the query count admits against the defined result; returns the screened form's listed count (None below 5 120)."""
    n = q.shape[0]
    qd, cbd = q.cuda(), cb.cuda()
    info = {}
    got = G.vq_argmin(qd, cbd, info=info).cpu()
    assert torch.equal(got, ref), f"{tag}: {(got != ref).sum().item()} of {n} differ from the int64 argmin (form 0)"
    if n >= R.VQ_WAVE_MAX_N:
        scan = G.vq_argmin(qd, cbd, form=1).cpu()
        assert torch.equal(scan, ref), f"{tag}: {(scan != ref).sum().item()} of {n} differ from the int64 argmin (scan)"
        wave = torch.cat([G.vq_argmin(qd[i:i + 4000], cbd).cpu() for i in range(0, n, 4000)])
        assert torch.equal(wave, ref), f"{tag}: {(wave != ref).sum().item()} of {n} differ from the int64 argmin (wavefront)"
    return info["listed"]


@pytest.mark.parametrize("dim", range(1, 9))
def test_vq_argmin_exact_on_the_integer_grid(dim):
    for k, n in R.vq_cases(dim):
        q, cb = R.vq_grid_case(dim, k, n, seed=100 * dim + len(str(k)) + k)
        ref, across = R.vq_argmin_ref(q, cb)
        listed = _search_all_forms(f"vq dim {dim} k {k} n {n}", q, cb, ref)
        print(f"[vq grid dim {dim} k {k} n {n}] listed {listed}, minimum shared across blocks {int(across.sum())}")
        if n >= R.VQ_WAVE_MAX_N:
            assert 0 < listed < n
            assert listed == int(across.sum()), "the screened form lists exactly the queries whose minimum is shared by two of its blocks"
    q, cb = R.vq_bisector_case(dim, 513, 5120, seed=dim)
    ref, across = R.vq_argmin_ref(q, cb)
    listed = _search_all_forms(f"vq dim {dim} bisectors", q, cb, ref)
    print(f"[vq bisectors dim {dim}] listed {listed} of 5120")
    assert across.all() and listed == 5120


def test_vq_argmin_out_of_domain_queries_get_index_zero():
    """include/l3ac_hip.h: no code below +inf -> index 0 (torch.argmin on an all-NaN / all-inf row), in the wavefront form, the
    screened form and the scan; every other query keeps the bits it has without such neighbours, which are the fp64 argmin's."""
    cb = O.codebook([7] * 3)
    assert cb.shape[0] == 343
    for n, forms in ((8, (0,)), (5200, (0, 1))):
        g = torch.Generator().manual_seed(n)
        clean = torch.tanh(torch.randn(n, 3, generator=g) * 1.2)
        bad = [1, 3, 5] if n == 8 else [0, 31, 32, 2047, 4096, n - 1]
        q = clean.clone()
        for j, i in enumerate(bad):
            if j % 3 == 0:
                q[i, 1] = float("nan")
            elif j % 3 == 1:
                q[i, 0] = float("inf")
            else:
                q[i] = 1e30
        d = torch.cdist(clean.double(), cb.double())
        best2 = d.topk(2, dim=1, largest=False).values
        clear = best2[:, 1] - best2[:, 0] > 1e-5  # clear winners: fp32 and fp64 agree on them
        clear[bad] = True
        assert clear.double().mean() > 0.99
        ref = d.argmin(1).int()
        ref[bad] = 0
        keep = torch.ones(n, dtype=torch.bool)
        keep[bad] = False
        for form in forms:
            got = G.vq_argmin(q.cuda(), cb.cuda(), form=form).cpu()
            base = G.vq_argmin(clean.cuda(), cb.cuda(), form=form).cpu()
            print(f"[vq out of domain n {n} form {form}] indices of the NaN / Inf / 1e30 queries: {got[bad].tolist()}")
            assert got[bad].tolist() == [0] * len(bad), f"n {n} form {form}: out-of-domain queries returned {got[bad].tolist()}"
            assert torch.equal(got[clear], ref[clear]), f"n {n} form {form}"
            assert torch.equal(got[keep], base[keep]), f"n {n} form {form}: a neighbour of an out-of-domain query changed"
