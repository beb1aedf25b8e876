"""GPU: the matrix-free EnTr scoring -- jmac_sim_softmax_stats_f32 (softmax statistics in the similarity product's epilogue)
and scoring.alignment_stats / alignment_stats_dbpv1 on top of it -- against the reference's golden matrices, bit for bit
against the stored product (sim_matrix), against the existing softmax / entropy entry points, and against the float64 oracle
at BASELINE config 5's size.  Expected values of the closed form: tests/align_stats_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import align_stats_ref as ref
from util import assert_close, load_golden


def _unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1)


def test_alignment_stats_matches_reference_golden():
    from jmac_amd import scoring
    g = load_golden("model_small")
    e1, e2 = torch.from_numpy(g["emb1_align"]).cuda(), torch.from_numpy(g["emb2_align"]).cuda()
    l1, l2 = g["aq_list1"], g["aq_list2"]
    H, rp, ri, cp, ci = scoring.alignment_stats(e1, e2, l1.tolist(), l2.tolist())
    assert ri.dtype == torch.int64 and ci.dtype == torch.int64
    assert abs(float(H) - float(g["aq_entropy"])) <= 1e-4 * float(g["aq_entropy"])
    P, Q = torch.from_numpy(g["aq_softmax_rows"]), torch.from_numpy(g["aq_softmax_cols"])
    assert_close(rp, P.max(1)[0], 1e-4, what="row maxima")
    assert_close(cp, Q.max(1)[0], 1e-4, what="column maxima")
    assert np.array_equal(ri.cpu().numpy()[l1], ref.first_argmax(P, 1)[l1])
    assert np.array_equal(ci.cpu().numpy()[l2], ref.first_argmax(Q, 1)[l2])
    N1, N2 = P.shape
    out1, out2 = np.setdiff1d(np.arange(N1), l1), np.setdiff1d(np.arange(N2), l2)
    assert bool((ri[out1] == 0).all()) and bool((ci[out2] == 0).all())
    assert bool((rp[out1] == np.float32(1.0 / N2)).all()) and bool((cp[out2] == np.float32(1.0 / N1)).all())


def test_alignment_stats_dbpv1_matches_reference_golden():
    from jmac_amd import scoring
    g = load_golden("scoring_dbpv1")
    emb = torch.from_numpy(g["emb"]).cuda()
    H, rp, ri, cp, ci = scoring.alignment_stats_dbpv1(emb, g["list1"].tolist(), g["list2"].tolist())
    assert abs(float(H) - float(g["entropy"])) <= 1e-4 * float(g["entropy"])
    P, Q = torch.from_numpy(g["softmax_simi"]), torch.from_numpy(g["softmax_simi2"])
    assert_close(rp, P.max(1)[0], 1e-4, what="row maxima")
    assert_close(cp, Q.max(1)[0], 1e-4, what="column maxima")
    assert np.array_equal(ri.cpu().numpy(), ref.first_argmax(P, 1)) and np.array_equal(ci.cpu().numpy(), ref.first_argmax(Q, 1))


def test_alignment_stats_repeats_and_antipodal_lines():
    """Lists with repeated entries (entropy counts them, the mask does not) and lines at / below the fill value: the first
    maximum of the masked matrix, as the float64 closed form and the materialised HIP path give it."""
    from jmac_amd import scoring
    e1, e2, l1, l2, (ia, ib, jc) = ref.seeded_case()
    want = ref.alignment_stats(e1, e2, l1, l2)
    H, rp, ri, cp, ci = scoring.alignment_stats(e1.cuda(), e2.cuda(), l1, l2)
    assert abs(float(H) - float(want[0])) <= 1e-5 * abs(float(want[0]))
    assert_close(rp, want[1], 1e-4, what="row maxima")
    assert_close(cp, want[3], 1e-4, what="column maxima")
    assert torch.equal(ri.cpu(), want[2]) and torch.equal(ci.cpu(), want[4])
    assert int(ri[ia]) == 0 and int(ri[ib]) == 2 and int(ci[jc]) == 0
    H2, P, Q = scoring.alignment_quality(e1.cuda(), e2.cuda(), l1, l2)
    assert abs(float(H) - float(H2)) <= 1e-5 * abs(float(H2))
    assert_close(rp, P.max(1)[0], 1e-4, what="rows, stored path")
    assert_close(cp, Q.max(1)[0], 1e-4, what="columns, stored path")


# ragged in both directions, below one tile, more than 8 column parts (64 columns each), d = 300 / 256 / 48
SHAPES = [(100, 70, 48), (300, 515, 300), (257, 1000, 256), (1000, 129, 300), (130, 2049, 48)]


@pytest.mark.parametrize("n1,n2,d", SHAPES)
def test_maxima_bit_identical_to_the_stored_product(n1, n2, d):
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(n1 * 7 + n2)
    a, b = _unit(n1, d, gen), _unit(n2, d, gen)
    b[5] = b[3]                                      # exact ties along the rows: three equal columns, one in the last part
    b[n2 - 1] = b[3]
    a[n1 - 2] = a[1]                                 # and along the columns
    a[7] = 0.0                                       # an all-equal row
    a, b = a.cuda(), b.cuda()
    S = scoring.sim_matrix(a, b)
    st = scoring.sim_softmax_stats(a, b)
    assert torch.equal(st.row_max, S.max(1)[0]) and torch.equal(st.col_max, S.max(0)[0])
    assert st.row_arg.dtype == torch.int32
    assert np.array_equal(st.row_arg.cpu().numpy(), ref.first_argmax(S, 1))
    assert np.array_equal(st.col_arg.cpu().numpy(), ref.first_argmax(S, 0))
    assert int(st.row_arg[7]) == 0
    rows_only = scoring.sim_softmax_stats(a, b, cols=False)
    assert rows_only.col_max is None and all(torch.equal(x, y) for x, y in zip(rows_only[:4], st[:4]))


def test_maxima_bit_identical_on_the_persistent_super_tile_walk():
    """65 x 65 tiles of 128 x 128: more tiles than resident blocks (every block walks several tiles, the next tile's first slab
    in flight across the statistics epilogue) in the XCD-aware super-tile order, ragged on both edges."""
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(3)
    n1, n2, d = 8200, 8300, 48
    a, b = _unit(n1, d, gen).cuda(), _unit(n2, d, gen).cuda()
    S = scoring.sim_matrix(a, b)
    st = scoring.sim_softmax_stats(a, b)
    assert torch.equal(st.row_max, S.max(1)[0]) and torch.equal(st.col_max, S.max(0)[0])
    assert np.array_equal(st.row_arg.cpu().numpy(), ref.first_argmax(S, 1))
    assert np.array_equal(st.col_arg.cpu().numpy(), ref.first_argmax(S, 0))
    _, hr, hc = scoring.align_entropy(a, b, 20.0)
    assert_close(st.row_ent, hr, 1e-4, what="row entropies")
    assert_close(st.col_ent, hc, 1e-4, what="column entropies")


@pytest.mark.parametrize("n1,n2,d", SHAPES[1:4])
def test_sums_and_entropies_against_the_existing_path(n1, n2, d):
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(n1 + n2)
    a, b = _unit(n1, d, gen).cuda(), _unit(n2, d, gen).cuda()
    st = scoring.sim_softmax_stats(a, b, scale=20.0)
    S = scoring.sim_matrix(a, b)
    P, hr = scoring.row_softmax(S, None, None, 0.0, 20.0, True, True)
    Qt, hc = scoring.col_softmax(S, None, None, 0.0, 20.0, True, True)
    assert_close(1.0 / st.row_sum, P.max(1)[0], 1e-4, what="row sums")
    assert_close(1.0 / st.col_sum, Qt.max(1)[0], 1e-4, what="column sums")
    assert_close(st.row_ent, hr, 1e-4, what="row entropies")
    assert_close(st.col_ent, hc, 1e-4, what="column entropies")
    H, hr2, hc2 = scoring.align_entropy(a, b, 20.0)
    assert_close(st.row_ent, hr2, 1e-4, what="row entropies (align_entropy)")
    assert_close(st.col_ent, hc2, 1e-4, what="column entropies (align_entropy)")
    assert abs(float(st.row_ent.mean() + st.col_ent.mean()) - float(H)) <= 1e-4 * float(H)


def test_stats_at_config5_size_against_oracle_mm_softmax():
    """[3 000 listed, 30 000 entities], d = 300, unit rows of test_get_neg_at_config5_size_against_oracle_mm_topk's recipe,
    against float64 mm + softmax in row slices.  The arg-max must agree on every row whose two largest float64 similarities
    are at least 1e-6 apart (fp32 rounding of a 300-term dot product of unit rows is ~1e-7)."""
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(5)
    N, L, d = 30000, 3000, 300
    emb = torch.nn.functional.normalize(torch.randn(N, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    ill = torch.randperm(N, generator=gen)[:L]
    st = scoring.sim_softmax_stats(emb[ill].cuda(), emb.cuda())
    (rm, ra, rl, rh), (cm, ca, cl, ch), gap = ref.sliced_softmax_stats(emb[ill], emb)
    assert_close(1.0 / st.row_sum, 1.0 / rl, 1e-4, what="row best probability")
    assert_close(1.0 / st.col_sum, 1.0 / cl, 1e-4, what="column best probability")
    assert_close(st.row_ent, rh, 1e-4, what="row entropy")
    assert_close(st.col_ent, ch, 1e-4, what="column entropy")
    assert_close(st.row_max, rm, 1e-6, what="row maximum")
    decided = gap >= 1e-6
    print("decided rows: %d of %d" % (int(decided.sum()), L))
    assert decided.float().mean() > 0.95
    assert torch.equal(st.row_arg.cpu().long()[decided], ra[decided])


def test_alignment_stats_allocates_no_matrix():
    """n1 = n2 = 20 000 all listed: the peak rises by less than HALF of one n1 x n2 fp32 matrix (workspace <= a quarter, two
    gathered operand tables of 24 MB); the materialised path holds more than three such matrices."""
    from jmac_amd import scoring
    n, d = 20000, 300
    gen = torch.Generator().manual_seed(2)
    e1, e2 = _unit(n, d, gen).cuda(), _unit(n, d, gen).cuda()
    lst = list(range(n))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    out = scoring.alignment_stats(e1, e2, lst, lst)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak rise %.1f MB, one matrix %.1f MB" % (rise / 2 ** 20, n * n * 4 / 2 ** 20))
    assert rise < n * n * 4 // 2
    assert out[1].shape == (n,) and bool(torch.isfinite(out[0]))


def test_two_calls_are_bitwise_equal():
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(9)
    a, b = _unit(3000, 300, gen).cuda(), _unit(5000, 300, gen).cuda()
    s1 = scoring.sim_softmax_stats(a, b)
    s2 = scoring.sim_softmax_stats(a, b)
    assert all(torch.equal(x, y) for x, y in zip(s1, s2))
    lst1, lst2 = list(range(0, 3000, 2)), list(range(1, 5000, 3))
    o1, o2 = scoring.alignment_stats(a, b, lst1, lst2), scoring.alignment_stats(a, b, lst1, lst2)
    assert all(torch.equal(x, y) for x, y in zip(o1, o2))
