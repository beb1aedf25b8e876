"""GPU: the alignment evaluator under metric="manhattan" -- s = 1 - L1 distance, CSLS on s -- stored (scoring.alignment_sim) and
without the n1 x n2 matrix (csls_terms, alignment_ranks, alignment_topk, alignment_topk_viable, stable_alignment, alignment_test,
harness.evaluate_alignment, JMAC.alignment_topk) on the L1 tile kernel's CSLS epilogues.

Against the stored path the comparison is bitwise: the tile kernel forms jmac_l1_score_f32's running sum, s = 1 - dist and the
rescoring are the same expressions, and every decision is taken on s or c -- also where 1 - dist rounds two distances to one s.
Against float64 (tests/align_metric_ref.py) the comparison is on DECIDED rows: no float64 competitor within 1e-4 of the value the
decision hangs on (the fp32 running sum of 64 terms on unit rows errs by at most 6.3e-6, so c by about 2.5e-5).

Widths: the top-k switches to its fused form (sample, filter epilogue, candidate lists) at 8 192 columns, so 8 200 is the smallest
width that runs it, ragged against the 64-wide tile; 257 and 260 take the staged form."""
import functools
import os

import numpy as np
import pytest
import torch

import align_metric_ref as ref
import stable_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = torch.nn.functional
M = "manhattan"
# (n1, n2, d, csls_k), normalize
CASES = [((300, 8200, 300, 10), False),      # smallest width on the fused path, ragged against the tile, d = 300
         ((8200, 8200, 20, 10), False),      # both orientations of csls_terms fused
         ((130, 257, 64, 1), False),         # staged
         ((150, 260, 30, 10), False),        # d % 4 != 0, rows of norm ~ 16
         ((150, 260, 30, 10), True)]


@functools.lru_cache(maxsize=None)
def stored(case):
    """Operands as given, the prepared operands, a random gold column per row and the stored S; computed once, never modified."""
    from jmac_amd import scoring
    (n1, n2, d, ck), norm = case
    gen = torch.Generator().manual_seed(2000 + n1 + d)
    if d == 30:
        a, b = torch.randn(n1, d, generator=gen) * 3, torch.randn(n2, d, generator=gen) * 3
    else:
        b = F.normalize(torch.randn(n2, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
        a = F.normalize(torch.randn(n1, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    gold = torch.randint(0, n2, (n1,), generator=gen, dtype=torch.int32)
    a, b, gold = a.cuda(), b.cuda(), gold.cuda()
    pa, pb = scoring._alignment_operands(a, b, M, norm)
    return a, b, pa, pb, gold, scoring.alignment_sim(a, b, M, norm, 0)


@pytest.mark.parametrize("case", CASES)
def test_stored_form_is_one_minus_l1_scores(case):
    from jmac_amd import scoring
    a, b, pa, pb, _, s = stored(case)
    (n1, n2, d, ck), norm = case
    assert s.shape == (n1, n2) and s.dtype == torch.float32
    assert torch.equal(s, 1.0 - scoring.l1_scores(pa, pb))
    assert torch.equal(scoring.alignment_sim(a, b, M, norm, ck), scoring.csls_sim(s, ck))
    # the distance has the same bits from either side: r2 may come from the transposed top-k
    assert torch.equal(scoring.l1_scores(pb, pa), scoring.l1_scores(pa, pb).t())


@pytest.mark.parametrize("case", CASES)
def test_csls_terms_equal_the_stored_forms(case):
    from jmac_amd import scoring
    _, _, pa, pb, _, s = stored(case)
    ck = case[0][3]
    r1, r2 = scoring.csls_terms(pa, pb, ck, M)
    assert torch.equal(r1, scoring.row_topk(s, ck)[0].mean(1))
    assert torch.equal(r2, scoring.col_topk_values(s, ck).mean(1))
    again = scoring.csls_terms(pa, pb, ck, M)
    assert torch.equal(again[0], r1) and torch.equal(again[1], r2)


@pytest.mark.parametrize("case", CASES)
def test_alignment_ranks_equal_csls_rank(case):
    from jmac_amd import scoring
    a, b, _, _, gold, s = stored(case)
    ck, norm = case[0][3], case[1]
    got = scoring.alignment_ranks(a, b, gold, ck, M, norm)
    assert got.dtype == torch.int32 and torch.equal(got, scoring.csls_rank(s, ck, gold))
    assert torch.equal(scoring.alignment_ranks(a, b, gold, ck, M, norm), got)                        # reproducible
    plain = scoring.alignment_ranks(a, b, gold, 0, M, norm)
    assert torch.equal(plain, scoring.filtered_rank(s, gold, descending=True))


@pytest.mark.parametrize("case", CASES)
def test_alignment_topk_equals_row_topk_of_the_rescored_matrix(case):
    from jmac_amd import scoring
    a, b, pa, pb, _, s = stored(case)
    ck, norm = case[0][3], case[1]
    c = scoring.csls_sim(s, ck)
    terms = scoring.csls_terms(pa, pb, ck, M)
    for k in (1, 10, 64):
        idx, val = scoring.alignment_topk(a, b, k, ck, M, norm, terms=terms)
        wval, widx = scoring.row_topk(c, k)
        assert idx.dtype == torch.int64 and torch.equal(idx, widx), k
        assert torch.equal(val, wval), k
        idx2, val2 = scoring.alignment_topk(a, b, k, ck, M, norm, terms=terms)                       # reproducible
        assert torch.equal(idx2, idx) and torch.equal(val2, val), k
    idx, val = scoring.alignment_topk(a, b, 10, ck, M, norm)                                         # its own csls_terms
    wval, widx = scoring.row_topk(c, 10)
    assert torch.equal(idx, widx) and torch.equal(val, wval)
    idx, val = scoring.alignment_topk(a, b, 10, 0, M, norm)                                          # plain s
    wval, widx = scoring.row_topk(s, 10)
    assert torch.equal(idx, widx) and torch.equal(val, wval)


def test_duplicate_columns_tie_exactly_and_resolve_by_index():
    """Columns 7 and 4100 of b are the same row: exact ties in s, in r2 and in c."""
    from jmac_amd import scoring
    n1, n2, d, ck = 300, 8200, 64, 10
    gen = torch.Generator().manual_seed(11)
    b = F.normalize(torch.randn(n2, d, generator=gen))
    b[4100] = b[7]
    a = F.normalize(b[torch.randint(0, n2, (n1,), generator=gen)] + 0.5 * torch.randn(n1, d, generator=gen) / d ** 0.5)
    a[:40] = F.normalize(b[7:8] + 0.3 * torch.randn(40, d, generator=gen) / d ** 0.5)     # rows whose best match IS the tied pair
    a, b = a.cuda(), b.cuda()
    s = scoring.alignment_sim(a, b, M, False, 0)
    c = scoring.csls_sim(s, ck)
    assert torch.equal(c[:, 7], c[:, 4100])
    ranks = {}
    for g in (7, 4100):
        gold = torch.full((n1,), g, dtype=torch.int32).cuda()
        ranks[g] = scoring.alignment_ranks(a, b, gold, ck, M)
        assert torch.equal(ranks[g], scoring.csls_rank(s, ck, gold))
    assert torch.equal(ranks[4100], ranks[7] + 1)                        # the twin with the lower index ranks just before
    idx, val = scoring.alignment_topk(a, b, 10, ck, M)
    wval, widx = scoring.row_topk(c, 10)
    assert torch.equal(idx, widx) and torch.equal(val, wval)
    assert bool((idx[:40, 0] == 7).all()) and bool((idx[:40, 1] == 4100).all())


# ---- selection exits ------------------------------------------------------------------------------------------------------
def test_constant_table_takes_the_overflow_path_and_stays_exact():
    """Every row of b is one vector: all s (and c) of a row are equal, so the rank is gold + 1, the top-k is 0 .. k-1, and every
    candidate list overflows (the selection recomputes the row with the tile's sum, and the arg-max rounds pick by index)."""
    from jmac_amd import scoring
    n1, n2, d, ck = 130, 8200, 64, 10
    gen = torch.Generator().manual_seed(12)
    b = F.normalize(torch.randn(1, d, generator=gen)).repeat(n2, 1).cuda()
    a = F.normalize(torch.randn(n1, d, generator=gen)).cuda()
    gold = torch.randint(0, n2, (n1,), generator=gen, dtype=torch.int32).cuda()
    assert torch.equal(scoring.alignment_ranks(a, b, gold, ck, M), gold + 1)
    assert torch.equal(scoring.alignment_ranks(a, b, gold, 0, M), gold + 1)
    c = scoring.alignment_sim(a, b, M, False, ck)
    for k in (1, 10, 64):
        idx, val = scoring.alignment_topk(a, b, k, ck, M)
        assert torch.equal(idx, torch.arange(k, device="cuda").repeat(n1, 1)), k
        assert torch.equal(val, c[:, :k]), k


def test_far_sample_columns_overflow_the_list_and_stay_exact():
    """The sample columns (the first 2 048) are all far from every row of a: the threshold they give passes every other column,
    each list overflows and the rows take the two-pass selection over recomputed scores."""
    from jmac_amd import scoring
    n1, n2, d = 130, 8200, 64
    gen = torch.Generator().manual_seed(13)
    b = F.normalize(torch.randn(n2, d, generator=gen))
    b[:2048] += 3.0
    a = F.normalize(torch.randn(n1, d, generator=gen))
    a, b = a.cuda(), b.cuda()
    for ck in (10, 0):
        c = scoring.alignment_sim(a, b, M, False, ck)
        for k in (1, 10, 64):
            idx, val = scoring.alignment_topk(a, b, k, ck, M)
            wval, widx = scoring.row_topk(c, k)
            assert torch.equal(idx, widx) and torch.equal(val, wval), (ck, k)
    assert int(idx.min()) >= 2048                                        # nothing of the sample is among the best


@functools.lru_cache(maxsize=None)
def clustered():
    """Noisy copies of 40 distinct rows of b: ~7 suitors share a favourite and most of their next choices."""
    from jmac_amd import scoring
    n1, n2, d = 300, 8200, 64
    gen = torch.Generator().manual_seed(31)
    b = F.normalize(torch.randn(n2, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    src = torch.randperm(n2, generator=gen)[:40][torch.randint(0, 40, (n1,), generator=gen)]
    a = F.normalize(b[src] + 0.1 * torch.randn(n1, d, generator=gen) / d ** 0.5)
    a, b = a.cuda(), b.cuda()
    return a, b, scoring.csls_terms(a, b, 10, M), scoring.alignment_sim(a, b, M, False, 10)


@pytest.mark.parametrize("cols", [8200, 257])
def test_viable_topk_with_nothing_held_is_alignment_topk(cols):
    from jmac_amd import scoring
    a, b, _, _ = clustered()
    b = b[:cols].contiguous()
    terms = scoring.csls_terms(a, b, 10, M)
    free = torch.zeros(cols, dtype=torch.int64, device="cuda")
    for ck, t in ((10, terms), (0, None)):
        for k in (1, 16):
            idx, val = scoring.alignment_topk_viable(a, b, k, free, csls_k=ck, metric=M, terms=t)
            widx, wval = scoring.alignment_topk(a, b, k, ck, M, terms=t)
            assert torch.equal(idx, widx) and torch.equal(val, wval), (ck, k)


@pytest.mark.parametrize("cols", [8200, 257])
def test_viable_topk_against_the_words_of_a_partial_matching(cols):
    """The reviewers' words after deferred acceptance on lists of 4 (suitors that ran out are left open): the viable top-k must be
    the k best of the stored c over the columns whose holder the row would displace."""
    from jmac_amd import scoring
    a, b, terms, c = clustered()
    if cols != c.shape[1]:
        b = b[:cols].contiguous()
        terms = scoring.csls_terms(a, b, 10, M)
        c = scoring.alignment_sim(a, b, M, False, 10)
    n1, n2 = c.shape
    idx4, val4 = scoring.alignment_topk(a, b, 4, 10, M, terms=terms)
    match1, match2 = scoring.stable_matching(idx4, val4, n2)
    assert 0 < int((match1 < 0).sum()) < n1                               # some suitors ran out: the words are a partial state
    taken = match2 >= 0
    col = torch.arange(n2, device="cuda")
    held = c[match2.clamp(min=0), col]                                    # c(holder, j)
    words = np.zeros(n2, dtype=np.uint64)
    t = taken.cpu().numpy()
    words[t] = stable_ref.pack_word(held.cpu().numpy()[t], match2.cpu().numpy()[t])
    best = torch.from_numpy(words.view(np.int64)).cuda()
    rid = torch.arange(n1, device="cuda")
    viable = ~taken[None, :] | (c > held[None, :]) | ((c == held[None, :]) & (rid[:, None] < match2[None, :]))
    masked = torch.where(viable, c, torch.full_like(c, float("-inf")))
    order = torch.sort(masked, dim=1, descending=True, stable=True)
    for k in (1, 10, 64):
        wval = order.values[:, :k]
        widx = torch.where(torch.isneginf(wval), torch.full_like(order.indices[:, :k], -1), order.indices[:, :k])
        idx, val = scoring.alignment_topk_viable(a, b, k, best, csls_k=10, metric=M, terms=terms)
        assert torch.equal(idx, widx) and torch.equal(val, wval), k


# ---- stable matching ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(400, 500), (500, 400)])
def test_stable_alignment_equals_deferred_acceptance_on_the_stored_matrix(n1, n2):
    from jmac_amd import scoring
    d = 32
    gen = torch.Generator().manual_seed(21)
    e2 = torch.randn(n2, d, generator=gen)
    e1 = e2[torch.randint(0, 60, (n1,), generator=gen)] + 0.6 * torch.randn(n1, d, generator=gen)       # crowded favourites
    e1, e2 = e1.cuda(), e2.cuda()
    m1, v1, stats = scoring.stable_alignment(e1, e2, k=4, csls_k=10, metric=M)
    print(stats)
    c = scoring.alignment_sim(e1, e2, M, False, 10).cpu().numpy()
    w1, _ = stable_ref.stable_dense(c)
    m1 = m1.cpu().numpy()
    assert np.array_equal(m1, w1)
    assert stats["complete"] and stats["unmatched"] == max(0, n1 - n2) == int((w1 < 0).sum())
    assert stats["refills"] >= 1                                         # lists of 4 run out
    v1 = v1.cpu().numpy()
    held = m1 >= 0
    assert np.array_equal(v1[held], c[np.nonzero(held)[0], m1[held]]) and bool(np.all(np.isneginf(v1[~held])))


# ---- against float64 ------------------------------------------------------------------------------------------------------
TOL = 1e-4


@functools.lru_cache(maxsize=None)
def f64_case():
    n1, n2, d, ck = 300, 8200, 64, 10
    gen = torch.Generator().manual_seed(22)
    b = F.normalize(torch.randn(n2, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    gold = torch.randperm(n2, generator=gen)[:n1]
    a = F.normalize(b[gold] + 1.5 * torch.randn(n1, d, generator=gen) / d ** 0.5)
    s = ref.manhattan_sim(a.numpy(), b.numpy())
    c = ref.csls(s, ck)
    g = gold.numpy()
    rank = ref.ranks(c, g)
    rank_decided = (np.abs(c - c[np.arange(n1), g][:, None]) < TOL).sum(1) == 1           # nothing but the gold itself
    order = np.argsort(-c, axis=1, kind="stable")[:, :11]
    top = np.take_along_axis(c, order, 1)
    order_decided = ((top[:, :-1] - top[:, 1:]) >= TOL).all(1)                           # a gap below each of the top 10
    return a, b, gold, s, rank, rank_decided, order[:, :10], order_decided


def test_stored_similarity_against_float64():
    from jmac_amd import scoring
    a, b, _, s64, _, _, _, _ = f64_case()
    s = scoring.alignment_sim(a.cuda(), b.cuda(), M, False, 0).cpu().numpy()
    err = float(np.abs(s - s64).max())
    print("max |S - float64| = %.3g" % err)
    assert err <= 1e-4


def test_ranks_and_top10_against_float64():
    from jmac_amd import scoring
    a, b, gold, _, rank, rank_decided, top10, order_decided = f64_case()
    print("decided rows: ranks %.4f, top-10 %.4f" % (rank_decided.mean(), order_decided.mean()))
    assert rank_decided.mean() >= 0.9 and order_decided.mean() >= 0.9
    got = scoring.alignment_ranks(a.cuda(), b.cuda(), gold.cuda(), 10, M).cpu().numpy()
    print("decided rows with another rank: %d" % int(((got != rank) & rank_decided).sum()))
    assert np.array_equal(got[rank_decided], rank[rank_decided])
    idx = scoring.alignment_topk(a.cuda(), b.cuda(), 10, 10, M)[0].cpu().numpy()
    print("decided rows with another top-10: %d" % int((idx != top10)[order_decided].any(1).sum()))
    assert np.array_equal(idx[order_decided], top10[order_decided])


# ---- fixture, harness, model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix_free", [False, True])
@pytest.mark.parametrize("normalize,csls_k", [(False, 0), (False, 10), (True, 0), (True, 10)])
def test_alignment_test_reproduces_the_reference_fixture(normalize, csls_k, matrix_free):
    from jmac_amd import scoring
    z = np.load(os.path.join(GOLD, "align_eval.npz"))
    g = np.load(os.path.join(GOLD, "align_manhattan.npz"))
    tag = "n%d_csls%d" % (int(normalize), csls_k)
    e1, e2 = torch.from_numpy(z["e1"]).cuda(), torch.from_numpy(z["e2"]).cuda()
    top_k, hits, mr, mrr = scoring.alignment_test(e1, e2, (1, 5, 10), M, normalize, csls_k, matrix_free=matrix_free)
    assert top_k == [1, 5, 10] and np.allclose(hits, g["hits_" + tag], atol=1e-9)
    assert abs(mr - float(g["mr_" + tag])) < 1e-9 and abs(mrr - float(g["mrr_" + tag])) < 1e-9


@functools.lru_cache(maxsize=None)
def mini():
    from jmac_amd import data, harness
    from jmac_amd.model import JMAC
    torch.manual_seed(0)
    kgs, s_train, s_test, n_ent = data.load_dbp5l(os.path.join(GOLD, "dbp5l_mini"), "ja")
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, dropout=0.0)
    name_emb = np.random.default_rng(0).standard_normal((n_ent, 24)).astype(np.float32)
    model = JMAC(args, name_emb, sum(kg.num_relation for kg in kgs.values()), n_ent).cuda()
    (l1, l2), pairs = sorted(s_test.items())[0]
    kg1, kg2 = kgs[l1], kgs[l2]
    graphs = tuple((torch.from_numpy(kg.edge_index).cuda(), torch.from_numpy(kg.edge_type).cuda()) for kg in (kg1, kg2))
    return model, kg1, kg2, np.asarray(pairs, dtype=np.int64), graphs, args


def _blocks(kg1, kg2, graphs):
    return [(ei, et, [kg.entity_id_base, kg.upper_entity_base], [kg.relation_id_base, kg.upper_relation_base])
            for kg, (ei, et) in zip((kg1, kg2), graphs)]


@pytest.mark.parametrize("csls_k", [0, 10])
def test_harness_evaluate_alignment_reads_the_metric_from_args(csls_k):
    import copy
    from jmac_amd import harness, scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(_blocks(kg1, kg2, graphs), on_device=True)
    model.train()
    p = torch.from_numpy(pairs).cuda()
    e1, e2 = a1[p[:, 0]], a2[p[:, 1]]
    assert args.eval_metric == "cosine" and args.eval_norm is False
    assert harness.evaluate_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=csls_k) == \
        scoring.alignment_test(e1, e2, (1, 5, 10), "cosine", False, csls_k)
    for norm in (False, True):
        margs = copy.copy(args)
        margs.eval_metric, margs.eval_norm = M, norm
        want = scoring.alignment_test(e1, e2, (1, 5, 10), M, norm, csls_k)
        for mf in (True, False):
            assert harness.evaluate_alignment(model, kg1, kg2, pairs, graphs, margs, csls_k=csls_k, matrix_free=mf) == want
    assert model.training


def test_harness_evaluate_stable_alignment_reads_the_metric_from_args():
    import copy
    from jmac_amd import harness, scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    margs = copy.copy(args)
    margs.eval_metric = M
    precision, stats = harness.evaluate_stable_alignment(model, kg1, kg2, pairs, graphs, margs, csls_k=10, k=4)
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(_blocks(kg1, kg2, graphs), on_device=True)
    model.train()
    p = torch.from_numpy(pairs).cuda()
    w1, _ = stable_ref.stable_dense(scoring.alignment_sim(a1[p[:, 0]], a2[p[:, 1]], M, False, 10).cpu().numpy())
    assert stats["complete"] and abs(precision - 100.0 * float((w1 == np.arange(len(w1))).mean())) < 1e-9


def test_model_alignment_topk_and_stable_pass_the_metric_through():
    from jmac_amd import scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    blocks = _blocks(kg1, kg2, graphs)
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(blocks, on_device=True)
        q, gold = pairs[:, 0], torch.from_numpy(pairs[:, 1]).cuda()
        idx, val = model.alignment_topk(q, 5, blocks, metric=M, emb=(a1, a2))
        qs = np.unique(q)[:23]
        m1, v1, stats = model.alignment_stable(qs, blocks, k=4, metric=M, emb=(a1, a2))
    model.train()
    qd = torch.from_numpy(q).cuda()
    c = scoring.alignment_sim(a1, a2, M, False, 10)
    wval, widx = scoring.row_topk(c, 5)
    assert torch.equal(idx, widx[qd]) and torch.equal(val, wval[qd])
    t1, t2 = scoring.csls_terms(a1, a2, 10, M)
    ranks = scoring.alignment_ranks(a1[qd], a2, gold, 10, M, terms=(t1[qd], t2))
    assert torch.equal(ranks == 1, idx[:, 0] == gold)                     # the best match is the gold exactly where it ranks first
    w1, _ = stable_ref.stable_dense(c.cpu().numpy()[qs])
    assert np.array_equal(m1.cpu().numpy(), w1) and stats["complete"]


def test_argument_errors():
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(3)
    e1, e2 = torch.randn(40, 16, generator=gen).cuda(), torch.randn(70, 16, generator=gen).cuda()
    gold = torch.zeros(40, dtype=torch.int32).cuda()
    with pytest.raises(NotImplementedError):
        scoring.alignment_ranks(e1, e2, gold, metric="euclidean")
    with pytest.raises(NotImplementedError):
        scoring.alignment_sim(e1, e2, "euclidean")
    with pytest.raises(IndexError):
        scoring.alignment_ranks(e1, e2, torch.full((40,), 70, dtype=torch.int32).cuda(), metric=M)
    with pytest.raises(IndexError):
        scoring.alignment_ranks(e1, e2, [-1] * 40, metric=M)
    for k in (0, 65, 71):
        with pytest.raises(ValueError):
            scoring.alignment_topk(e1, e2, k, metric=M)
    with pytest.raises(ValueError):
        scoring.alignment_topk(e1, e2[:50], 64, metric=M)                 # k > n2
    with pytest.raises(ValueError):
        scoring.alignment_topk_viable(e1, e2, 65, torch.zeros(70, dtype=torch.int64).cuda(), metric=M)
    with pytest.raises(ValueError):
        scoring.stable_alignment(e1, e2, k=65, metric=M)
    with pytest.raises(ValueError):
        scoring.csls_terms(e1, e2, 65, M)
