"""GPU: alignment evaluation and inference without the n1 x n2 matrix -- scoring.csls_terms / alignment_ranks / alignment_topk,
alignment_test(matrix_free=True), harness.evaluate_alignment, JMAC.alignment_topk.

Against the stored path the comparison is bitwise: the matrix-free forms consume the products of jmac_sim_matrix_f32 bit for bit
and rescore them with the same expression, so there is no tolerance.  Against float64 on the CPU the comparison is on DECIDED
rows: those where no competitor's float64 score lies within 1e-5 of the value the decision hangs on (the fp32 error of a
rescored unit-row dot product is ~1e-6).

Widths: jmac_sim_topk_f32 switches to its matrix-free path at 8 192 columns, so 8 200 is the smallest width that runs it, ragged
against the 64-, 128- and 256-wide tiles; 257 takes the staged path."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(300, 8200, 300, 10), (8200, 8200, 20, 10), (8320, 8200, 64, 16), (130, 257, 64, 1)]
F = torch.nn.functional


@functools.lru_cache(maxsize=None)
def stored(shape):
    """Operands, a random gold column per row and the stored path's matrix for one shape; computed once, never modified."""
    from jmac_amd import scoring
    n1, n2, d, ck = shape
    gen = torch.Generator().manual_seed(1000 + n1 + d)
    b = F.normalize(torch.randn(n2, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    a = F.normalize(torch.randn(n1, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    gold = torch.randint(0, n2, (n1,), generator=gen, dtype=torch.int32)
    a, b, gold = a.cuda(), b.cuda(), gold.cuda()
    return a, b, gold, scoring.sim_matrix(a, b)


@pytest.mark.parametrize("shape", SHAPES)
def test_csls_terms_equal_the_stored_forms(shape):
    from jmac_amd import scoring
    a, b, _, s = stored(shape)
    ck = shape[3]
    r1, r2 = scoring.csls_terms(a, b, ck)
    assert torch.equal(r1, scoring.row_topk(s, ck)[0].mean(1))
    assert torch.equal(r2, scoring.col_topk_values(s, ck).mean(1))


@pytest.mark.parametrize("shape", SHAPES)
def test_alignment_ranks_equal_csls_rank(shape):
    from jmac_amd import scoring
    a, b, gold, s = stored(shape)
    ck = shape[3]
    got = scoring.alignment_ranks(a, b, gold, csls_k=ck, metric="inner")
    assert got.dtype == torch.int32 and torch.equal(got, scoring.csls_rank(s, ck, gold))
    assert torch.equal(scoring.alignment_ranks(a, b, gold, csls_k=ck, metric="inner"), got)             # reproducible
    plain = scoring.alignment_ranks(a, b, gold, csls_k=0, metric="inner")
    assert torch.equal(plain, scoring.filtered_rank(s, gold, descending=True))


@pytest.mark.parametrize("shape", SHAPES)
def test_alignment_topk_equals_row_topk_of_the_rescored_matrix(shape):
    from jmac_amd import scoring
    a, b, _, s = stored(shape)
    ck = shape[3]
    c = scoring.csls_sim(s, ck)
    terms = scoring.csls_terms(a, b, ck)
    for k in (1, 10, 64):
        idx, val = scoring.alignment_topk(a, b, k, csls_k=ck, metric="inner", terms=terms)
        wval, widx = scoring.row_topk(c, k)
        assert idx.dtype == torch.int64 and torch.equal(idx, widx), k
        assert torch.equal(val, wval), k
        idx2, val2 = scoring.alignment_topk(a, b, k, csls_k=ck, metric="inner", terms=terms)             # reproducible
        assert torch.equal(idx2, idx) and torch.equal(val2, val), k
    idx, val = scoring.alignment_topk(a, b, 10, csls_k=ck, metric="inner")                               # its own csls_terms
    wval, widx = scoring.row_topk(c, 10)
    assert torch.equal(idx, widx) and torch.equal(val, wval)
    idx, val = scoring.alignment_topk(a, b, 10, csls_k=0, metric="inner")
    widx, wval = scoring.sim_topk(a, b, 10, return_values=True)
    assert torch.equal(idx, widx) and torch.equal(val, wval)


def test_cosine_and_normalize_are_handled_as_alignment_sim_does():
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(3)
    e1 = (torch.randn(150, 30, generator=gen) * 3).cuda()               # not unit rows, d % 4 != 0
    e2 = (torch.randn(260, 30, generator=gen) * 3).cuda()
    gold = torch.randint(0, 260, (150,), generator=gen, dtype=torch.int32).cuda()
    for metric, normalize in (("cosine", False), ("inner", True), ("inner", False)):
        s = scoring.alignment_sim(e1, e2, metric, normalize, 0)
        assert torch.equal(scoring.alignment_ranks(e1, e2, gold, 10, metric, normalize), scoring.csls_rank(s, 10, gold))
        idx, val = scoring.alignment_topk(e1, e2, 5, 10, metric, normalize)
        wval, widx = scoring.row_topk(scoring.alignment_sim(e1, e2, metric, normalize, 10), 5)
        assert torch.equal(idx, widx) and torch.equal(val, wval)
    with pytest.raises(IndexError):
        scoring.alignment_ranks(e1, e2, torch.full((150,), 260, dtype=torch.int32).cuda())
    with pytest.raises(IndexError):
        scoring.alignment_ranks(e1, e2, [-1] * 150)
    with pytest.raises(NotImplementedError):
        scoring.alignment_ranks(e1, e2, gold, metric="euclidean")


def test_duplicate_columns_tie_exactly_and_resolve_by_index():
    """Columns 7 and 4100 of b are the same row: exact ties in S, in r2 and in c."""
    from jmac_amd import scoring
    n1, n2, d, ck = 300, 8200, 64, 10
    gen = torch.Generator().manual_seed(11)
    b = F.normalize(torch.randn(n2, d, generator=gen))
    b[4100] = b[7]
    a = F.normalize(b[torch.randint(0, n2, (n1,), generator=gen)] + 0.5 * torch.randn(n1, d, generator=gen) / d ** 0.5)
    a[:40] = F.normalize(b[7:8] + 0.3 * torch.randn(40, d, generator=gen) / d ** 0.5)     # rows whose best match IS the tied pair
    a, b = a.cuda(), b.cuda()
    s = scoring.sim_matrix(a, b)
    c = scoring.csls_sim(s, ck)
    assert torch.equal(c[:, 7], c[:, 4100])
    for g in (7, 4100):
        gold = torch.full((n1,), g, dtype=torch.int32).cuda()
        got = scoring.alignment_ranks(a, b, gold, ck, "inner")
        assert torch.equal(got, scoring.csls_rank(s, ck, gold))
    lo = scoring.alignment_ranks(a, b, torch.full((n1,), 7, dtype=torch.int32).cuda(), ck, "inner")
    hi = scoring.alignment_ranks(a, b, torch.full((n1,), 4100, dtype=torch.int32).cuda(), ck, "inner")
    assert torch.equal(hi, lo + 1)                                       # the twin with the lower index ranks just before
    idx, val = scoring.alignment_topk(a, b, 10, ck, "inner")
    wval, widx = scoring.row_topk(c, 10)
    assert torch.equal(idx, widx) and torch.equal(val, wval)
    assert bool((idx[:40, 0] == 7).all()) and bool((idx[:40, 1] == 4100).all())


def test_constant_columns_take_the_overflow_path_and_stay_exact():
    """Every row of b is one vector: all c of a row are equal, so the rank is gold + 1, the top-k is 0 .. k-1, and every
    candidate list overflows (the selection recomputes and rescores)."""
    from jmac_amd import scoring
    n1, n2, d, ck = 130, 8200, 64, 10
    gen = torch.Generator().manual_seed(12)
    b = F.normalize(torch.randn(1, d, generator=gen)).repeat(n2, 1).cuda()
    a = F.normalize(torch.randn(n1, d, generator=gen)).cuda()
    gold = torch.randint(0, n2, (n1,), generator=gen, dtype=torch.int32).cuda()
    assert torch.equal(scoring.alignment_ranks(a, b, gold, ck, "inner"), gold + 1)
    assert torch.equal(scoring.alignment_ranks(a, b, gold, 0, "inner"), gold + 1)
    c = scoring.csls_sim(scoring.sim_matrix(a, b), ck)
    for k in (1, 10, 64):
        idx, val = scoring.alignment_topk(a, b, k, ck, "inner")
        assert torch.equal(idx, torch.arange(k, device="cuda").repeat(n1, 1)), k
        assert torch.equal(val, c[:, :k]), k


@pytest.mark.parametrize("csls_k", [0, 10])
def test_alignment_test_matrix_free_on_the_golden_fixture(csls_k):
    from jmac_amd import scoring
    z = np.load(os.path.join(GOLD, "align_eval.npz"))
    e1, e2 = torch.from_numpy(z["e1"]).cuda(), torch.from_numpy(z["e2"]).cuda()
    want = scoring.alignment_test(e1, e2, csls_k=csls_k)
    assert scoring.alignment_test(e1, e2, csls_k=csls_k, matrix_free=True) == want


# ---- against float64 on the CPU ------------------------------------------------------------------------------------------
F64_CASES = [(8200, 8200, 64, 1.5, 23), (300, 8200, 300, 3.0, 22)]
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def f64_case(case):
    import oracle.jmac_oracle as orc
    n1, n2, d, noise, seed = case
    gen = torch.Generator().manual_seed(seed)
    b = F.normalize(torch.randn(n2, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    gold = torch.randperm(n2, generator=gen)[:n1]
    a = F.normalize(b[gold] + noise * torch.randn(n1, d, generator=gen) / d ** 0.5)
    c = orc.csls_sim(a.double() @ b.double().t(), 10)
    g = c.gather(1, gold.view(-1, 1))
    ar = torch.arange(n2).view(1, -1)
    rank = ((c > g) | ((c == g) & (ar < gold.view(-1, 1)))).sum(1) + 1                  # orc.alignment_test's rule
    rank_decided = ((c - g).abs() < TOL).sum(1) == 1                                     # nothing but the gold itself
    top = torch.topk(c, 11, dim=1)
    gaps = top.values[:, :-1] - top.values[:, 1:]                                        # gap below each of the top 10
    return a, b, gold, rank, rank_decided, top.indices[:, :10], gaps[:, 9] >= TOL, (gaps >= TOL).all(1)


@pytest.mark.parametrize("case", F64_CASES)
def test_ranks_against_float64(case):
    from jmac_amd import scoring
    a, b, gold, rank, decided, _, _, _ = f64_case(case)
    share = float(decided.float().mean())
    print("decided rows: %.4f, Hits@1 %.3f, largest rank %d" % (share, float((rank == 1).float().mean()), int(rank.max())))
    assert share >= 0.97
    got = scoring.alignment_ranks(a.cuda(), b.cuda(), gold.cuda(), 10).cpu().long()
    wrong = (got != rank) & decided
    print("decided rows with another rank: %d; undecided rows that differ: %d" % (int(wrong.sum()), int((got != rank).sum() - wrong.sum())))
    assert not bool(wrong.any())


@pytest.mark.parametrize("case", F64_CASES)
def test_top10_against_float64(case):
    from jmac_amd import scoring
    a, b, _, _, _, ref, set_decided, order_decided = f64_case(case)
    print("decided: set %.4f, order %.4f" % (float(set_decided.float().mean()), float(order_decided.float().mean())))
    assert float(order_decided.float().mean()) >= 0.97
    got = scoring.alignment_topk(a.cuda(), b.cuda(), 10, 10)[0].cpu()
    same_set = (got.sort(1).values == ref.sort(1).values).all(1)
    print("decided rows with another set: %d, with another order: %d" % (int((~same_set[set_decided]).sum()),
                                                                         int((got != ref)[order_decided].any(1).sum())))
    assert bool(same_set[set_decided].all())
    assert bool((got == ref)[order_decided].all())


def test_hits_against_the_oracle_evaluator():
    import oracle.jmac_oracle as orc
    from jmac_amd import scoring
    a, b, gold, _, decided, _, _, _ = f64_case(F64_CASES[0])
    e2 = b[gold]                                                         # row i of a is aligned with row i of e2
    _, want, _, _, _ = orc.alignment_test(a, e2, (1, 5, 10), 10)
    top_k, hits, mr, mrr = scoring.alignment_test(a.cuda(), e2.cuda(), (1, 5, 10), csls_k=10, matrix_free=True)
    slack = 100.0 * int((~decided).sum()) / len(a) + 2e-3                # each undecided row may fall on either side (+ two roundings to 3 places)
    print("Hits@1/5/10: %s, oracle %s, slack %.4f" % (hits, want, slack))
    assert top_k == [1, 5, 10] and all(abs(h - w) <= slack for h, w in zip(hits, want))
    assert 1.0 <= mr and 0.0 < mrr <= 1.0


# ---- harness and model -------------------------------------------------------------------------------------------------
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
def test_harness_evaluate_alignment(csls_k):
    from jmac_amd import harness, scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    got = harness.evaluate_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=csls_k)
    assert model.training
    assert harness.evaluate_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=csls_k, matrix_free=False) == got
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(_blocks(kg1, kg2, graphs), pyt=True)
    model.train()
    want = scoring.alignment_test(a1[pairs[:, 0]].cuda(), a2[pairs[:, 1]].cuda(), (1, 5, 10), csls_k=csls_k)
    assert got == want
    assert got[0] == [1, 5, 10] and 1.0 <= got[2] <= len(pairs)


def test_model_alignment_topk():
    from jmac_amd import scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    blocks = _blocks(kg1, kg2, graphs)
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(blocks, on_device=True)
        q = pairs[:17, 0]
        idx, val = model.alignment_topk(q, 5, blocks)
        idx2, val2 = model.alignment_topk(torch.from_numpy(q).cuda(), 5, blocks, emb=(a1, a2))
    model.train()
    wval, widx = scoring.row_topk(scoring.alignment_sim(a1, a2, "cosine", False, 10), 5)
    assert torch.equal(idx, widx[q]) and torch.equal(val, wval[q])
    assert torch.equal(idx2, idx) and torch.equal(val2, val)
    with pytest.raises(IndexError):
        model.alignment_topk([kg1.num_entity], 5, blocks, emb=(a1, a2))
