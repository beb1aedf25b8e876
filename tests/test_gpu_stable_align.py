"""GPU: the stable one-to-one alignment -- scoring.stable_matching (deferred acceptance on given lists), scoring.stable_alignment
(top-k lists + viable refills, no n1 x n2 matrix), scoring.alignment_topk_viable, JMAC.alignment_stable and
harness.evaluate_stable_alignment -- against sequential Gale-Shapley on the CPU (tests/stable_ref.py).

The dense reference runs on ``scoring.alignment_sim(..)`` copied to the host: that stored form is bit-identical to the values
the matrix-free path decides on, and with strict preferences the suitor-optimal stable matching is unique, so every comparison is
exact equality of integer arrays.

Widths: the top-k switches to its fused (sample / filter epilogue / candidate lists) form at 8 192 columns; 8 200 is the smallest
ragged width that runs it, everything below takes the staged form."""
import functools
import os

import numpy as np
import pytest
import torch

import stable_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = torch.nn.functional


def _dense(e1, e2, metric="cosine", normalize=False, csls_k=10):
    from jmac_amd import scoring
    return scoring.alignment_sim(e1, e2, metric, normalize, csls_k).cpu().numpy()


def _check_against_dense(c, m1, v1, stats, want_unmatched=0):
    w1, w2 = stable_ref.stable_dense(c)
    m1 = m1.cpu().numpy()
    assert np.array_equal(m1, w1)
    assert stats["complete"] and stats["unmatched"] == want_unmatched == int((w1 < 0).sum())
    assert stable_ref.blocking_pairs(c, m1) == 0
    v1 = v1.cpu().numpy()
    held = m1 >= 0
    assert np.array_equal(v1[held], c[np.nonzero(held)[0], m1[held]]) and bool(np.all(np.isneginf(v1[~held])))
    return w1, w2


# ---- the matching kernel alone ---------------------------------------------------------------------------------------------
def test_stable_matching_on_random_incomplete_lists_with_ties():
    from jmac_amd import scoring
    n1, n2, k = 700, 500, 3
    rng = np.random.default_rng(5)
    idx = np.stack([rng.permutation(n2)[:k] for _ in range(n1)]).astype(np.int64)
    val = (np.round(rng.standard_normal((n1, k)) * 2) / 4).astype(np.float32)            # quantised to 1/4: many exact ties
    val = -np.sort(-val, axis=1)
    cut = rng.integers(0, k + 1, n1)                                                      # some lists are shorter (a few empty)
    cut[rng.random(n1) < 0.6] = k
    idx[np.arange(k)[None, :] >= cut[:, None]] = -1
    w1, w2 = stable_ref.stable_lists(idx, val, n2)
    m1, m2 = scoring.stable_matching(torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda(), n2)
    assert m1.dtype == torch.int64 and m2.dtype == torch.int64
    assert np.array_equal(m1.cpu().numpy(), w1) and np.array_equal(m2.cpu().numpy(), w2)
    assert 0 < int((w1 < 0).sum()) < n1
    again = scoring.stable_matching(torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda(), n2)
    assert torch.equal(again[0], m1) and torch.equal(again[1], m2)


def test_stable_matching_crowd_on_eight_reviewers():
    """600 suitors, every list a permutation of the same 8 reviewers: long displacement chains, 592 suitors run out."""
    from jmac_amd import scoring
    n1, n2, k = 600, 20, 8
    rng = np.random.default_rng(6)
    idx = np.stack([rng.permutation(8) + 3 for _ in range(n1)]).astype(np.int64)
    val = -np.sort(-rng.standard_normal((n1, k)).astype(np.float32), axis=1)
    w1, w2 = stable_ref.stable_lists(idx, val, n2)
    m1, m2 = scoring.stable_matching(torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda(), n2)
    assert np.array_equal(m1.cpu().numpy(), w1) and np.array_equal(m2.cpu().numpy(), w2)
    assert int((w1 >= 0).sum()) == 8


# ---- the whole alignment ------------------------------------------------------------------------------------------------
def test_narrow_refill_heavy():
    from jmac_amd import scoring
    n, d = 300, 32
    gen = torch.Generator().manual_seed(21)
    e2 = torch.randn(n, d, generator=gen)
    e1 = e2[torch.randint(0, 60, (n,), generator=gen)] + 0.6 * torch.randn(n, d, generator=gen)      # crowded favourites
    e1, e2 = e1.cuda(), e2.cuda()
    m1, v1, stats = scoring.stable_alignment(e1, e2, k=2, csls_k=10)
    print(stats)
    c = _dense(e1, e2)
    w1, w2 = _check_against_dense(c, m1, v1, stats)
    assert stats["refills"] >= 1 and bool((m1 >= 0).all())
    m2 = np.full(n, -1)
    m2[m1.cpu().numpy()] = np.arange(n)
    assert np.array_equal(m2, w2)
    again = scoring.stable_alignment(e1, e2, k=2, csls_k=10)
    assert torch.equal(again[0], m1) and torch.equal(again[1], v1) and again[2] == stats


@pytest.mark.parametrize("n1,n2", [(150, 260), (260, 150)])
def test_rectangular_unnormalised(n1, n2):
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(3)
    e1 = (torch.randn(n1, 30, generator=gen) * 3).cuda()                 # not unit rows, d % 4 != 0
    e2 = (torch.randn(n2, 30, generator=gen) * 3).cuda()
    for metric, normalize, ck in (("cosine", False, 10), ("inner", True, 10), ("inner", False, 10), ("cosine", False, 0)):
        m1, v1, stats = scoring.stable_alignment(e1, e2, k=16, csls_k=ck, metric=metric, normalize=normalize)
        _check_against_dense(_dense(e1, e2, metric, normalize, ck), m1, v1, stats, want_unmatched=max(0, n1 - n2))


@functools.lru_cache(maxsize=None)
def clustered():
    """test_gpu_align_matrix_free.py's noisy copies, drawn from 40 distinct rows of b with little noise: ~7 suitors share a
    favourite and most of their next choices, so lists of 4 run out."""
    n1, n2, d = 300, 8200, 64
    gen = torch.Generator().manual_seed(31)
    b = F.normalize(torch.randn(n2, d, generator=gen) + 0.3 * torch.randn(1, d, generator=gen))
    src = torch.randperm(n2, generator=gen)[:40][torch.randint(0, 40, (n1,), generator=gen)]
    a = F.normalize(b[src] + 0.1 * torch.randn(n1, d, generator=gen) / d ** 0.5)
    return a.cuda(), b.cuda()


def test_fused_path_with_refills():
    from jmac_amd import scoring
    a, b = clustered()
    m1, v1, stats = scoring.stable_alignment(a, b, k=4, csls_k=10, metric="inner")
    print(stats)
    _check_against_dense(_dense(a, b, "inner"), m1, v1, stats)
    assert stats["refills"] >= 1


def test_exact_ties_go_to_the_lower_index():
    """Rows 5 and 140 of a are one vector, columns 7 and 4100 of b another, and that vector's favourite is the twin column: four
    equal scores.  Suitor 5 takes reviewer 7 (lower suitor id, lower reviewer id), suitor 140 the twin."""
    from jmac_amd import scoring
    n1, n2, d = 300, 8200, 64
    gen = torch.Generator().manual_seed(32)
    b = F.normalize(torch.randn(n2, d, generator=gen))
    b[4100] = b[7]
    a = F.normalize(b[torch.randperm(n2, generator=gen)[:n1] // 2 * 2 + 1] + 0.5 * torch.randn(n1, d, generator=gen) / d ** 0.5)
    a[5] = F.normalize(b[7:8] + 0.05 * torch.randn(1, d, generator=gen) / d ** 0.5)[0]
    a[140] = a[5]
    a, b = a.cuda(), b.cuda()
    m1, v1, stats = scoring.stable_alignment(a, b, k=4, csls_k=10, metric="inner")
    c = _dense(a, b, "inner")
    assert c[5, 7] == c[140, 7] == c[5, 4100] == c[140, 4100] == c[5].max()
    _check_against_dense(c, m1, v1, stats)
    assert int(m1[5]) == 7 and int(m1[140]) == 4100


@pytest.mark.parametrize("n1,n2,k", [(200, 200, 16), (130, 8200, 32)])
def test_constant_tables(n1, n2, k):
    """Every score is equal: suitor i ends with reviewer i, list after list through the top-k's overflow recompute."""
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(12)
    row = F.normalize(torch.randn(1, 64, generator=gen))
    a, b = row.repeat(n1, 1).cuda(), row.repeat(n2, 1).cuda()
    m1, v1, stats = scoring.stable_alignment(a, b, k=k, csls_k=10, metric="inner")
    print(stats)
    assert torch.equal(m1, torch.arange(n1, device="cuda"))
    assert stats["complete"] and stats["unmatched"] == 0 and stats["refills"] == (n1 - 1) // k
    assert torch.equal(v1, scoring.alignment_sim(a, b, "inner", False, 10)[:, 0])


# ---- the viable top-k alone ------------------------------------------------------------------------------------------------
def _masked_topk(c, best, row_id, k):
    """k best viable columns per row of the stored matrix c, by a stable sort (descending, lower index first)."""
    words = stable_ref.pack_word(c, np.asarray(row_id)[:, None])
    masked = np.where(words > best[None, :], c, -np.inf).astype(np.float32)
    order = np.argsort(-masked, axis=1, kind="stable")[:, :k]
    val = np.take_along_axis(masked, order, 1)
    return np.where(np.isneginf(val), -1, order), val


@functools.lru_cache(maxsize=None)
def viable_case():
    from jmac_amd import scoring
    a, b = clustered()
    terms = scoring.csls_terms(a, b, 10)
    return a, b, terms, scoring.alignment_sim(a, b, "inner", False, 10).cpu().numpy()


def test_viable_topk_with_most_columns_held():
    from jmac_amd import scoring
    a, b, terms, c = viable_case()
    n1, n2 = c.shape
    rng = np.random.default_rng(41)
    row_id = rng.permutation(5000)[:n1].astype(np.int32)                                   # the rows stand for other suitor ids
    best = np.zeros(n2, dtype=np.uint64)
    kind = rng.random(n2)
    strong = kind < 0.6                                                                    # nobody wins these
    best[strong] = stable_ref.pack_word(np.full(int(strong.sum()), 10.0, np.float32), rng.integers(0, 5000, int(strong.sum())))
    own = (kind >= 0.6) & (kind < 0.9)                                                     # held by one of the rows with its own score:
    rows = rng.integers(0, n1, n2)                                                         # some rows beat it, that row ties with itself
    best[own] = stable_ref.pack_word(c[rows[own], np.nonzero(own)[0]], row_id[rows[own]])
    for k in (1, 10, 64):
        widx, wval = _masked_topk(c, best, row_id, k)
        idx, val = scoring.alignment_topk_viable(a, b, k, torch.from_numpy(best.view(np.int64)).cuda(), torch.from_numpy(row_id).cuda(),
                                                 csls_k=10, metric="inner", terms=terms)
        assert np.array_equal(idx.cpu().numpy(), widx), k
        assert np.array_equal(val.cpu().numpy(), wval), k
    # raw similarities (csls_k = 0) take the same predicate
    s = scoring.alignment_sim(a, b, "inner", False, 0).cpu().numpy()
    best0 = best.copy()
    best0[own] = stable_ref.pack_word(s[rows[own], np.nonzero(own)[0]], row_id[rows[own]])
    widx, wval = _masked_topk(s, best0, row_id, 10)
    idx, val = scoring.alignment_topk_viable(a, b, 10, torch.from_numpy(best0.view(np.int64)).cuda(), torch.from_numpy(row_id).cuda(),
                                             csls_k=0, metric="inner")
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(val.cpu().numpy(), wval)


def test_viable_topk_with_three_columns_left():
    from jmac_amd import scoring
    a, b, terms, c = viable_case()
    a, c = a[:64], c[:64]
    n2 = c.shape[1]
    best = stable_ref.pack_word(np.full(n2, 10.0, np.float32), np.zeros(n2, dtype=np.int64))
    best[[5, 3000, 8199]] = 0
    row_id = np.arange(64, dtype=np.int32)
    widx, wval = _masked_topk(c, best, row_id, 10)
    assert bool((widx[:, 3:] == -1).all()) and bool((widx[:, :3] >= 0).all())
    idx, val = scoring.alignment_topk_viable(a, b, 10, torch.from_numpy(best.view(np.int64)).cuda(), csls_k=10, metric="inner",
                                             terms=(terms[0][:64], terms[1]))
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(val.cpu().numpy(), wval)


@pytest.mark.parametrize("cols", [8200, 257])
def test_viable_topk_with_nothing_held_is_alignment_topk(cols):
    from jmac_amd import scoring
    a, b, _, _ = viable_case()
    b = b[:cols]
    terms = scoring.csls_terms(a, b, 10)
    free = torch.zeros(cols, dtype=torch.int64, device="cuda")
    for k in (1, 16):
        idx, val = scoring.alignment_topk_viable(a, b, k, free, csls_k=10, metric="inner", terms=terms)
        widx, wval = scoring.alignment_topk(a, b, k, csls_k=10, metric="inner", terms=terms)
        assert torch.equal(idx, widx) and torch.equal(val, wval)


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def test_max_refills_stops_early_with_a_stable_part():
    from jmac_amd import scoring
    n, d = 300, 32
    gen = torch.Generator().manual_seed(21)
    e2 = torch.randn(n, d, generator=gen)
    e1 = e2[torch.randint(0, 60, (n,), generator=gen)] + 0.6 * torch.randn(n, d, generator=gen)
    e1, e2 = e1.cuda(), e2.cuda()
    m1, v1, stats = scoring.stable_alignment(e1, e2, k=2, csls_k=10, max_refills=0)
    assert stats["complete"] is False and stats["refills"] == 0 and stats["unmatched"] > 0
    m1 = m1.cpu().numpy()
    held = np.nonzero(m1 >= 0)[0]
    assert len(np.unique(m1[held])) == len(held) > 0
    c = _dense(e1, e2)
    assert np.array_equal(v1.cpu().numpy()[held], c[held, m1[held]])
    sub = c[np.ix_(held, m1[held])]                                       # the held pairs among themselves: pair p is (p, p)
    assert stable_ref.blocking_pairs(sub, np.arange(len(held))) == 0


def test_argument_errors():
    from jmac_amd import scoring
    from jmac_amd._lib import JmacError
    e1, e2 = torch.randn(40, 16).cuda(), torch.randn(50, 16).cuda()
    for k in (0, 65, 51):
        with pytest.raises(ValueError):
            scoring.stable_alignment(e1, e2, k=k)
    with pytest.raises(JmacError):
        scoring.stable_alignment(e1.cpu(), e2.cpu())
    with pytest.raises(JmacError):
        scoring.stable_matching(torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, 2), 5)
    with pytest.raises(ValueError):
        scoring.stable_matching(torch.zeros(4, 6, dtype=torch.int64).cuda(), torch.zeros(4, 6).cuda(), 5)       # k > n2
    with pytest.raises(ValueError):
        scoring.alignment_topk_viable(e1, e2, 65, torch.zeros(50, dtype=torch.int64).cuda())


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


def test_model_alignment_stable():
    from jmac_amd import scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    blocks = _blocks(kg1, kg2, graphs)
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(blocks, on_device=True)
        q = np.unique(pairs[:, 0])[:23]
        m1, v1, stats = model.alignment_stable(q, blocks, k=4)
        n1, n2, n3 = model.alignment_stable(torch.from_numpy(q).cuda(), blocks, k=4, emb=(a1, a2))
    model.train()
    assert torch.equal(n1, m1) and torch.equal(n2, v1) and n3 == stats
    a, b = scoring._alignment_operands(a1, a2, "cosine", False)
    t1, t2 = scoring.csls_terms(a, b, 10)
    qd = torch.from_numpy(q).cuda()
    w1, wv, wstats = scoring.stable_alignment(a[qd], b, 4, 10, "inner", False, terms=(t1[qd], t2))
    assert torch.equal(m1, w1) and torch.equal(v1, wv) and stats == wstats
    c = scoring.alignment_sim(a1, a2, "cosine", False, 10).cpu().numpy()[q]
    _check_against_dense(c, m1, v1, stats, want_unmatched=max(0, len(q) - c.shape[1]))
    with pytest.raises(IndexError):
        model.alignment_stable([kg1.num_entity], blocks, emb=(a1, a2))


def test_harness_evaluate_stable_alignment():
    from jmac_amd import harness, scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    precision, stats = harness.evaluate_stable_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=10, k=4)
    assert model.training and stats["complete"] and stats["unmatched"] == 0
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(_blocks(kg1, kg2, graphs), on_device=True)
    model.train()
    p = torch.from_numpy(pairs).cuda()
    c = _dense(a1[p[:, 0]], a2[p[:, 1]])
    w1, _ = stable_ref.stable_dense(c)
    assert abs(precision - 100.0 * float((w1 == np.arange(len(w1))).mean())) < 1e-9
    assert harness.evaluate_stable_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=10, k=4) == (precision, stats)
