"""GPU: the screened alignment ranks (jmac_sim_csls_rank_screened_f32; scoring.alignment_ranks(screen="bf16")) equal the fp32 entry's
ranks bit for bit on every input family of screen_ref.py -- with csls_k = 10 terms (sub_bound_gaps and overflow have 8 and 6 rows:
that many neighbours), without terms and with Sinkhorn terms -- for golds at the top, at the 100th place and in the middle of their
rows and for golds spread over the columns; and the screen really ran: a row's n_rescored is -1 exactly where the numpy
restatement (screen_rank_ref.py) lists more than the kernel's 512 columns, and between 1 (the gold column is always rescored)
and twice the restated length + 8 everywhere else.  (The restatement's list lengths are the kernel's up to the roundings of the
bf16 product: a row within 32 entries of the capacity is asserted on neither side; test_sim_screen_rank_ref.py bounds how many
rows that excuses.)  N just past 8192 is the smallest width that reaches the screened path."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import screen_rank_ref as K
import screen_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = R.families()
KINDS = ("csls", "none", "sinkhorn")


@functools.lru_cache(maxsize=None)
def dev(name, kind):
    """a, b on the device; csls_k and the terms of `kind`; c, the fp32 entries' value as a stored matrix (numpy): 2 s is exact, each
    subtraction rounds once -- csls_value's bits"""
    from jmac_amd import scoring
    f = FAMILIES[name]
    a, b = torch.from_numpy(f["a"]).cuda(), torch.from_numpy(f["b"]).cuda()
    ck, terms = 0, None
    if kind == "csls":
        ck = min(10, a.shape[0])
        terms = scoring.csls_terms(a, b, ck, "inner")
    elif kind == "sinkhorn":
        ck, terms = 1, scoring.sinkhorn_terms(a, b, metric="inner")
        assert bool(torch.isfinite(terms[0]).all()) and bool(torch.isfinite(terms[1]).all())
    s = scoring.sim_matrix(a, b)
    c = (s if terms is None else (2.0 * s - terms[0][:, None]) - terms[1][None, :]).cpu().numpy()
    return a, b, ck, terms, c


@functools.lru_cache(maxsize=None)
def case(name, kind, choice):
    """the gold columns of `choice` (numpy, and on the device) and the unscreened ranks, computed once"""
    from jmac_amd import scoring
    a, b, ck, terms, c = dev(name, kind)
    gold = K.golds(c, choice)
    want = scoring.alignment_ranks(a, b, gold, csls_k=ck, metric="inner", terms=terms)
    return gold, torch.from_numpy(gold).cuda(), want


def _np(t):
    return None if t is None else t.cpu().numpy()


def _entry(a, b, terms, gold, finish, counts=True):
    """the raw entry through ctypes: (rank, n_rescored)"""
    from jmac_amd._lib import check, lib, ptr, stream
    n1, d = a.shape
    n2 = b.shape[0]
    rank = torch.full((n1,), -7, dtype=torch.int32, device="cuda")
    nres = torch.full((n1,), -7, dtype=torch.int32, device="cuda") if counts else None
    r1, r2 = terms if terms is not None else (None, None)
    ws_bytes = int(lib().jmac_sim_csls_rank_screened_workspace_bytes(n1, n2, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    check(lib().jmac_sim_csls_rank_screened_f32(ptr(a), d, ptr(b), d, n1, n2, d, ptr(r1), ptr(r2), ptr(gold), ptr(rank), ptr(nres),
                                                ctypes.c_int32(finish), ptr(ws), ws_bytes, stream()), "jmac_sim_csls_rank_screened_f32")
    return rank, nres


@pytest.mark.parametrize("choice", K.CHOICES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_screened_ranks_equal_the_fp32_entry(name, kind, choice):
    from jmac_amd import scoring
    a, b, ck, terms, c = dev(name, kind)
    gold, gold_d, want = case(name, kind, choice)
    # the fp32 entry is the stored matrix's count
    assert np.array_equal(want.cpu().numpy(), 1 + K.before(c, c[np.arange(len(c)), gold], gold).sum(1))
    got, st = scoring.alignment_ranks(a, b, gold_d, csls_k=ck, metric="inner", terms=terms, screen="bf16", return_stats=True)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert st["screened"] and st["rows"] == len(c)
    rank, nres = _entry(a, b, terms, gold_d, finish=1)
    assert torch.equal(rank, want)
    assert torch.equal(nres.cpu(), st["n_rescored"])                     # the lists do not depend on who finishes the row
    assert torch.equal(_entry(a, b, terms, gold_d, finish=1, counts=False)[0], want)      # n_rescored may be NULL
    if kind == "csls":                                                   # the terms computed inside, both products screened
        assert torch.equal(scoring.alignment_ranks(a, b, gold_d, csls_k=ck, metric="inner", screen="bf16"), want)


@pytest.mark.parametrize("choice", ["best", "r100", "median"])
@pytest.mark.parametrize("kind", ["csls", "none"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_counts_against_the_restatement(name, kind, choice):
    from jmac_amd import scoring
    a, b, ck, terms, c = dev(name, kind)
    gold, gold_d, want = case(name, kind, choice)
    ref = K.screen_rank(FAMILIES[name]["a"], FAMILIES[name]["b"], gold, *(map(_np, terms) if terms is not None else (None, None)), c=c)
    assert np.array_equal(ref["rank"], want.cpu().numpy())
    _, st = scoring.alignment_ranks(a, b, gold_d, csls_k=ck, metric="inner", terms=terms, screen="bf16", return_stats=True)
    n = st["n_rescored"].numpy()
    near = K.in_band(ref)
    over, fit = ref["overflow"] & ~near, ~ref["overflow"] & ~near
    print("%s %s %s: rescored per row mean %.1f max %d, overflow rows %d; restated list mean %.1f max %d, overflow rows %d, band %d"
          % (name, kind, choice, n[n >= 0].mean() if (n >= 0).any() else 0, n.max(), (n == -1).sum(),
             ref["list_len"][fit].mean() if fit.any() else 0, ref["list_len"][fit].max() if fit.any() else 0, ref["overflow"].sum(), near.sum()))
    assert near.sum() <= 0.05 * len(n)
    assert (n[over] == -1).all()
    assert (n[fit] >= 1).all() and (n[fit] <= 2 * ref["list_len"][fit] + 8).all()
    assert st["screened"]
    if not near.any():
        assert st["overflow_rows"] == int(ref["overflow"].sum())
    must = K.must_overflow(c, gold)
    assert (n[must] == -1).all()


@pytest.mark.parametrize("name,kind,choice", [("two_row_tiles", "csls", "spread"), ("unnormalised", "none", "median"),
                                              ("overflow", "csls", "spread"), ("random_unit", "none", "r100")])
def test_finish_zero_leaves_the_overflowing_rows(name, kind, choice):
    """finish = 0: an overflowing row comes back as rank 0, n_rescored -1; every other row is final already"""
    a, b, ck, terms, c = dev(name, kind)
    gold, gold_d, want = case(name, kind, choice)
    rank, nres = _entry(a, b, terms, gold_d, finish=0)
    over = nres == -1
    assert bool((rank[over] == 0).all()) and bool((rank[~over] >= 1).all()) and bool((nres[~over] >= 1).all())
    assert torch.equal(rank[~over], want[~over])
    full, nfull = _entry(a, b, terms, gold_d, finish=1)
    assert torch.equal(nfull, nres) and torch.equal(full, want)
    if name == "overflow":
        assert bool(over.all())
    if name == "random_unit":
        assert not bool(over.any())
    if name == "two_row_tiles":                                          # a mixed call: some rows of either kind
        assert bool(over.any()) and not bool(over.all())


def test_ties():
    """every column of the one-row-repeated family ties: the rank is G + 1; a gold among the 12 exact copies of base 0 of
    near_duplicates is ranked behind the copies at lower columns only"""
    from jmac_amd import scoring
    for kind in ("csls", "none"):
        a, b, ck, terms, c = dev("overflow", kind)
        gold = K.golds(c, "spread")
        got, st = scoring.alignment_ranks(a, b, torch.from_numpy(gold).cuda(), csls_k=ck, metric="inner", terms=terms, screen="bf16",
                                          return_stats=True)
        assert np.array_equal(got.cpu().numpy(), gold + 1) and st["overflow_rows"] == len(gold)
    f = FAMILIES["near_duplicates"]
    copies = np.flatnonzero((f["b"] == f["a"][0]).all(1))                # base 0 is row 0 of a
    assert len(copies) == 12
    a, b, ck, terms, c = dev("near_duplicates", "none")
    assert len(np.unique(c[0, copies])) == 1                             # exact ties in the fp32 product
    for pick in (0, 5, 11):
        gold = K.golds(c, "best")
        gold[0] = copies[pick]
        want = scoring.alignment_ranks(a, b, gold, csls_k=0, metric="inner")
        got = scoring.alignment_ranks(a, b, gold, csls_k=0, metric="inner", screen="bf16")
        assert torch.equal(got, want)
        assert int(got[0]) == int(K.before(c[:1], c[0, gold[:1]], gold[:1]).sum()) + 1 >= 1 + pick


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_best_gold_ranks_first(name, kind):
    """the gold column never counts against itself"""
    from jmac_amd import scoring
    a, b, ck, terms, c = dev(name, kind)
    gold, gold_d, _ = case(name, kind, "best")
    assert bool((scoring.alignment_ranks(a, b, gold_d, csls_k=ck, metric="inner", terms=terms, screen="bf16") == 1).all())


def test_narrow_exit_takes_the_fp32_code():
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(3)
    a = torch.nn.functional.normalize(torch.randn(40, 16, generator=gen), dim=1).cuda()
    b = torch.nn.functional.normalize(torch.randn(8191, 16, generator=gen), dim=1).cuda()
    gold = ((37 * torch.arange(40) + 5) % 8191).to(torch.int32).cuda()
    for ck in (10, 0):
        want = scoring.alignment_ranks(a, b, gold, csls_k=ck, metric="inner")
        got, st = scoring.alignment_ranks(a, b, gold, csls_k=ck, metric="inner", screen="bf16", return_stats=True)
        assert torch.equal(got, want)
        assert (st["n_rescored"] == -2).all() and not st["screened"] and st["overflow_rows"] == 0
    rank, nres = _entry(a, b, None, gold, finish=0)
    assert torch.equal(rank, want) and bool((nres == -2).all())


def test_two_calls_return_identical_bits():
    from jmac_amd import scoring
    a, b, ck, terms, c = dev("two_row_tiles", "csls")
    for choice in ("r100", "spread"):
        gold_d = case("two_row_tiles", "csls", choice)[1]
        one = scoring.alignment_ranks(a, b, gold_d, csls_k=ck, metric="inner", terms=terms, screen="bf16", return_stats=True)
        two = scoring.alignment_ranks(a, b, gold_d, csls_k=ck, metric="inner", terms=terms, screen="bf16", return_stats=True)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1]["n_rescored"], two[1]["n_rescored"])
        r1, n1 = _entry(a, b, terms, gold_d, finish=1)
        r2, n2 = _entry(a, b, terms, gold_d, finish=1)
        assert torch.equal(r1, r2) and torch.equal(n1, n2)


def test_alignment_test_passes_the_screen_on():
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(5)
    tab = torch.nn.functional.normalize(torch.randn(8300, 128, generator=gen), dim=1)
    q = torch.nn.functional.normalize(tab + 0.03 * torch.randn(8300, 128, generator=gen), dim=1)
    # every tenth gold is a random column: at this row length about 600 columns lie within the bound of a median score
    q[::10] = torch.nn.functional.normalize(torch.randn(830, 128, generator=gen), dim=1)
    q, tab = q.cuda(), tab.cuda()
    for ck in (10, 0):
        want = scoring.alignment_test(q, tab, (1, 5, 10), "cosine", csls_k=ck, matrix_free=True)
        assert scoring.alignment_test(q, tab, (1, 5, 10), "cosine", csls_k=ck, matrix_free=True, screen="bf16") == want
    gold = torch.arange(8300, dtype=torch.int32, device="cuda")
    rank, st = scoring.alignment_ranks(q, tab, gold, screen="bf16", return_stats=True)
    print("8300 x 8300 x 128, every tenth gold random: %s" % {k: v for k, v in st.items() if k != "n_rescored"})
    assert torch.equal(rank, scoring.alignment_ranks(q, tab, gold)) and st["screened"] and 0 < st["overflow_rows"] < 8300


def test_harness_evaluate_alignment_passes_the_screen_on():
    """the mini data set is narrow: the plumbing only"""
    from jmac_amd import data, harness
    from jmac_amd.model import JMAC
    torch.manual_seed(0)
    kgs, s_train, s_test, n_ent = data.load_dbp5l(os.path.join(GOLD, "dbp5l_mini"), "ja")
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, dropout=0.0)
    name_emb = np.random.default_rng(0).standard_normal((n_ent, 24)).astype(np.float32)
    model = JMAC(args, name_emb, sum(kg.num_relation for kg in kgs.values()), n_ent).cuda()
    (l1, l2), pairs = sorted(s_test.items())[0]
    kg1, kg2 = kgs[l1], kgs[l2]
    pairs = np.asarray(pairs, dtype=np.int64)
    graphs = tuple((torch.from_numpy(kg.edge_index).cuda(), torch.from_numpy(kg.edge_type).cuda()) for kg in (kg1, kg2))
    for ck in (10, 0):
        want = harness.evaluate_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=ck)
        assert harness.evaluate_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=ck, screen="bf16") == want
    want = harness.evaluate_sinkhorn_alignment(model, kg1, kg2, pairs, graphs, args, iters=3)
    assert harness.evaluate_sinkhorn_alignment(model, kg1, kg2, pairs, graphs, args, iters=3, screen="bf16") == want
    with pytest.raises(ValueError):
        harness.evaluate_alignment(model, kg1, kg2, pairs, graphs, args, matrix_free=False, screen="bf16")


def test_errors():
    from jmac_amd import scoring
    a, b, ck, terms, c = dev("random_unit", "none")
    gold = case("random_unit", "none", "spread")[1]
    with pytest.raises(ValueError):
        scoring.alignment_ranks(a, b, gold, csls_k=0, metric="manhattan", screen="bf16")
    with pytest.raises(ValueError):
        scoring.alignment_ranks(a, b, gold, csls_k=0, metric="inner", return_stats=True)
    with pytest.raises(ValueError):
        scoring.alignment_ranks(a, b, gold, csls_k=0, metric="inner", screen="fp8")
    with pytest.raises(ValueError):
        scoring.alignment_test(a, a, matrix_free=False, screen="bf16")
    with pytest.raises(ValueError):
        scoring.alignment_test(a, a, metric="manhattan", matrix_free=True, screen="bf16")
    with pytest.raises(NotImplementedError):
        scoring.alignment_ranks(a, b, gold, csls_k=0, metric="euclidean", screen="bf16")
