"""GPU: the MIDDLE exit of the shared top-k selection (jmac_amd/csrc/topk_select.h), once per score source.

A row of a fused top-k takes one of three exits: its candidate list fits (sort the list); the list overflows but the bins at and
above the one that holds the k-th best fit the LDS list (two recomputing passes, then the sort); even those overflow (arg-max
rounds).  The first and the last are reached by the tests of the three callers; the inputs here are built for the middle one,
and every test of it ASSERTS from a materialised matrix that its rows take it, per row:
  A  more than 1024 - k of the columns past the sample (the first 2048 columns at N = 8192) reach the row's k-th best sample
     score, so the list of 1024 overflows;
  B  the 12-bit bin of the row's k-th best score holds, together with the bins above it, at most 1024 elements.
test_narrow_fused_seam runs every source on both sides of the driver's one narrow / fused decision.  The last test pins the byte
counts of the workspace functions (it needs no GPU)."""
import numpy as np
import pytest
import torch

import linkpred_ref

N, NS, CAP = 8192, 2048, 1024


def _bins(x):
    """The selection's histogram bin of every score: the 12 leading bits of its order-preserving key."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = np.where(x == 0, np.uint32(0), x.view(np.uint32))
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return (key >> np.uint32(20)).astype(np.int64)


def _assert_middle_exit(score, k, live=None):
    """Preconditions A and B for every row of ``score`` [L, N] (larger is better; ``live``: the columns that take part)."""
    score = np.asarray(score, dtype=np.float32)
    live = np.ones(score.shape, dtype=bool) if live is None else live
    bins = _bins(score)
    for i in range(score.shape[0]):
        s, ok = score[i], live[i]
        tau = np.sort(s[:NS][ok[:NS]])[::-1][k - 1]
        passing = int((s[NS:][ok[NS:]] >= tau).sum())
        kth = np.argsort(-s[ok], kind="stable")[k - 1]
        collected = int((bins[i][ok] >= bins[i][ok][kth]).sum())
        print("row %d: %d columns past the sample reach tau (list: %d), %d elements in the bins >= b*" % (i, passing, CAP - k, collected))
        assert passing > CAP - k                         # A: the list overflows
        assert k <= collected <= CAP                     # B: the two-pass selection fits


@pytest.fixture(scope="module")
def operands():
    """b: unit rows whose first coordinate is <= 0 on the sample columns, linspace(0.26, 0.99) on columns 2048 .. 3547; a[i] =
    s_i e_0: the scores are exactly s_i b[:, 0] whatever the contraction order."""
    gen = torch.Generator().manual_seed(5)
    b = torch.randn(N, 16, generator=gen)
    b = b / b.norm(dim=1, keepdim=True)
    b[:NS, 0] = -b[:NS, 0].abs()
    first = torch.linspace(0.26, 0.99, 1500)
    rest = b[NS:NS + 1500, 1:]
    b[NS:NS + 1500, 1:] = rest / rest.norm(dim=1, keepdim=True) * (1 - first * first).sqrt()[:, None]
    b[NS:NS + 1500, 0] = first
    a = torch.zeros(16, 16)
    a[:, 0] = torch.linspace(0.5, 1.0, 16)
    return a.cuda(), b.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 64])
def test_sim_topk_two_pass_recompute(operands, k):
    from jmac_amd import scoring
    a, b = operands
    s = scoring.sim_matrix(a, b)
    _assert_middle_exit(s.cpu().numpy(), k)
    rval, ridx = scoring.row_topk(s, k)
    idx, val = scoring.sim_topk(a, b, k, return_values=True)
    assert torch.equal(idx, ridx) and torch.equal(val.view(torch.int32), rval.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 64])
def test_alignment_topk_rescored_two_pass_recompute(operands, k):
    from jmac_amd import scoring
    a, b = operands
    c = scoring.csls_sim(scoring.sim_matrix(a, b), 10)
    _assert_middle_exit(c.cpu().numpy(), k)
    rval, ridx = scoring.row_topk(c, k)
    idx, val = scoring.alignment_topk(a, b, k, csls_k=10, metric="inner")
    assert torch.equal(idx, ridx) and torch.equal(val.view(torch.int32), rval.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True])
def test_linkpred_topk_two_pass_recompute_with_listed_tails(bf16):
    """One layer of integer tables: every distance is an exact integer in fp32, in bf16 tables and in float64.  Candidates
    2048 .. 3547 lie at distance 1 .. 1500 of the zero query (one non-zero coordinate each; bf16 rounds the larger ones to
    exact ties), all the others at 800; the second query's list covers some of its nearest candidates."""
    from jmac_amd import scoring
    from jmac_amd.sampling import TrueTailIndex
    d, k = 8, 10
    tab = torch.full((N, d), 100.0)
    tab[NS:NS + 1500] = 0.0
    tab[torch.arange(NS, NS + 1500), torch.arange(1500) % d] = torch.arange(1, 1501, dtype=torch.float32)
    rel = torch.full((1, d), -100.0)                         # E[h] + R[0] = 0 for the far entities h = 0, 1
    h, r = np.array([0, 1]), np.array([0, 0])
    tt = {(1, 0): np.array([5, NS, NS + 1, NS + 3, NS + 12, NS + 700, 4000])}
    comp, rels = [tab.cuda()], [rel.cuda()]
    d64 = linkpred_ref.dist64([tab.numpy()], [rel.numpy()], h, r, bf16=bf16)
    listed = linkpred_ref.listed_mask(h, r, tt, N)
    assert (d64 == np.round(d64)).all() and d64.max() < 2 ** 24
    _assert_middle_exit(-d64, k, ~listed)
    ridx, rval = linkpred_ref.topk(d64, k, listed)
    idx, val = scoring.linkpred_topk(comp, rels, h, r, k, index=TrueTailIndex.from_dict(tt, "cuda"),
                                     table_dtype=torch.bfloat16 if bf16 else torch.float32)
    assert (idx.cpu().numpy() == ridx).all() and (val.cpu().numpy() == rval).all()
    assert ridx[0, 0] == NS and ridx[1, 0] == NS + 2


@pytest.fixture(scope="module")
def seam_rows():
    gen = torch.Generator().manual_seed(11)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 16, generator=gen), dim=1)       # noqa: E731
    return unit(10).cuda(), unit(N).cuda(), torch.randn(3, 16, generator=gen).cuda()


def _same(got, want):
    """(idx, val) pairs, bit for bit"""
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N - 1, N])
def test_narrow_fused_seam(seam_rows, n):
    """N = 8191 stores the scores and runs the row pass, N = 8192 is the first fused shape (k = 64 <= 64; k = 65 is narrow again):
    every source's fused form against the stored path, bit for bit, on both sides of the decision.  Five query rows; the CSLS terms
    (csls_k = 10 needs ten rows) are those of ten rows, of which the queries are the first five."""
    from jmac_amd import scoring
    from jmac_amd.sampling import TrueTailIndex
    a10, b, rel = seam_rows[0], seam_rows[1][:n].contiguous(), seam_rows[2]
    a = a10[:5].contiguous()
    k = 64
    for kk in [k] + ([k + 1] if n == N else []):
        rval, ridx = scoring.row_topk(scoring.sim_matrix(a, b), kk)
        assert _same(scoring.sim_topk(a, b, kk, return_values=True), (ridx, rval)), kk
    for metric in ("inner", "manhattan"):
        rval, ridx = scoring.row_topk(scoring.alignment_sim(a10, b, metric, csls_k=10)[:5], k)
        r1, r2 = scoring.csls_terms(a10, b, 10, metric)
        got = scoring.alignment_topk(a, b, k, csls_k=10, metric=metric, terms=(r1[:5], r2))
        assert _same(got, (ridx, rval)), metric
        free = torch.zeros(n, dtype=torch.int64, device="cuda")
        assert _same(scoring.alignment_topk_viable(a, b, k, free, csls_k=10, metric=metric, terms=(r1[:5], r2)), got), metric
    # link prediction: one fp32 layer, whose fused distance has the stored l1_scores' bits; the lists reach into both column ranges
    h, r = np.array([0, 7, n - 1, 4000, 7]), np.array([0, 1, 2, 0, 2])
    tt = {(0, 0): np.array([0, 3, NS - 1, NS, n - 1]), (7, 2): np.array([5000]), (9, 1): np.array([1])}
    dist = scoring.linkpred_dist([b], [rel], h, r).cpu().numpy()
    ridx, rval = linkpred_ref.topk(dist, k, linkpred_ref.listed_mask(h, r, tt, n))
    idx, val = scoring.linkpred_topk([b], [rel], h, r, k, index=TrueTailIndex.from_dict(tt, "cuda"))
    assert (idx.cpu().numpy() == ridx).all()
    assert (val.cpu().numpy().view(np.int32) == rval.astype(np.float32).view(np.int32)).all()


def test_topk_workspace_sizes_are_unchanged():
    """The byte counts the library returned before the candidate-list layout became one struct (L / B, N, [d, layers,] k)."""
    from jmac_amd import _lib
    L = _lib.lib()
    sim = {(100, 4000, 10): 1600256, (3, 8191, 64): 98560, (50, 10000, 65): 2000384,                  # narrow (N < 8192 or k > 64)
           (16, 8192, 10): 264192, (3000, 30000, 64): 56844288, (1, 100000, 1): 43008}                # fused
    for shape, want in sim.items():
        assert L.jmac_sim_topk_workspace_bytes(*shape) == want, shape
        assert L.jmac_sim_csls_topk_workspace_bytes(*shape) == want, shape
        rows, n, k = shape
        assert L.jmac_l1_csls_topk_workspace_bytes(rows, n, 32, k) == want, shape                        # the sim value for any d > 0
        assert L.jmac_l1_csls_topk_workspace_bytes(rows, n, 0, k) == 0, shape
    link = {(9, 70, 7, 3, 10): 4352, (40, 4000, 64, 1, 64): 651008,                                    # narrow
            (70, 9000, 30, 2, 10): 1171968, (96, 20000, 64, 1, 64): 1648128, (2, 8192, 8, 1, 10): 34304,
            (5, 8192, 13, 2, 3): 83968}                                                                # d % 4 != 0, fused
    for shape, want in link.items():
        assert L.jmac_linkpred_topk_workspace_bytes(*shape) == want, shape
