"""GPU: the model's predictions -- scoring.linkpred_topk / jmac_linkpred_topk_*: the k nearest candidate tails of (h, r) that
the known-tail index does not list, without the [B, N] distance matrix.

Two kinds of check.  EXACT, against the rank kernel (same distances bit for bit): the j-th prediction ranks j + 1, order, tie
rule, exclusion, repeatability.  Against FLOAT64 (tests/linkpred_ref.py) with a derived tolerance: the kernel's distance is a
sequential fp32 sum of m = n_layers * d terms, whose error is below (m + 2) 2^-24 max dist (one rounding per subtraction, one per
addition, one for the query row); `bound` doubles that, so two candidates whose float64 distances differ by more than `bound`
cannot change order in fp32.  A position j of a row is DECIDED when the float64 gap between the j-th and the (j + 1)-th
candidate exceeds `bound`; at a decided position the first j + 1 predictions must be the float64 first j + 1 as a set, which
pins the index itself wherever position j - 1 is decided too (and at j = 0): an undecided pair (j - 1, j) may legitimately
swap in fp32, so `idx[b, j]` alone is not determined there.  Both shares are printed -- decided positions, and positions whose
index is asserted; where a test requires a share s of decided positions it requires 2 s - 1 of asserted ones (a position drops
out only if it or its predecessor is undecided).  Both shares depend on the float64 reference alone, not on the kernel."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import linkpred_ref
from conftest import GOLDEN


def _index(tt):
    from jmac_amd.sampling import TrueTailIndex
    return TrueTailIndex.from_dict(tt, "cuda") if tt else None


def _topk(comp, rel, h, r, k, tt, **kw):
    from jmac_amd import scoring
    return scoring.linkpred_topk(comp, rel, h, r, k, index=_index(tt), **kw)


def check_exact(comp, rel, h, r, k, tt, pred_head=False, dt=torch.float32):
    """The contract, without a tolerance; returns (idx, val) as numpy."""
    from jmac_amd import scoring
    kw = dict(pred_head=pred_head, table_dtype=dt)
    index = _index(tt)
    idx_t, val_t = scoring.linkpred_topk(comp, rel, h, r, k, index=index, **kw)
    idx2, val2 = scoring.linkpred_topk(comp, rel, h, r, k, index=index, **kw)
    assert idx_t.dtype == torch.int64 and val_t.dtype == torch.float32 and idx_t.shape == val_t.shape == (len(h), k)
    assert torch.equal(idx_t, idx2) and torch.equal(val_t.view(torch.int32), val2.view(torch.int32))     # identical bits
    idx, val = idx_t.cpu().numpy(), val_t.cpu().numpy()
    N = comp[0].shape[0]
    valid = idx >= 0
    assert ((idx < N) & (np.isinf(val) == ~valid)).all() and (val[~valid] > 0).all()
    assert (valid[:, :-1] | ~valid[:, 1:]).all()                             # padding only at the end of a row
    assert (val[:, 1:] >= val[:, :-1]).all()                                 # ascending distance
    tie = (val[:, 1:] == val[:, :-1]) & valid[:, 1:]
    assert (idx[:, 1:][tie] > idx[:, :-1][tie]).all()                        # equal distances: lower index first
    for b in range(len(h)):
        lst = np.asarray(tt.get((int(h[b]), int(r[b])), []) if tt else [], dtype=np.int64)
        got = idx[b][valid[b]]
        assert len(set(got.tolist())) == len(got) and not np.isin(got, lst).any()      # distinct, none listed
        assert valid[b].sum() == min(k, N - len(np.unique(lst[(lst >= 0) & (lst < N)])))
    for j in range(k):                                                       # EVERY prediction: the j-th ranks j + 1
        gold = np.where(valid[:, j], idx[:, j], 0)
        rk = scoring.linkpred_ranks(comp, rel, h, r, gold, index=index, **kw).cpu().numpy()
        assert (rk[valid[:, j]] == j + 1).all(), (j, rk[valid[:, j]][:10])
    return idx, val


def check_float64(comp, rel, h, r, k, tt, idx, val, pred_head=False, bf16=False, min_decided=None):
    N, d = comp[0].shape
    d64 = linkpred_ref.dist64([c.cpu().numpy() for c in comp], [x.cpu().numpy() for x in rel], h, r, pred_head, bf16=bf16)
    listed = linkpred_ref.listed_mask(h, r, tt or {}, N)
    ridx, rval = linkpred_ref.topk(d64, k + 1, listed)
    m = len(comp) * d
    bound = 2 * (m + 2) * 2.0 ** -24 * np.abs(d64).max()
    valid = idx >= 0
    assert (valid == (ridx[:, :k] >= 0)).all()
    rows = np.arange(len(h))[:, None]
    got64 = np.where(valid, d64[rows, np.where(valid, idx, 0)], np.inf)
    err = np.abs(np.where(valid, val, 0.0) - np.where(valid, got64, 0.0)).max()
    # (ii) completeness: nothing unlisted and not returned is nearer than the last prediction by more than the bound
    rest = np.where(listed, np.inf, d64)
    for b in range(len(h)):
        rest[b, idx[b][valid[b]]] = np.inf
    last = np.where(valid[:, -1], got64[:, -1], np.inf)
    slack = rest.min(1)[np.isfinite(last)] - last[np.isfinite(last)]
    # (iii) decided positions
    with np.errstate(invalid="ignore"):                                      # inf - inf past the end of a short row
        gap = rval[:, 1:] - rval[:, :-1]                                     # [B, k]: position j to position j + 1
        decided = (gap > bound) & valid
    pinned = decided.copy()                                                  # positions whose INDEX is asserted: j and j - 1 decided
    pinned[:, 1:] &= decided[:, :-1]
    wrong_sets = wrong_idx = 0
    for b in range(len(h)):
        for j in np.flatnonzero(decided[b]):
            wrong_sets += set(idx[b, :j + 1].tolist()) != set(ridx[b, :j + 1].tolist())
        wrong_idx += int((idx[b][pinned[b]] != ridx[b, :k][pinned[b]]).sum())
    share, share_pinned = decided[valid].mean(), pinned[valid].mean()
    print("float64: |val - d64| max %.3g (allowed %.3g), bound %.3g at scale %.4g, completeness slack min %.3g, decided %.4f and "
          "index asserted %.4f of %d" % (err, 1e-4 * np.abs(d64).max(), bound, np.abs(d64).max(), slack.min() if len(slack) else np.inf,
                                       share, share_pinned, valid.sum()))
    assert err <= 1e-4 * np.abs(d64).max()                                   # (i) the project's tolerance
    assert len(slack) == 0 or slack.min() >= -bound                          # (ii)
    assert wrong_sets == 0 and wrong_idx == 0                                # (iii)
    if min_decided is not None:
        # a position's index is asserted unless it or its predecessor is undecided: at least 1 - 2 (1 - min_decided) of them
        assert share >= min_decided and share_pinned >= 2 * min_decided - 1
    return share


def _tables(N, d, nl, nrel, seed, integer=False):
    gen = torch.Generator().manual_seed(seed)
    if integer:
        mk = lambda n: torch.randint(-2, 3, (n, d), generator=gen).float().cuda()
    else:
        mk = lambda n: torch.randn(n, d, generator=gen).cuda()
    return [mk(N) for _ in range(nl)], [mk(nrel) for _ in range(nl)]


def _lists(h, r, N, rng, lo=0, hi=40, absent=0.2):
    tt = {}
    for hb, rb in zip(h, r):
        if (int(hb), int(rb)) not in tt and rng.random() >= absent:
            n = int(rng.integers(lo, hi))
            if n:
                tt[(int(hb), int(rb))] = np.sort(rng.choice(N, min(n, N), replace=False))
    return tt


@pytest.mark.parametrize("N,d,nl,B,k,bf16,pred_head", [
    (70, 7, 3, 9, 10, False, False),             # rows of 28 bytes, three layers
    (300, 48, 2, 37, 1, False, True),
    (4000, 300, 2, 130, 10, False, False),       # the matrix path (N < 8192)
    (4000, 64, 1, 40, 64, True, False),
    (9000, 30, 2, 70, 10, False, True),          # the fused path, rows of 120 bytes (scalar loads)
    (20000, 64, 1, 96, 10, False, False),
    (20000, 64, 1, 96, 64, True, True),
    (200000, 64, 1, 96, 10, False, False),
    (200000, 64, 1, 96, 1, True, False),
])
def test_topk_contract_filtered_and_raw(N, d, nl, B, k, bf16, pred_head):
    rng = np.random.default_rng(N + d + k)
    comp, rel = _tables(N, d, nl, 11, N + k)
    h, r = rng.integers(0, N, B), rng.integers(0, 11, B)
    tt = _lists(h, r, N, rng)
    dt = torch.bfloat16 if bf16 else torch.float32
    for lists in (tt, None):
        idx, val = check_exact(comp, rel, h, r, k, lists, pred_head, dt)
        check_float64(comp, rel, h, r, k, lists, idx, val, pred_head, bf16)


def _ja():
    from jmac_amd import data
    kgs, _, _, _ = data.kgs_from_arrays(data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz")), "ja")
    return kgs["ja"]


@pytest.mark.parametrize("bf16", [False, True])
def test_topk_against_float64_on_the_seeded_ja_case(bf16):
    """N = 11 805, d = 300, two layers of standard-normal tables (seed 1234), 256 queries of the real ja validation split with
    ja's real known-tail lists, k = 10; then 256 random queries, raw.  At least 90 % of the positions must be decided (the
    float64 distances alone decide 94-95 % at this bound, 0.069 at distance scale 960, and pin the index of 90 %)."""
    ja = _ja()
    N, d = ja.num_entity, 300
    assert N == 11805
    gen = torch.Generator().manual_seed(1234)
    comp = [torch.randn(N, d, generator=gen).cuda() for _ in range(2)]
    rel = [torch.randn(ja.num_relation, d, generator=gen).cuda() for _ in range(2)]
    rng = np.random.default_rng(1234)
    q = ja.val_data[rng.choice(len(ja.val_data), 256, replace=False)]
    dt = torch.bfloat16 if bf16 else torch.float32
    idx, val = check_exact(comp, rel, q[:, 0], q[:, 1], 10, ja.true_tail, False, dt)
    check_float64(comp, rel, q[:, 0], q[:, 1], 10, ja.true_tail, idx, val, False, bf16, min_decided=0.90)
    h, r = rng.integers(0, N, 256), rng.integers(0, ja.num_relation, 256)
    idx, val = check_exact(comp, rel, h, r, 10, None, False, dt)
    check_float64(comp, rel, h, r, 10, None, idx, val, False, bf16, min_decided=0.90)


@pytest.mark.parametrize("N", [300, 9000])
def test_topk_exact_ties_equal_float64_stable_topk(N):
    """Integer tables in {-2, ..., 2}: every distance is an exact fp32 integer, thousands of ties: the predictions ARE the
    float64 stable top-k, index for index."""
    rng = np.random.default_rng(N)
    comp, rel = _tables(N, 12, 2, 7, N, integer=True)
    h, r = rng.integers(0, N, 64), rng.integers(0, 7, 64)
    tt = _lists(h, r, N, rng, hi=60)
    for lists in (tt, None):
        for k in (10, 64):
            idx, val = check_exact(comp, rel, h, r, k, lists)
            d64 = linkpred_ref.dist64([c.cpu().numpy() for c in comp], [x.cpu().numpy() for x in rel], h, r)
            ridx, rval = linkpred_ref.topk(d64, k, linkpred_ref.listed_mask(h, r, lists or {}, N))
            assert (idx == ridx).all() and (val == rval).all()
            assert (rval[:, 1:] == rval[:, :-1]).sum() > 100


def test_topk_overflowing_rows_are_recomputed_exactly():
    """Rows whose candidate list overflows take the recompute path: a constant candidate table (every distance of a row
    equal: the answer is 0 .. k-1 minus the listed ones) and a row tied across 5 000 candidates."""
    N, d, k = 9000, 16, 10
    rng = np.random.default_rng(9)
    rel = [torch.randn(5, d, generator=torch.Generator().manual_seed(2)).cuda()]
    comp = [torch.ones(N, d).cuda()]
    h, r = np.array([0, 17, 8999, 4000]), np.array([0, 1, 2, 3])
    tt = {(0, 0): np.array([0, 1, 5, 8000]), (17, 1): np.array([3]), (4000, 3): np.arange(0, 40, 2)}
    idx, val = check_exact(comp, rel, h, r, k, tt)
    for b in range(4):
        lst = tt.get((int(h[b]), int(r[b])), np.zeros(0, dtype=np.int64))
        assert idx[b].tolist() == [n for n in range(60) if n not in set(lst.tolist())][:k]
        assert (val[b] == val[b, 0]).all()
    idx, _ = check_exact(comp, rel, h, r, k, None)
    assert (idx == np.arange(k)).all()
    # 5 000 candidates at exactly the same (smallest) distance: rows 1000 .. 5999 are zero, the others far away
    for start in (1000, 3000):
        tab = torch.randn(N, d, generator=torch.Generator().manual_seed(3)) + 10.0
        tab[start:start + 5000] = 0.0
        comp = [tab.cuda()]
        h = np.array([start, start + 4999, start + 77])
        r = np.array([0, 1, 2])
        tt = {(start, 0): np.array([start, start + 1, start + 3, 12]), (start + 77, 2): np.arange(start, start + 5000)}
        idx, val = check_exact(comp, rel, h, r, k, tt)
        assert idx[0].tolist() == [start + n for n in range(14) if n not in (0, 1, 3)][:k]
        assert idx[1].tolist() == list(range(start, start + k)) and (val[:2] == val[:2, :1]).all()
        assert not ((idx[2] >= start) & (idx[2] < start + 5000)).any()        # the whole tie is listed: the far ones remain
        check_float64(comp, rel, h, r, k, tt, idx, val)


def test_topk_short_rows_are_padded():
    N, d, k = 20, 8, 10
    comp, rel = _tables(N, d, 2, 3, 5)
    listed = np.arange(15) + 2
    tt = {(4, 1): listed, (5, 1): np.arange(N)}
    h, r = np.array([4, 5, 6]), np.array([1, 1, 1])
    idx, val = check_exact(comp, rel, h, r, k, tt)
    assert (idx[0, :5] >= 0).all() and (idx[0, 5:] == -1).all() and np.isposinf(val[0, 5:]).all() and np.isfinite(val[0, :5]).all()
    assert sorted(idx[0, :5].tolist()) == [0, 1, 17, 18, 19]
    assert (idx[1] == -1).all() and (idx[2] >= 0).all()
    check_float64(comp, rel, h, r, k, tt, idx, val)


def test_topk_refuses_bad_k_and_cpu_tensors():
    from jmac_amd import _lib, scoring
    comp, rel = _tables(50, 8, 1, 3, 1)
    for k in (0, 65, 51):
        with pytest.raises(ValueError):
            scoring.linkpred_topk(comp, rel, [1], [1], k)
    with pytest.raises(_lib.JmacError):
        scoring.linkpred_topk([c.cpu() for c in comp], [x.cpu() for x in rel], [1], [1], 3)


def test_whole_ja_validation_split_in_one_call():
    """8 633 queries x 11 805 candidates, d = 300, two layers, k = 10, ONE call: the peak memory above the tables stays under
    half of the B x N fp32 matrix, and Hits@10 read off the predictions is the evaluator's.
    Subset rule for Hits@10: the raw predictions (index=None) hold the gold iff its raw rank is <= 10; the evaluator's filtered
    rank exempts the gold and skips every other known tail.  On the queries whose raw top 10 holds no known tail other than the
    gold, the two agree query by query: a gold inside has filtered rank <= raw rank <= 10, and a gold outside has ten unlisted
    candidates before it."""
    from jmac_amd import scoring
    from jmac_amd.sampling import TrueTailIndex
    ja = _ja()
    val = ja.val_data
    B, N = len(val), ja.num_entity
    gen = torch.Generator().manual_seed(1234)
    comp = [torch.randn(N, 300, generator=gen).cuda() for _ in range(2)]
    rel = [torch.randn(ja.num_relation, 300, generator=gen).cuda() for _ in range(2)]
    vh, vr, vt = (torch.from_numpy(val[::2, c].copy()).cuda() for c in range(3))
    for c, x in zip(comp, rel):                     # a planted signal, so that Hits@10 is not vacuous: t ~ h + r on half the split
        c[vt] = (c[vh] + x[vr]) / 2 + 0.3 * c[vt]
    index = TrueTailIndex.from_dict(ja.true_tail, "cuda")
    h, r = torch.from_numpy(val[:, 0]).cuda(), torch.from_numpy(val[:, 1]).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx_f, val_f = scoring.linkpred_topk(comp, rel, h, r, 10, index=index)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak above the tables: %.1f MB; B x N x 4 = %.1f MB" % (peak / 1e6, B * N * 4 / 1e6))
    assert peak < B * N * 4 / 2
    idx_f = idx_f.cpu().numpy()
    listed = linkpred_ref.listed_mask(val[:, 0], val[:, 1], ja.true_tail, N)
    assert (idx_f >= 0).all() and not listed[np.arange(B)[:, None], idx_f].any()
    for j in range(10):
        assert (scoring.linkpred_ranks(comp, rel, h, r, idx_f[:, j], index=index).cpu().numpy() == j + 1).all()
    idx_r = scoring.linkpred_topk(comp, rel, h, r, 10)[0].cpu().numpy()
    rk = scoring.linkpred_ranks(comp, rel, h, r, val[:, 2], index=index).cpu().numpy()
    hit_pred = (idx_r == val[:, 2:3]).any(1)
    other = listed[np.arange(B)[:, None], idx_r] & (idx_r != val[:, 2:3])
    subset = ~other.any(1)
    print("subset %d of %d queries; Hits@10 %.4f" % (subset.sum(), B, hit_pred[subset].mean()))
    assert subset.mean() > 0.5 and 0.05 < hit_pred[subset].mean() < 0.95
    assert (hit_pred[subset] == (rk[subset] <= 10)).all()
