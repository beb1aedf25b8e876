"""GPU: cross-KG ensemble link prediction -- scoring.linkpred_ranks_ensemble / linkpred_topk_ensemble (jmac_linkpred_ens_*): ranks
and top-k of the target KG's tails on D = w_0 d_0 + sum_s w_s (d_s where the head and the candidate are both linked into
supporting KG s, d_0 otherwise), the supporting rows read through the link maps inside the kernel.

The two kinds of check of test_gpu_linkpred_topk.py.  EXACT, against the ensemble rank kernel (the same D bit for bit): the j-th
prediction ranks j + 1, order, tie rule, exclusion, repeatability; and bit for bit against the single-KG entry points where D
reduces to d_0.  Against FLOAT64 (tests/ensemble_ref.py) with a derived tolerance: every member's distance is a sequential fp32
sum of m = n_layers * d terms, error below (m + 2) 2^-24 max|d_g|; the members pass through their weights and every fold rounds
once more (S + 1 folds), so |D - D64| < (m + 2 + S + 1) 2^-24 sum(w) max_g max|d_g|, and `bound` doubles that: two candidates
whose float64 D differ by more than `bound` cannot change order in fp32.  Decided and index-asserted positions are defined as in
test_gpu_linkpred_topk.py; both shares are printed and depend on the float64 reference alone."""
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ensemble_ref
import linkpred_ref
from conftest import GOLDEN

TILE = 64           # the tile kernel's candidate tile: a tile without a link skips the supporting member's loop


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _links(N, rows, rng, frac=0.5):
    """One random injective partial map per supporting KG, about ``frac`` of the target rows each.  Row 0 is linked in every
    member; a contiguous block of unlinked rows (128, or the last tile of a small N) holds a whole candidate tile and row
    ``free`` inside it is unlinked everywhere."""
    if N >= 256:
        start = (N // 2) // TILE * TILE
        block = np.arange(start, start + 2 * TILE)
    else:
        block = np.arange((N - 1) // TILE * TILE, N)
    links = []
    for n in rows:
        cnt = min(int(N * frac), n * 3 // 4)
        pool = np.setdiff1d(np.arange(1, N), block)
        src = np.concatenate(([0], rng.choice(pool, cnt - 1, replace=False)))
        link = np.full(N, -1, dtype=np.int64)
        link[src] = rng.choice(n, cnt, replace=False)
        links.append(link)
    return links, int(block[len(block) // 2])


def _assert_inputs(links, h, N):
    for link in links:
        assert (link[h] >= 0).any() and (link[h] < 0).any()              # linked and unlinked heads in every member
        lk = link[link >= 0]
        assert len(np.unique(lk)) == len(lk)                              # injective
        tiles = [link[t:t + TILE] for t in range(0, N, TILE)]
        assert any((t < 0).all() for t in tiles) and any((t >= 0).any() for t in tiles)       # a tile without any link


def _case(N, rows, d, nl, B, seed, nrel=11, integer=False, shared_rel=False):
    """(members on the device, members as numpy for the reference, h, r, links)"""
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    if integer:
        mk = lambda n: torch.randint(-2, 3, (n, d), generator=gen).float()
    else:
        mk = lambda n: torch.randn(n, d, generator=gen)
    links, free = _links(N, rows, rng)
    h, r = rng.integers(0, N, B), rng.integers(0, nrel, B)
    h[0], h[1] = 0, free
    _assert_inputs(links, h, N)
    tabs = [([mk(n) for _ in range(nl)], [mk(nrel) for _ in range(nl)]) for n in [N] + list(rows)]
    if shared_rel:
        tabs = [(e, tabs[0][1]) for e, _ in tabs]
    return tabs, links, h, r, rng


def _members(tabs, links, weights):
    dev = [([e.cuda() for e in ent], [x.cuda() for x in rel], None if g == 0 else torch.from_numpy(links[g - 1]).cuda(), w)
           for g, ((ent, rel), w) in enumerate(zip(tabs, weights))]
    ref = [([e.numpy() for e in ent], [x.numpy() for x in rel], None if g == 0 else links[g - 1], w)
           for g, ((ent, rel), w) in enumerate(zip(tabs, weights))]
    return dev, ref


def _lists(h, r, N, rng, lo=0, hi=40, absent=0.2):
    tt = {}
    for hb, rb in zip(h, r):
        if (int(hb), int(rb)) not in tt and rng.random() >= absent:
            n = int(rng.integers(lo, hi))
            if n:
                tt[(int(hb), int(rb))] = np.sort(rng.choice(N, min(n, N), replace=False))
    return tt


def _index(tt):
    from jmac_amd.sampling import TrueTailIndex
    return TrueTailIndex.from_dict(tt, "cuda") if tt else None


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def check_exact(members, h, r, k, tt, pred_head=False):
    """The contract, without a tolerance; returns (idx, val) as numpy."""
    from jmac_amd import scoring
    index = _index(tt)
    idx_t, val_t = scoring.linkpred_topk_ensemble(members, h, r, k, index=index, pred_head=pred_head)
    idx2, val2 = scoring.linkpred_topk_ensemble(members, h, r, k, index=index, pred_head=pred_head)
    assert idx_t.dtype == torch.int64 and val_t.dtype == torch.float32 and idx_t.shape == val_t.shape == (len(h), k)
    assert torch.equal(idx_t, idx2) and torch.equal(val_t.view(torch.int32), val2.view(torch.int32))     # identical bits
    idx, val = idx_t.cpu().numpy(), val_t.cpu().numpy()
    N = members[0][0][0].shape[0]
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
        assert valid[b].sum() == min(k, N - len(np.unique(lst[(lst >= 0) & (lst < N)])))          # row lengths
    rk2 = None
    for j in range(k):                                                       # EVERY prediction: the j-th ranks j + 1
        gold = np.where(valid[:, j], idx[:, j], 0)
        rk = scoring.linkpred_ranks_ensemble(members, h, r, gold, index=index, pred_head=pred_head)
        if j == 0:
            rk2 = scoring.linkpred_ranks_ensemble(members, h, r, gold, index=index, pred_head=pred_head)
            assert torch.equal(rk, rk2)
        rk = rk.cpu().numpy()
        assert (rk[valid[:, j]] == j + 1).all(), (j, rk[valid[:, j]][:10])
    return idx, val


def _bound(ref_members, h, r, pred_head, nl, d):
    ds, _ = ensemble_ref.member_dists(ref_members, h, r, pred_head)
    scale = max(np.abs(x).max() for x in ds)
    S, wsum = len(ref_members) - 1, sum(float(m[3]) for m in ref_members)
    return 2 * (nl * d + 2 + S + 1) * 2.0 ** -24 * wsum * scale


def check_float64(D64, listed, bound, k, idx, val, min_decided=None):
    """test_gpu_linkpred_topk.check_float64 on the ensemble distance: the project's tolerance on the values, completeness,
    decided positions; returns the two shares."""
    B = D64.shape[0]
    ridx, rval = linkpred_ref.topk(D64, k + 1, listed)
    valid = idx >= 0
    assert (valid == (ridx[:, :k] >= 0)).all()
    rows = np.arange(B)[:, None]
    got64 = np.where(valid, D64[rows, np.where(valid, idx, 0)], np.inf)
    err = np.abs(np.where(valid, val, 0.0) - np.where(valid, got64, 0.0)).max()
    rest = np.where(listed, np.inf, D64)
    for b in range(B):
        rest[b, idx[b][valid[b]]] = np.inf
    last = np.where(valid[:, -1], got64[:, -1], np.inf)
    slack = rest.min(1)[np.isfinite(last)] - last[np.isfinite(last)]
    with np.errstate(invalid="ignore"):
        gap = rval[:, 1:] - rval[:, :-1]
        decided = (gap > bound) & valid
    pinned = decided.copy()
    pinned[:, 1:] &= decided[:, :-1]
    wrong_sets = wrong_idx = 0
    for b in range(B):
        for j in np.flatnonzero(decided[b]):
            wrong_sets += set(idx[b, :j + 1].tolist()) != set(ridx[b, :j + 1].tolist())
        wrong_idx += int((idx[b][pinned[b]] != ridx[b, :k][pinned[b]]).sum())
    share, share_pinned = decided[valid].mean(), pinned[valid].mean()
    print("float64: |val - D64| max %.3g (allowed %.3g), bound %.3g at scale %.4g, completeness slack min %.3g, decided %.4f and "
          "index asserted %.4f of %d" % (err, 1e-4 * np.abs(D64).max(), bound, np.abs(D64).max(), slack.min() if len(slack) else np.inf,
                                       share, share_pinned, valid.sum()))
    assert err <= 1e-4 * np.abs(D64).max()                                   # (i) the project's tolerance
    assert len(slack) == 0 or slack.min() >= -bound                          # (ii) completeness
    assert wrong_sets == 0 and wrong_idx == 0                                # (iii) decided positions
    if min_decided is not None:
        assert share >= min_decided and share_pinned >= 2 * min_decided - 1
    return share, share_pinned


def check_ranks_float64(members, D64, listed, bound, h, r, gold, tt, pred_head=False):
    """rank[b] between 1 + #{unlisted n: D64 < D64[gold] - bound} and 1 + #{unlisted n != gold: D64 <= D64[gold] + bound}, and the
    float64 rank wherever no other candidate lies within `bound` of the gold."""
    from jmac_amd import scoring
    rk = scoring.linkpred_ranks_ensemble(members, h, r, gold, index=_index(tt), pred_head=pred_head).cpu().numpy()
    rows = np.arange(len(gold))
    g = D64[rows, gold][:, None]
    other = ~listed
    other[rows, gold] = False
    lo = 1 + (other & (D64 < g - bound)).sum(1)
    hi = 1 + (other & (D64 <= g + bound)).sum(1)
    assert ((rk >= lo) & (rk <= hi)).all()
    clear = lo == hi
    ref = ensemble_ref.ranks(D64, gold, listed)
    assert (rk[clear] == ref[clear]).all()
    print("ranks: %d of %d queries have no candidate within the bound of their gold" % (clear.sum(), len(gold)))
    return rk, clear


# ---- the contract on every path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,rows,d,nl,B,k,pred_head,weights", [
    (70, [50], 7, 3, 9, 10, False, (0.6, 0.4)),                              # rows of 28 bytes, three layers
    (300, [250, 400], 48, 2, 37, 1, True, (0.5, 0.3, 0.2)),
    (4000, [3000], 300, 2, 130, 10, False, (0.5, 0.5)),                      # the matrix path (N < 8192)
    (9000, [7000], 30, 2, 70, 10, False, (0.7, 0.3)),                        # the fused path, rows of 120 bytes (scalar loads)
    (20000, [15000, 9000, 12000], 64, 1, 96, 64, False, (0.4, 0.3, 0.2, 0.1)),       # S = 3
])
def test_ensemble_contract_filtered_and_raw(N, rows, d, nl, B, k, pred_head, weights):
    tabs, links, h, r, rng = _case(N, rows, d, nl, B, N + d + k)
    members, ref = _members(tabs, links, weights)
    tt = _lists(h, r, N, rng)
    D64 = ensemble_ref.D64(ref, h, r, pred_head)
    bound = _bound(ref, h, r, pred_head, nl, d)
    gold = rng.integers(0, N, B)
    for lists in (tt, None):
        listed = linkpred_ref.listed_mask(h, r, lists or {}, N)
        idx, val = check_exact(members, h, r, k, lists, pred_head)
        check_float64(D64, listed, bound, k, idx, val)
        check_ranks_float64(members, D64, listed, bound, h, r, gold, lists, pred_head)


# ---- reductions to the single-KG path, bit for bit ---------------------------------------------------------------------------
def _equal_to_single_kg(members, comp, rel, h, r, k, tt, pred_head):
    from jmac_amd import scoring
    index = _index(tt)
    gold = np.random.default_rng(1).integers(0, comp[0].shape[0], len(h))
    idx, val = scoring.linkpred_topk_ensemble(members, h, r, k, index=index, pred_head=pred_head)
    idx1, val1 = scoring.linkpred_topk(comp, rel, h, r, k, index=index, pred_head=pred_head)
    assert torch.equal(idx, idx1) and torch.equal(val.view(torch.int32), val1.view(torch.int32))
    rk = scoring.linkpred_ranks_ensemble(members, h, r, gold, index=index, pred_head=pred_head)
    assert torch.equal(rk, scoring.linkpred_ranks(comp, rel, h, r, gold, index=index, pred_head=pred_head))


@pytest.mark.parametrize("N,rows,d,pred_head", [(300, [250, 400], 48, True), (9000, [7000, 5000], 30, False)])
def test_ensemble_reduces_to_the_single_kg_entry_points(N, rows, d, pred_head):
    k, B = 10, 40
    tabs, links, h, r, rng = _case(N, rows, d, 2, B, N + 1)
    tt = _lists(h, r, N, rng)
    members, _ = _members(tabs, links, (1.0, 0.0, 0.0))                      # weights (1, 0, 0), arbitrary links
    comp, rel = members[0][0], members[0][1]
    for lists in (tt, None):
        _equal_to_single_kg(members, comp, rel, h, r, k, lists, pred_head)
        _equal_to_single_kg(members[:1], comp, rel, h, r, k, lists, pred_head)           # n_members = 1
    # no link at all, weights (0.5, 0.25, 0.25), integer tables in {-2 .. 2}: every product and sum is exact
    tabs, _, h, r, rng = _case(N, rows, d, 2, B, N + 2, integer=True)
    none = [np.full(N, -1, dtype=np.int64) for _ in rows]
    members, _ = _members(tabs, none, (0.5, 0.25, 0.25))
    for lists in (tt, None):
        _equal_to_single_kg(members, members[0][0], members[0][1], h, r, k, lists, pred_head)


# ---- exact ties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [300, 9000])
def test_ensemble_exact_ties_equal_float64_stable_topk(N):
    """Integer tables in {-2 .. 2} in every member, weights (0.5, 0.25, 0.25): every D is an exact multiple of 1/4 in fp32,
    thousands of ties: the predictions ARE the float64 stable top-k, index for index, and the ranks the float64 ranks."""
    from jmac_amd import scoring
    rows = [N - 50, N + 100]
    tabs, links, h, r, rng = _case(N, rows, 12, 2, 64, N, nrel=7, integer=True)
    members, ref = _members(tabs, links, (0.5, 0.25, 0.25))
    tt = _lists(h, r, N, rng, hi=60)
    D64 = ensemble_ref.D64(ref, h, r)
    gold = rng.integers(0, N, len(h))
    for lists in (tt, None):
        listed = linkpred_ref.listed_mask(h, r, lists or {}, N)
        for k in (10, 64):
            idx, val = check_exact(members, h, r, k, lists)
            ridx, rval = linkpred_ref.topk(D64, k, listed)
            assert (idx == ridx).all() and (val == rval).all()
            assert (rval[:, 1:] == rval[:, :-1]).sum() > 100
        rk = scoring.linkpred_ranks_ensemble(members, h, r, gold, index=_index(lists)).cpu().numpy()
        assert (rk == ensemble_ref.ranks(D64, gold, listed)).all()


def test_ensemble_overflowing_rows_are_recomputed_exactly():
    """Constant candidate tables in every member (and the same relation rows): every D of a row is equal, every candidate list
    overflows, the recompute path answers 0 .. k-1 minus the listed ones."""
    N, d, k = 9000, 16, 10
    rng = np.random.default_rng(9)
    rows = [7000, 9500]
    links, free = _links(N, rows, rng)
    rel = [torch.randn(5, d, generator=torch.Generator().manual_seed(2))]
    tabs = [([torch.ones(n, d)], rel) for n in [N] + rows]
    members, _ = _members(tabs, links, (0.5, 0.25, 0.25))
    h, r = np.array([0, 17, 8999, free]), np.array([0, 1, 2, 3])
    _assert_inputs(links, h, N)
    tt = {(0, 0): np.array([0, 1, 5, 8000]), (17, 1): np.array([3]), (free, 3): np.arange(0, 40, 2)}
    idx, val = check_exact(members, h, r, k, tt)
    for b in range(4):
        lst = tt.get((int(h[b]), int(r[b])), np.zeros(0, dtype=np.int64))
        assert idx[b].tolist() == [n for n in range(60) if n not in set(lst.tolist())][:k]
        assert (val[b] == val[b, 0]).all()
    idx, _ = check_exact(members, h, r, k, None)
    assert (idx == np.arange(k)).all()


# ---- the ja-sized case -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(0.5, 0.3, 0.2), (0.5, 0.5)])
def test_ensemble_against_float64_on_the_seeded_ja_sized_case(weights):
    """N = 11 805 with supports of 13 996 and 5 231 rows, d = 300, two layers, k = 10; standard-normal tables (seed 1234: per
    member the entity layers, then the relation layers of 50 rows), 40 % random injective links (numpy seed 1234), 256 queries.
    At least 0.90 of the positions must be decided and 0.80 index-asserted; the float64 reference alone decides 0.937 (S = 2)
    and 0.944 (S = 1) of them at bound 0.069, distance scale about 955, and index-asserts 0.893 and 0.904 (draw order as coded
    here: tables, then per support the linked rows and their images, then the queries)."""
    N, rows, d, nl, k, B = 11805, [13996, 5231][:len(weights) - 1], 300, 2, 10, 256
    gen = torch.Generator().manual_seed(1234)
    tabs = []
    for n in [N, 13996, 5231]:                                               # (the S = 1 case draws the same tables)
        ent = [torch.randn(n, d, generator=gen) for _ in range(nl)]
        tabs.append((ent, [torch.randn(50, d, generator=gen) for _ in range(nl)]))
    rng = np.random.default_rng(1234)
    links = []
    for n in [13996, 5231]:
        link = np.full(N, -1, dtype=np.int64)
        cnt = int(0.4 * N)
        link[rng.choice(N, cnt, replace=False)] = rng.choice(n, cnt, replace=False)
        links.append(link)
    h, r = rng.integers(0, N, B), rng.integers(0, 50, B)
    tabs, links = tabs[:len(weights)], links[:len(weights) - 1]
    for link in links:
        assert (link[h] >= 0).any() and (link[h] < 0).any()
    members, ref = _members(tabs, links, weights)
    D64 = ensemble_ref.D64(ref, h, r)
    bound = _bound(ref, h, r, False, nl, d)
    listed = np.zeros((B, N), dtype=bool)
    idx, val = check_exact(members, h, r, k, None)
    check_float64(D64, listed, bound, k, idx, val, min_decided=0.90)
    check_ranks_float64(members, D64, listed, bound, h, r, rng.integers(0, N, B), None)


# ---- plumbing on the real el + ja pair -----------------------------------------------------------------------------------------
def _ja_el():
    from jmac_amd import data, harness
    from jmac_amd.model import JMAC
    kgs, s_train, _, n_ent = data.kgs_from_arrays(data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz")), "ja")
    torch.manual_seed(0)
    args = harness.make_args(dim=32, batch_size=256, num_negative=5, dropout=0.0)
    name_emb = np.random.default_rng(0).standard_normal((n_ent, 24)).astype(np.float32)
    model = JMAC(args, name_emb, sum(kg.num_relation for kg in kgs.values()), n_ent).cuda()
    (pair, seeds), = s_train.items()
    seeds = seeds if pair == ("ja", "el") else seeds[:, ::-1]                # (target = ja row, support = el row)
    graphs = [(torch.from_numpy(kgs[l].edge_index).cuda(), torch.from_numpy(kgs[l].edge_type).cuda()) for l in ("ja", "el")]
    link = harness.alignment_links(kgs["ja"], kgs["el"], seeds, device="cuda")
    return model, kgs, graphs, link, seeds, args


def test_ensemble_plumbing_on_the_real_ja_el_pair():
    from jmac_amd import harness, scoring
    model, kgs, graphs, link, seeds, args = _ja_el()
    ja, el = kgs["ja"], kgs["el"]
    N = ja.num_entity
    lk = link.cpu().numpy()
    assert lk.shape == (N,) and (lk >= 0).sum() == len(np.unique(seeds[:, 0])) and lk.max() < el.num_entity
    # alignment_links: seeds win over a predicted match, which fills the rows without a seed
    pred = torch.full((N,), 3, dtype=torch.int64)
    both = harness.alignment_links(ja, el, seeds, predicted=pred).numpy()
    assert (both[lk >= 0] == lk[lk >= 0]).all() and (both[lk < 0] == 3).all()
    blocks = [(ei, et, [k.entity_id_base, k.upper_entity_base], [k.relation_id_base, k.upper_relation_base])
              for k, (ei, et) in zip((ja, el), graphs)]
    q = ja.val_data[np.random.default_rng(0).choice(len(ja.val_data), 512, replace=False)]
    index = harness._true_tail_index(ja, "cuda")
    model.eval()
    with torch.no_grad():
        cached = model.forward_blocks(blocks)
        members = [(c[1], c[2], l, w) for c, l, w in zip(cached, (None, link), (0.5, 0.5))]
        rk_model = model.linkpred_ranks_ensemble(q[:, 0], q[:, 1], q[:, 2], blocks, [link], (0.5, 0.5), index=index)
        rk = scoring.linkpred_ranks_ensemble(members, q[:, 0], q[:, 1], q[:, 2], index=index)
        assert torch.equal(rk_model, rk)
        assert torch.equal(model.linkpred_ranks_ensemble(q[:, 0], q[:, 1], q[:, 2], blocks, [link], (0.5, 0.5), index=index,
                                                         cached=cached), rk)
        idx_m, val_m = model.linkpred_topk_ensemble(q[:, 0], q[:, 1], 10, blocks, [link], (0.5, 0.5), index=index, cached=cached)
        idx_s, val_s = scoring.linkpred_topk_ensemble(members, q[:, 0], q[:, 1], 10, index=index)
        assert torch.equal(idx_m, idx_s) and torch.equal(val_m, val_s)
        # the evaluator encodes every KG with forward_base, as evaluate_completion does
        members = [(c[1], c[2], l, w) for c, l, w in zip([model.forward_base(*b) for b in blocks], (None, link), (0.5, 0.5))]
    # weights (1, 0): exactly the single-KG evaluator's numbers
    kw = dict(split="val", filtered=True)
    assert harness.evaluate_completion_ensemble(model, kgs, "ja", ["el"], graphs, [link], (1.0, 0.0), args, **kw) == \
        harness.evaluate_completion(model, ja, graphs[0][0], graphs[0][1], args, "val", filtered=True, fused=True)
    # weights (0.5, 0.5) on 512 queries of the split: the float64 reference's metrics, up to the undecided ranks
    sub = dict(kgs, ja=dataclasses.replace(ja, val_data=q))
    sub["ja"]._true_tail_index = getattr(ja, "_true_tail_index", None)
    got = harness.evaluate_completion_ensemble(model, sub, "ja", ["el"], graphs, [link], (0.5, 0.5), args, **kw)
    ref = [([x.cpu().numpy() for x in m[0]], [x.cpu().numpy() for x in m[1]], None if m[2] is None else lk, m[3]) for m in members]
    D64 = ensemble_ref.D64(ref, q[:, 0], q[:, 1])
    listed = linkpred_ref.listed_mask(q[:, 0], q[:, 1], ja.true_tail, N)
    bound = _bound(ref, q[:, 0], q[:, 1], False, len(members[0][0]), members[0][0][0].shape[1])
    _, clear = check_ranks_float64(members, D64, listed, bound, q[:, 0], q[:, 1], q[:, 2], ja.true_tail)
    r64 = ensemble_ref.ranks(D64, q[:, 2], listed).astype(np.float64)
    want = ((r64 <= 1).mean(), (r64 <= 10).mean(), (1.0 / r64).mean())
    slack = float((~clear).sum()) / len(q)                                   # every undecided query moves a metric by <= 1 / B
    print("ensemble metrics %s, float64 %s, undecided ranks %d of %d" % (got, want, (~clear).sum(), len(q)))
    assert all(abs(a - b) <= slack + 1e-12 for a, b in zip(got, want))


# ---- refusals, before any launch -----------------------------------------------------------------------------------------------
def test_ensemble_refuses_bad_arguments_before_any_launch():
    from jmac_amd import _lib, scoring
    tabs, links, h, r, _ = _case(70, [50], 8, 1, 4, 3)
    members, _ = _members(tabs, links, (0.5, 0.5))
    for k in (0, 65, 71):                                                    # k outside [1, min(64, N)]
        with pytest.raises(ValueError):
            scoring.linkpred_topk_ensemble(members, h, r, k)
    cpu = [([e.cpu() for e in m[0]], [x.cpu() for x in m[1]], None if m[2] is None else m[2].cpu(), m[3]) for m in members]
    with pytest.raises(_lib.JmacError):                                      # a CPU tensor
        scoring.linkpred_topk_ensemble(cpu, h, r, 3)
    with pytest.raises(_lib.JmacError):
        scoring.linkpred_ranks_ensemble([members[0], (members[1][0], members[1][1], members[1][2].cpu(), 0.5)], h, r, h)
    short = [members[0], (members[1][0], members[1][1], members[1][2][:-1].clone(), 0.5)]
    with pytest.raises(ValueError):                                          # a link map of the wrong length
        scoring.linkpred_ranks_ensemble(short, h, r, h)
    big = members[1][2].clone()
    big[5] = 50                                                              # a link value >= n_rows
    with pytest.raises(IndexError):
        scoring.linkpred_ranks_ensemble([members[0], (members[1][0], members[1][1], big, 0.5)], h, r, h)
    with pytest.raises(IndexError):
        scoring.linkpred_topk_ensemble([members[0], (members[1][0], members[1][1], big, 0.5)], h, r, 3)
    with pytest.raises(ValueError):                                          # a negative weight, a link on the target
        scoring.linkpred_ranks_ensemble([members[0], (members[1][0], members[1][1], members[1][2], -1.0)], h, r, h)
    with pytest.raises(ValueError):
        scoring.linkpred_ranks_ensemble([(members[0][0], members[0][1], members[1][2], 1.0)], h, r, h)
