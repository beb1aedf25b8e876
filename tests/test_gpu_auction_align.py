"""GPU: the optimal one-to-one alignment -- jmac_auction_rounds_f32 (the bidding rounds, both launch forms) bit for bit against
the numpy reference on the same lists (tests/auction_ref.py), and scoring.auction_alignment / JMAC.alignment_auction /
harness.evaluate_auction_alignment against the optimality certificate computed in float64 from the STORED matrix
(scoring.alignment_sim) and the returned prices.

Shapes: none is a multiple of a block; 130 rows are more than one wave of rows per block of the row-wise launches; 600 rows open
with more rows than the one-workgroup form's queue (256), so a default run uses both forms."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import auction_ref as ar

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-3


# ---- the rounds kernel against the reference, batch after batch -----------------------------------------------------------------
BATCHES = [1, 64, 3, 64]                     # rounds per call, repeated: a batch of 1 and a batch of 64 among them
MAX_BATCHES = 24                             # (a k = 2 run refills for long: the comparison covers its first calls)


@functools.lru_cache(maxsize=None)
def trajectory(n1, n2, k):
    """The reference run on the lists of a planted CSLS matrix: per call (rounds, lists before it, state and counters after it).
    Computed once, shared by both forms."""
    a, b, _ = ar.planted(n1, n2, 8, 2.0, seed=1)
    c = ar.csls_matrix(a, b, 10)
    st = ar.State(n1, n2)
    idx, val = ar.topk_lists(c, k)
    pref = np.zeros_like(val)
    steps = []
    for t in range(MAX_BATCHES):
        rounds = BATCHES[t % len(BATCHES)]
        before = (idx.copy(), val.copy(), pref.copy(), st.match1.copy())
        counters = ar.run_rounds(idx, val, pref, st, EPS, rounds)
        steps.append((rounds, before, (st.price.copy(), st.owner.copy(), st.match1.copy()), counters))
        if counters[0] == 0:
            break
        ar.refill(c, idx, val, pref, st, k)
    return steps


def _rounds_call(idx, val, pref, n1, n2, k, price, owner, match1, rounds, form, n_open, counters, ws, ld=None, ws_bytes=None, eps=EPS):
    from jmac_amd._lib import lib, ptr, stream
    return lib().jmac_auction_rounds_f32(ptr(idx), ptr(val), ptr(pref), k if ld is None else ld, n1, n2, k, ptr(price), ptr(owner),
                                         ptr(match1), eps, rounds, form, n_open, ptr(counters), ptr(ws),
                                         ws.numel() if ws_bytes is None else ws_bytes, stream())


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("k", [2, 4, 8, 64])
@pytest.mark.parametrize("n1,n2", [(64, 64), (40, 70), (130, 130)])
def test_rounds_kernel_equals_the_reference(n1, n2, k, form):
    from jmac_amd._lib import lib, workspace
    steps = trajectory(n1, n2, k)
    dev = "cuda"
    price = torch.zeros(n2, dtype=torch.float32, device=dev)
    owner = torch.full((n2,), -1, dtype=torch.int32, device=dev)
    match1 = torch.full((n1,), -1, dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = workspace(int(lib().jmac_auction_rounds_workspace_bytes(n1, n2)), dev)
    n_open = n1
    total_rounds = 0
    for t, (rounds, (idx, val, pref, m_before), (w_price, w_owner, w_match1), w_counters) in enumerate(steps):
        # the refill the reference made, applied to the device state: new lists, the refilled rows open again
        d_idx, d_val, d_pref = (torch.from_numpy(x).to(dev) for x in (idx, val, pref))
        match1[torch.from_numpy(m_before == -1).to(dev) & (match1 == -2)] = -1
        assert np.array_equal(match1.cpu().numpy(), m_before), t
        assert _rounds_call(d_idx, d_val, d_pref, n1, n2, k, price, owner, match1, rounds, form, n_open, counters, ws) == 0
        got = counters.tolist()
        assert got == w_counters, (t, got, w_counters)
        assert np.array_equal(match1.cpu().numpy(), w_match1), t
        assert np.array_equal(owner.cpu().numpy(), w_owner), t
        assert np.array_equal(price.cpu().numpy().view(np.uint32), w_price.view(np.uint32)), t
        n_open = got[0]
        total_rounds += got[2]
    assert total_rounds > 0 and len(steps) >= 2
    if k == n2:
        assert n_open == 0                                          # complete lists: the run ends inside the comparison


def test_rounds_kernel_return_codes():
    from jmac_amd._lib import lib, workspace
    n1, n2, k = 300, 300, 4
    dev = "cuda"
    idx = torch.zeros((n1, k), dtype=torch.int32, device=dev)
    val = torch.zeros((n1, k), dtype=torch.float32, device=dev)
    price = torch.zeros(n2, dtype=torch.float32, device=dev)
    owner = torch.full((n2,), -1, dtype=torch.int32, device=dev)
    match1 = torch.zeros(n1, dtype=torch.int32, device=dev)              # every row "holds" column 0: no call here bids
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = workspace(int(lib().jmac_auction_rounds_workspace_bytes(n1, n2)), dev)
    call = functools.partial(_rounds_call, idx, val, val, n1, n2)
    tail = (price, owner, match1, 1, 0, 0, counters, ws)
    assert call(k, *tail) == 0 and counters.tolist() == [0, 0, 0, 0]
    for bad_k in (1, 0, 65):
        assert call(bad_k, *tail, ld=64) == -1                           # JMAC_EINVAL
    assert _rounds_call(idx, val, val, n1, 3, 4, *tail) == -1            # k > n2
    assert call(k, *tail, ld=3) == -1                                    # ld < k
    assert call(k, *tail, ws_bytes=ws.numel() - 256) == -3               # JMAC_EWORKSPACE
    assert call(k, price, owner, match1, 1, 2, 257, counters, ws) == -1  # more open rows than the one-workgroup queue
    assert call(k, price, owner, match1, 1, 2, 256, counters, ws) == 0
    assert call(k, price, owner, match1, 1, 3, 0, counters, ws) == -1    # no such form
    assert call(k, price, owner, match1, 4097, 0, 0, counters, ws) == -1
    for bad_eps in (0.0, -1e-3, float("inf"), float("nan")):
        assert call(k, *tail, eps=bad_eps) == -1
    assert bool((match1 == 0).all()) and bool((price == 0).all())


# ---- the whole alignment: the certificate on the stored matrix -------------------------------------------------------------------
def _operands(n1, n2, d=8, noise=2.0, seed=0):
    a, b, perm = ar.planted(n1, n2, d, noise, seed)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), perm


def _certify(c, m1, v1, price, stats, eps=EPS):
    """The certificate of a result of scoring.auction_alignment on the stored matrix c [n1, n2] (numpy); a transposed run is
    certified on c^T with the matching inverted."""
    n1, n2 = c.shape
    m1, v1, price = m1.cpu().numpy(), v1.cpu().numpy(), price.cpu().numpy()
    assert stats["complete"] and stats["transposed"] == (n1 > n2) and stats["eps"] == eps
    assert stats["unmatched"] == max(0, n1 - n2) == int((m1 < 0).sum())
    held = m1 >= 0
    assert bool(np.isneginf(v1[~held]).all())
    if n1 > n2:
        assert price.shape == (n1,)
        inv = np.full(n2, -1, dtype=np.int64)
        inv[m1[held]] = np.nonzero(held)[0]
        slack, gap, tol = ar.certificate(c.T, inv, price, eps)
    else:
        assert price.shape == (n2,)
        slack, gap, tol = ar.certificate(c, m1, price, eps)
    assert np.abs(v1[held].astype(np.float64) - c[np.nonzero(held)[0], m1[held]]).max() <= 2 * tol
    print("%dx%d: %s, slack %.3e (limit %.3e), gap %.3e (limit %.3e)"
          % (n1, n2, stats, slack, eps + 2 * tol, gap, min(n1, n2) * (eps + 2 * tol)))
    return m1


# (n1, n2, d, noise, k)
CASES = [(64, 64, 8, 2.0, 4), (64, 64, 8, 2.0, 64), (40, 70, 8, 2.0, 4), (70, 40, 8, 2.0, 4), (150, 150, 8, 3.0, 8), (600, 600, 8, 2.0, 16),
         (300, 300, 16, 0.3, 8)]


@pytest.mark.parametrize("n1,n2,d,noise,k", CASES)
def test_auction_alignment_meets_the_certificate(n1, n2, d, noise, k):
    from jmac_amd import scoring
    a, b, perm = _operands(n1, n2, d, noise)
    m1, v1, price, stats = scoring.auction_alignment(a, b, k=k, csls_k=10, eps=EPS)
    assert m1.dtype == torch.int64 and v1.dtype == torch.float32 and price.dtype == torch.float32
    c = scoring.alignment_sim(a, b, "cosine", False, 10).cpu().numpy()
    m1 = _certify(c, m1, v1, price, stats)
    if k == n2:
        assert stats["refills"] == 0 and stats["refill_rows"] == 0
    if n1 > n2:
        assert int((m1 < 0).sum()) == n1 - n2 == 30
    if noise < 1:
        assert stats["rounds"] == 1 and stats["bids"] == n1 and np.array_equal(m1, perm)
    if n1 == 600:
        assert stats["batches"] >= 2                                 # opens on the grid form, ends in the one-workgroup form


def test_raw_similarity():
    from jmac_amd import scoring
    a, b, _ = _operands(64, 64)
    m1, v1, price, stats = scoring.auction_alignment(a, b, k=4, csls_k=0, eps=EPS)
    _certify(scoring.alignment_sim(a, b, "cosine", False, 0).cpu().numpy(), m1, v1, price, stats)
    assert stats["refill_rows"] > 0                                  # the (0, 2 price) refill ran


def test_manhattan():
    from jmac_amd import scoring
    a, b, _ = _operands(40, 70)
    m1, v1, price, stats = scoring.auction_alignment(a, b, k=4, csls_k=10, metric="manhattan", eps=EPS)
    _certify(scoring.alignment_sim(a, b, "manhattan", False, 10).cpu().numpy(), m1, v1, price, stats)


def test_sinkhorn_terms():
    from jmac_amd import scoring
    from jmac_amd._lib import lib, ptr, stream
    a, b, _ = _operands(64, 64)
    r1, r2 = scoring.sinkhorn_terms(a, b, 20.0, 5)
    m1, v1, price, stats = scoring.auction_alignment(a, b, k=4, csls_k=1, terms=(r1, r2), eps=EPS)
    S = scoring.alignment_sim(a, b, "cosine", False, 0)
    c = torch.empty_like(S)
    assert lib().jmac_csls_apply_f32(ptr(S), 64, 64, 64, ptr(r1), ptr(r2), ptr(c), 64, stream()) == 0
    _certify(c.cpu().numpy(), m1, v1, price, stats)


def test_runs_are_bitwise_reproducible_and_the_grid_form_gives_the_same_bits():
    from jmac_amd import scoring
    a, b, _ = _operands(150, 150, noise=3.0)
    m1, v1, price, stats = scoring.auction_alignment(a, b, k=8, eps=EPS)
    again = scoring.auction_alignment(a, b, k=8, eps=EPS)
    assert torch.equal(again[0], m1) and torch.equal(again[1], v1) and torch.equal(again[2], price) and again[3] == stats
    grid = scoring.auction_alignment(a, b, k=8, eps=EPS, form=1)     # the default run took the one-workgroup form: 150 open rows
    assert torch.equal(grid[0], m1) and torch.equal(grid[1], v1) and torch.equal(grid[2], price) and grid[3] == stats


def test_max_rounds_stops_with_a_partial_matching():
    from jmac_amd import scoring
    a, b, _ = _operands(64, 64)
    m1, v1, price, stats = scoring.auction_alignment(a, b, k=4, eps=EPS, max_rounds=1)
    assert stats["complete"] is False and stats["rounds"] == 1 and stats["unmatched"] > 0
    m1 = m1.cpu().numpy()
    held = m1[m1 >= 0]
    assert m1.min() >= -1 and 0 < len(held) == len(np.unique(held))
    assert bool(torch.isneginf(v1[torch.from_numpy(m1 < 0).cuda()]).all())


def test_seven_by_seven_is_the_brute_force_optimum():
    from jmac_amd import scoring
    a, b, _ = ar.planted(7, 7, 8, 2.0, 3)
    a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    c = scoring.alignment_sim(a, b, "cosine", False, 0).cpu().numpy()
    c64 = c.astype(np.float64)
    perms = np.array(list(itertools.permutations(range(7))))
    totals = c64[np.arange(7)[None, :], perms].sum(1)
    order = np.argsort(-totals)
    m1, v1, price, stats = scoring.auction_alignment(a, b, k=2, csls_k=0, eps=EPS)
    tol = ar.tolerance(c, price.cpu().numpy())
    assert totals[order[0]] - totals[order[1]] > 7 * (EPS + 2 * tol)
    assert np.array_equal(m1.cpu().numpy(), perms[order[0]])
    _certify(c, m1, v1, price, stats)


def test_argument_errors():
    from jmac_amd import scoring
    from jmac_amd._lib import JmacError
    e1, e2 = torch.randn(40, 16).cuda(), torch.randn(50, 16).cuda()
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            scoring.auction_alignment(e1, e2, eps=eps)
    for k in (1, 65, 51):
        with pytest.raises(ValueError):
            scoring.auction_alignment(e1, e2, k=k)
    with pytest.raises(ValueError):
        scoring.auction_alignment(e2, e1, k=51)                      # transposed: the 50 rows of e2 are the columns bid for
    with pytest.raises(ValueError):
        scoring.auction_alignment(e1[:0], e2)
    with pytest.raises(ValueError):
        scoring.auction_alignment(e1, e2[:, :12])
    with pytest.raises(JmacError):
        scoring.auction_alignment(e1.cpu(), e2.cpu())


# ---- model and harness ------------------------------------------------------------------------------------------------------------
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


def test_model_alignment_auction():
    from jmac_amd import scoring
    model, kg1, kg2, pairs, graphs, args = mini()
    blocks = _blocks(kg1, kg2, graphs)
    model.eval()
    with torch.no_grad():
        (a1, _), (a2, _) = model.get_emb_blocks(blocks, on_device=True)
        q = np.unique(pairs[:, 0])[:23]
        m1, v1, price, stats = model.alignment_auction(q, blocks, k=4)
        again = model.alignment_auction(torch.from_numpy(q).cuda(), blocks, k=4, emb=(a1, a2))
    model.train()
    assert torch.equal(again[0], m1) and torch.equal(again[1], v1) and torch.equal(again[2], price) and again[3] == stats
    a, b = scoring._alignment_operands(a1, a2, "cosine", False)
    t1, t2 = scoring.csls_terms(a, b, 10)
    qd = torch.from_numpy(q).cuda()
    want = scoring.auction_alignment(a[qd], b, 4, 10, "inner", False, terms=(t1[qd], t2))
    assert torch.equal(m1, want[0]) and torch.equal(v1, want[1]) and torch.equal(price, want[2]) and stats == want[3]
    c = scoring.alignment_sim(a1, a2, "cosine", False, 10).cpu().numpy()[q]
    _certify(c, m1, v1, price, stats)
    with pytest.raises(IndexError):
        model.alignment_auction([kg1.num_entity], blocks, emb=(a1, a2))


def test_harness_evaluate_auction_alignment():
    from jmac_amd import harness
    model, kg1, kg2, pairs, graphs, args = mini()
    precision, stats = harness.evaluate_auction_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=10, k=4)
    assert model.training and 0.0 <= precision <= 100.0 and stats["complete"] is True and stats["unmatched"] == 0
    assert harness.evaluate_auction_alignment(model, kg1, kg2, pairs, graphs, args, csls_k=10, k=4) == (precision, stats)
