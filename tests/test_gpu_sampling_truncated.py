"""GPU: jmac_sample_completion_batch_truncated / sampling.NeighborTable / CompletionSampler(neighbors=) / the harness'
"truncated" mode -- BootEA's hard negatives (modules/train/batch.py:88-165 with neighbor=).  The batches equal the numpy
restatement (tests/trunc_sampler_ref.py) bit for bit and the plain sampler's where nothing is eligible; the table holds the
float64 top-M sets on every row whose M-th / (M+1)-th gap the fp32 scores can resolve, and the reference's ``find_neighbours``
lists (tests/golden/neighbours_small.npz, written by tests/golden/gen_neighbours.py); a captured launch and a captured training
epoch equal the eager ones bitwise.  (The entry point's argument checks need no device: tests/test_trunc_sampler_ref.py.)"""
import os

import numpy as np
import pytest
import torch

import trunc_sampler_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MINI = os.path.join(GOLDEN, "dbp5l_mini")
NUM_ENT, HUB = 600, 80


def _graph():
    """~2 000 triples on 600 entities; (0, 0) is a hub with 80 true tails.  Returns the triples and a batch order that puts the
    hub's triples among the first 200, so the few batches a test draws meet them."""
    rng = np.random.default_rng(7)
    hub_tails = rng.choice(NUM_ENT, HUB, replace=False)
    hub = np.stack((np.zeros(HUB, np.int64), np.zeros(HUB, np.int64), hub_tails), 1)
    n = 1920
    rest = np.stack((rng.integers(1, NUM_ENT, n), rng.integers(0, 4, n), rng.integers(0, NUM_ENT, n)), 1)
    order = rng.permutation(HUB + n)
    triples = np.concatenate((hub, rest)).astype(np.int64)[order]
    is_hub = (triples[:, 0] == 0) & (triples[:, 1] == 0)
    front = rng.permutation(np.concatenate((np.flatnonzero(is_hub), np.flatnonzero(~is_hub)[:200 - HUB])))
    perm = np.concatenate((front, rng.permutation(np.flatnonzero(~is_hub)[200 - HUB:])))
    return triples, np.sort(hub_tails), perm


def _table(M, hub_tails, kind="mixed"):
    """int64 [600, M].  "mixed": random ids (repeats happen by chance); the row of every second hub tail lists hub tails only
    (A = 0 for the hub's triples) and the other hub tails' rows list hub tails after three random ids (A <= 3);
    "repeats": every row is three ids over and over, with -1 and ids >= num_ent in between;
    "own": filled per test with the row's own true tails."""
    rng = np.random.default_rng(100 + M)
    nbr = rng.integers(0, NUM_ENT, (NUM_ENT, M))
    if kind == "repeats":
        base = rng.integers(0, NUM_ENT, (NUM_ENT, 3))
        nbr = base[:, np.arange(M) % 3]
        nbr[:, 4 % M::7] = -1
        nbr[:, 5 % M::11] = NUM_ENT + 5
        return nbr
    for i, t in enumerate(hub_tails):
        nbr[t] = hub_tails[rng.integers(0, HUB, M)]
        if i % 2:
            nbr[t, :min(3, M)] = rng.integers(0, NUM_ENT, min(3, M))
    return nbr


def _sampler(triples, num_ent, B, K, nbr, n_hard, seed, perm=None):
    """(sampler, table); the table's buffer is written directly, past from_indices' range check, so that bad ids reach the kernel."""
    from jmac_amd.sampling import CompletionSampler, NeighborTable
    nbr = np.asarray(nbr)
    tab = NeighborTable(num_ent, nbr.shape[1], "cuda")
    tab.idx.copy_(torch.from_numpy(nbr.astype(np.int32)))
    s = CompletionSampler(triples, num_ent, B, K, "cuda", seed=seed, neighbors=tab, n_hard=n_hard)
    return s, tab


def _check_epochs(triples, num_ent, B, K, nbr, n_hard, perm, what):
    """Two epochs of three launches each against the restatement: the draw counter runs on, the batch number restarts."""
    from jmac_amd import data
    seed = (0x1234567890ABCDE, -77)
    s, _ = _sampler(triples, num_ent, B, K, nbr, n_hard, seed)
    tt = data.true_tail_dict(triples)
    launches = 0
    for epoch in range(2):
        s.new_epoch(torch.Generator(device="cuda").manual_seed(3 + epoch))
        p = np.roll(perm, 7 * epoch)
        s.perm.copy_(torch.from_numpy(p))                                    # an order of the test's own, in the sampler's buffer
        for i in range(3):
            got = s.next_batch()
            want = ref.batch(triples, p, tt, nbr, num_ent, B, K, n_hard, seed, launches, i)
            for name, w in zip(("batch_h", "batch_r", "batch_t"), want):
                assert np.array_equal(got[name].cpu().numpy(), w), (what, epoch, i, name)
            launches += 1
        assert s.step.tolist() == [launches, 3]


@pytest.mark.parametrize("B", [33, 64])
@pytest.mark.parametrize("K,M,n_hard", [(5, 7, 5), (25, 64, 25), (25, 16, 25), (64, 64, 64), (25, 64, 10), (25, 1, 25)])
def test_batches_equal_the_restatement_bit_for_bit(B, K, M, n_hard):
    from jmac_amd import data
    triples, hub_tails, perm = _graph()
    nbr = _table(M, hub_tails)
    tt = data.true_tail_dict(triples)
    first = triples[perm[:3 * B]]                                            # the rows of the first epoch: every regime is there
    A = np.array([sum(ref.eligible(nbr[t], tt[(int(h), int(r))], NUM_ENT)) for h, r, t in first])
    assert (A == 0).any() and (A > 0).any()
    if M >= 7:
        assert ((A > 0) & (A < n_hard)).any()                                # stage 2 fills behind a short stage 1 ...
    if n_hard <= 25:
        assert (A >= min(n_hard, M)).any()                                   # ... and stage 1 has more than it needs
    _check_epochs(triples, NUM_ENT, B, K, nbr, n_hard, perm, (B, K, M, n_hard))


def test_a_tight_entity_set_leaves_stage_two_almost_nothing():
    """num_ent = 70, K = 64: every key has at most 6 true tails, so a row's 64 negatives are nearly all it may have."""
    rng = np.random.default_rng(11)
    triples = np.stack((rng.integers(0, 70, 64), rng.integers(0, 3, 64), rng.integers(0, 70, 64)), 1).astype(np.int64)
    triples[:6, 0], triples[:6, 1], triples[:6, 2] = 5, 1, np.arange(10, 16)  # one key with exactly 6 tails: 64 of 64 allowed
    nbr = rng.integers(0, 70, (70, 64))
    _check_epochs(triples, 70, 16, 64, nbr, 64, rng.permutation(64), "tight")
    _check_epochs(triples, 70, 16, 64, nbr[:, :9], 4, rng.permutation(64), "tight-9")


@pytest.mark.parametrize("kind", ["repeats", "own"])
def test_tables_with_repeats_bad_ids_or_only_true_tails(kind):
    from jmac_amd import data
    triples, hub_tails, perm = _graph()
    if kind == "repeats":
        nbr = _table(16, hub_tails, "repeats")
    else:                                                                    # row t: true tails of some (h, r) that has t as a tail
        tt = data.true_tail_dict(triples)
        nbr = np.zeros((NUM_ENT, 16), dtype=np.int64)
        for h, r, t in triples:
            own = tt[(int(h), int(r))]
            nbr[t] = np.resize(own, 16)
    _check_epochs(triples, NUM_ENT, 33, 25, nbr, 25, perm, kind)


def _epoch(sampler, gen):
    sampler.new_epoch(gen)
    out = []
    for _ in range(len(sampler)):
        d = sampler.next_batch()
        out.append(torch.stack((d["batch_h"], d["batch_r"], d["batch_t"])).cpu().numpy())
    with pytest.raises(StopIteration):
        sampler.next_batch()
    return np.stack(out)


def test_without_an_eligible_neighbour_the_batches_are_the_plain_samplers():
    from jmac_amd.sampling import CompletionSampler
    triples, hub_tails, _ = _graph()
    B, K = 64, 25
    plain = _epoch(CompletionSampler(triples, NUM_ENT, B, K, "cuda", seed=(8, 9)), torch.Generator(device="cuda").manual_seed(2))
    s, _ = _sampler(triples, NUM_ENT, B, K, _table(64, hub_tails), 0, (8, 9))                      # n_hard = 0
    assert np.array_equal(_epoch(s, torch.Generator(device="cuda").manual_seed(2)), plain)
    s, _ = _sampler(triples, NUM_ENT, B, K, np.arange(NUM_ENT)[:, None], None, (8, 9))             # M = 1, nbr[e, 0] = e
    assert s.n_hard == K
    assert np.array_equal(_epoch(s, torch.Generator(device="cuda").manual_seed(2)), plain)
    s, _ = _sampler(triples, NUM_ENT, B, K, _table(64, hub_tails), None, (8, 9))                   # and a table that does bite
    assert not np.array_equal(_epoch(s, torch.Generator(device="cuda").manual_seed(2)), plain)


# ---- the neighbour table ------------------------------------------------------------------------------------------------------
_EMB = {}


def _emb(N, d):
    """Seeded normalised rows (each shape from a fresh default_rng(20261021)) and their float64 products / L1 distances."""
    if (N, d) not in _EMB:
        e = np.random.default_rng(20261021).standard_normal((N, d))
        e = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
        x = e.astype(np.float64)
        _EMB[(N, d)] = (e, x @ x.T, np.abs(x[:, None, :] - x[None, :, :]).sum(2))
    return _EMB[(N, d)]


def _decided_sets(score, M, gap=1e-5):
    """(top-M index sets by descending ``score`` (float64), rows whose M-th and (M+1)-th scores differ by more than ``gap``)."""
    order = np.argsort(-score, axis=1, kind="stable")
    s = np.take_along_axis(score, order, 1)
    return order[:, :M], (s[:, M - 1] - s[:, M]) > gap if M < score.shape[1] else np.ones(len(score), bool)


def _assert_sets(got, want, decided, what):
    n = len(want)
    print("%s: %d of %d rows left out (gap <= 1e-5)" % (what, int((~decided).sum()), n))
    assert (~decided).sum() <= 0.02 * n
    bad = [i for i in range(n) if decided[i] and set(got[i].tolist()) != set(want[i].tolist())]
    assert not bad, (what, bad[:5])
    assert all(len(set(r.tolist())) == got.shape[1] for r in got)            # M distinct ids in every row, decided or not


@pytest.mark.parametrize("N,d,M", [(600, 32, 16), (300, 20, 64)])
def test_neighbor_table_holds_the_float64_top_m_sets(N, d, M):
    """Left out on these inputs (measured in float64 on the CPU): inner 1 of 600 and 2 of 300; manhattan 0 of 600 and 1 of 300.
    The fp32 running sums differ from float64 by at most 2.3e-7 (products) and 2.5e-6 (L1) here, under half the 1e-5 gap."""
    from jmac_amd.sampling import NeighborTable
    e, S, D = _emb(N, d)
    emb = torch.from_numpy(e).cuda()
    tab = NeighborTable(N, M, "cuda")
    p = tab.idx.data_ptr()
    want, decided = _decided_sets(S, M)
    for screen in (None, "bf16"):
        tab.idx.fill_(-1)
        assert tab.refresh(emb, screen=screen) is tab and tab.idx.data_ptr() == p
        got = tab.idx.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (N, M) and got.min() >= 0 and got.max() < N
        _assert_sets(got, want, decided, "inner %s (%d, %d, %d)" % (screen, N, d, M))
        assert (got[:, 0] == np.arange(N)).all()                             # a normalised row's best match is itself
    want, decided = _decided_sets(-D, M)
    tab.idx.fill_(-1)
    tab.refresh(emb, metric="manhattan")
    assert tab.idx.data_ptr() == p
    _assert_sets(tab.idx.cpu().numpy(), want, decided, "manhattan (%d, %d, %d)" % (N, d, M))
    with pytest.raises(ValueError):
        tab.refresh(emb, metric="manhattan", screen="bf16")
    with pytest.raises(ValueError):
        tab.refresh(emb[:-1])


def test_neighbor_table_agrees_with_the_references_find_neighbours():
    from jmac_amd.sampling import NeighborTable
    z = np.load(os.path.join(GOLDEN, "neighbours_small.npz"))
    e, k, want = z["emb"], int(z["k"]), z["neighbours"]
    assert np.array_equal(e, _emb(*e.shape)[0])
    x = e.astype(np.float64)
    _, decided = _decided_sets(x @ x.T, k)
    got = NeighborTable(len(e), k, "cuda").refresh(torch.from_numpy(e).cuda()).idx.cpu().numpy()
    _assert_sets(got, want, decided, "find_neighbours")


def test_from_indices_checks_the_range_and_keeps_repeats():
    from jmac_amd.sampling import NeighborTable
    idx = np.random.default_rng(0).integers(0, 50, (50, 8))
    idx[:, 1] = idx[:, 0]
    for src in (idx, torch.from_numpy(idx).cuda(), torch.from_numpy(idx.astype(np.int32)).cuda()):
        tab = NeighborTable.from_indices(src, "cuda")
        assert (tab.num_ent, tab.m) == (50, 8) and tab.idx.dtype == torch.int32 and np.array_equal(tab.idx.cpu().numpy(), idx)
    bad = idx.copy()
    bad[3, 3] = 50
    with pytest.raises(IndexError):
        NeighborTable.from_indices(bad, "cuda")
    with pytest.raises(IndexError):
        NeighborTable.from_indices(torch.from_numpy(bad).cuda())
    for m in (0, 65):
        with pytest.raises(ValueError):
            NeighborTable(100, m, "cuda")
    with pytest.raises(ValueError):
        NeighborTable(10, 11, "cuda")                                        # m > num_ent


def test_negatives_from_the_table_are_harder():
    """(600, 32) embeddings, M = 16, K = 5: the mean inner product between a gold tail and its negatives is larger under the
    table (a neighbour's product is among its row's 16 largest of 600) than under the filtered sampler at the same seed."""
    from jmac_amd.sampling import CompletionSampler, NeighborTable
    triples, _, _ = _graph()
    e, _, _ = _emb(600, 32)
    tab = NeighborTable(NUM_ENT, 16, "cuda").refresh(torch.from_numpy(e).cuda())
    means = []
    for kw in ({}, {"neighbors": tab}):
        s = CompletionSampler(triples, NUM_ENT, 64, 5, "cuda", seed=(3, 4), **kw)
        ep = _epoch(s, torch.Generator(device="cuda").manual_seed(1))
        gold, neg = ep[:, 2, :64], ep[:, 2, 64:].reshape(-1, 64, 5)
        means.append(float(np.einsum("sbd,sbkd->sbk", e[gold], e[neg]).mean()))
    print("mean <gold, negative>: filtered %.4f, truncated %.4f" % tuple(means))
    assert means[1] > means[0]


def test_a_captured_next_batch_replays_the_epoch():
    triples, hub_tails, _ = _graph()
    B, K = 64, 25
    nbr = _table(16, hub_tails)
    want = _epoch(_sampler(triples, NUM_ENT, B, K, nbr, 20, (8, 9))[0], torch.Generator(device="cuda").manual_seed(2))
    s, tab = _sampler(triples, NUM_ENT, B, K, nbr, 20, (8, 9))
    s.new_epoch(torch.Generator(device="cuda").manual_seed(2))
    n = len(s)
    out = torch.zeros(n, 3, B * (K + 1), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                         # warm-up on a side stream: the epoch's first batch, eager
        d = s.next_batch()
        out[0].copy_(torch.stack((d["batch_h"], d["batch_r"], d["batch_t"])))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d2 = s.next_batch()
    assert d2 is d
    for i in range(1, n):
        graph.replay()
        out[i].copy_(torch.stack((d["batch_h"], d["batch_r"], d["batch_t"])))
    s.skip(n - 1)
    torch.cuda.synchronize()
    assert s.step.tolist() == [n, n]
    assert np.array_equal(out.cpu().numpy(), want)
    # the captured launch reads the table's buffer: new contents, written in place, show in the next replay
    tab.idx.copy_(torch.arange(NUM_ENT, dtype=torch.int32, device="cuda")[:, None].expand(-1, 16))
    plain = _sampler(triples, NUM_ENT, B, K, nbr, 0, (8, 9))[0]
    plain.new_epoch(torch.Generator(device="cuda").manual_seed(2))
    plain.step.copy_(s.step)
    graph.replay()                                                           # wraps to batch 0 of the same order, draw counter n
    p = plain.next_batch()
    torch.cuda.synchronize()
    assert torch.equal(s.batch_t, p["batch_t"]) and torch.equal(s.batch_h, p["batch_h"])


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def _train(mode, capture, epochs=2, **kw):
    """``epochs`` epochs of harness.train_epoch on the mini dataset, a refresh in front of each: per-epoch step losses of every
    pair, and the tables' contents after each refresh."""
    from jmac_amd import data, harness, optim
    from jmac_amd.model import JMAC
    torch.manual_seed(0)
    kgs, s_train, s_test, n_ent = data.load_dbp5l(MINI, "ja")
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, dropout=0.0, lr=5e-3, neg_sampler=mode, neg_neighbors=16,
                             capture_completion=capture, **kw)
    name_emb = np.random.default_rng(0).standard_normal((n_ent, 24)).astype(np.float32)
    model = JMAC(args, name_emb, sum(kg.num_relation for kg in kgs.values()), n_ent).cuda()
    opt_c, opt_a = optim.Adam(model.parameters(), lr=args.lr), optim.Adam(model.parameters(), lr=args.lr)
    gen = torch.Generator(device="cuda").manual_seed(1)
    torch.manual_seed(7)                                                     # the samplers take their seed words from this generator
    state, losses, tables, ptrs = {}, [], [], []
    model.train()
    for _ in range(epochs):
        log = harness.train_epoch(model, kgs, s_train, s_test, opt_c, opt_a, args, state, refresh=True, generator=gen)
        assert all(np.isfinite(p["completion_loss"]) for p in log)
        pairs = sorted(k for k in state if isinstance(k, int))
        losses.append(torch.cat([state[k]["completion"]["step_losses"] for k in pairs]).cpu())
        nb = [t for k in pairs for t in state[k]["completion"].get("neighbors", ())]
        tables.append([t.idx.cpu().numpy().copy() for t in nb])
        ptrs.append([t.idx.data_ptr() for t in nb])
        if mode == "truncated":
            for k in pairs:
                comp = state[k]["completion"]
                assert all(s["sampler"].neighbors in comp["neighbors"] and s["sampler"].n_hard == kw.get("neg_hard", 5) for s in comp["completion_sides"])
                assert all((s["graph"] is not None) == capture for s in comp["completion_sides"])
    return losses, tables, ptrs                                              # (the triple lists grow: an epoch has its own length)


def test_the_harness_trains_with_truncated_negatives_eager_and_captured():
    eager, tables, ptrs = _train("truncated", False)
    assert all(l.numel() > 8 and torch.isfinite(l).all() and (l > 0).all() for l in eager)
    assert len(tables[0]) >= 2 and all(t.shape[1] == 16 for t in tables[0])
    assert ptrs[0] == ptrs[1]                                                # one buffer per KG for the whole run ...
    assert all(not np.array_equal(a, b) for a, b in zip(*tables))            # ... with new contents at the second refresh
    captured, tables_c, _ = _train("truncated", True)
    assert all(torch.equal(a, b) for a, b in zip(eager, captured)), (eager, captured)      # per-step losses, bitwise
    assert all(np.array_equal(a, b) for a, b in zip(tables[1], tables_c[1]))
    # "filtered" is what it was: no table, the plain entry, other losses than the hard negatives give -- and exactly the losses
    # of the new entry when it is told to place no hard negative (the same batches bit for bit, through the other path)
    filt, none, _ = _train("filtered", False, epochs=1)
    assert none == [[]] and torch.isfinite(filt[0]).all()
    assert filt[0].shape == eager[0].shape and not torch.equal(filt[0], eager[0])
    hard0, _, _ = _train("truncated", False, epochs=1, neg_hard=0)
    assert torch.equal(filt[0], hard0[0]), (filt, hard0)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_mismatched_tables_and_missing_embeddings_are_refused():
    from jmac_amd import harness
    from jmac_amd.sampling import CompletionSampler, NeighborTable
    triples, _, _ = _graph()
    with pytest.raises(ValueError, match="601 entities"):
        CompletionSampler(triples, NUM_ENT, 32, 5, "cuda", neighbors=NeighborTable(NUM_ENT + 1, 4, "cuda"))
    tab = NeighborTable(NUM_ENT, 4, "cuda")
    with pytest.raises(ValueError):
        CompletionSampler(triples, NUM_ENT, 32, 5, "cuda", neighbors=tab, n_hard=6)
    with pytest.raises(ValueError):
        CompletionSampler(triples, NUM_ENT, 32, 5, "cuda", n_hard=2)         # n_hard without a table
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, neg_sampler="truncated")
    ei = torch.zeros((2, 1), dtype=torch.int64, device="cuda")
    for state in (None, {}):
        with pytest.raises(ValueError, match="neighbors.*embeddings"):
            harness.train_completion_component(None, None, ei, None, ei, None, {}, triples, triples, NUM_ENT, NUM_ENT, args, state=state)
    args.neg_sampler = "nearest"
    with pytest.raises(ValueError, match="truncated"):
        harness.train_completion_component(None, None, ei, None, ei, None, {}, triples, triples, NUM_ENT, NUM_ENT, args)
