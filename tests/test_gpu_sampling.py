"""GPU: jmac_sample_completion_batch / sampling.CompletionSampler -- the completion batches built on the device equal the numpy
restatement of the stream definition (tests/sampler_ref.py) bit for bit, hold the reference sampler's properties on the real
DBP-5L triples (modules/load/data_loader.py:36-47: distinct negatives, none a true tail of the row's (h, r)), replay from a
hipGraph as the batches of an epoch, and feed the harness' "filtered" and captured modes."""
import os

import numpy as np
import pytest
import torch

import sampler_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MINI = os.path.join(GOLDEN, "dbp5l_mini")


def _real(lang):
    from jmac_amd import data
    z = data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz"))
    return np.asarray(z[lang + ".train"], dtype=np.int64), int(z[lang + ".num_entity"])


def _toy(num_ent, n_tails, T, seed):
    """T triples on num_ent entities; (0, 0) has n_tails true tails."""
    rng = np.random.default_rng(seed)
    big = np.stack((np.zeros(n_tails, np.int64), np.zeros(n_tails, np.int64), rng.choice(num_ent, n_tails, replace=False)), 1)
    rest = np.stack((rng.integers(1, num_ent, T - n_tails), rng.integers(0, 3, T - n_tails), rng.integers(0, num_ent, T - n_tails)), 1)
    return rng.permutation(np.concatenate((big, rest)).astype(np.int64))


def _cases():
    from jmac_amd import data
    kgs, _, _, _ = data.load_dbp5l(MINI, "ja")
    ja, n_ja = _real("ja")
    return {"mini": (kgs["ja"].train_data, kgs["ja"].num_entity, 32, 5),
            "ja": (ja, n_ja, 1000, 25),
            "toy70-k25": (_toy(70, 40, 64, 0), 70, 16, 25),
            "toy70-k30": (_toy(70, 40, 64, 1), 70, 16, 30),               # K = every allowed entity of the long key
            "toy200-k64": (_toy(200, 5, 64, 2), 200, 16, 64)}


@pytest.mark.parametrize("case", ["mini", "ja", "toy70-k25", "toy70-k30", "toy200-k64"])
def test_batches_equal_the_restatement_bit_for_bit(case):
    from jmac_amd import data
    from jmac_amd.sampling import CompletionSampler
    triples, num_ent, B, K = _cases()[case]
    seed = (0x1234567890ABCDE, -77)                                       # both words wider than 32 bits: the low halves key the stream
    s = CompletionSampler(triples, num_ent, B, K, "cuda", seed=seed)
    tt = data.true_tail_dict(triples)
    gen = torch.Generator(device="cuda").manual_seed(3)
    launches = 0
    for epoch in range(2):                                                # the second epoch: step[0] runs on, step[1] restarts
        s.new_epoch(gen)
        perm = s.perm.cpu().numpy()
        assert np.array_equal(np.sort(perm), np.arange(len(triples)))
        first = None
        for i in range(3):
            got = s.next_batch()
            first = first or got
            assert got is first and got["batch_t"] is s.batch_t           # the same objects every time
            want = sampler_ref.batch(triples, perm, tt, num_ent, B, K, seed, launches, i)
            for name, w in zip(("batch_h", "batch_r", "batch_t"), want):
                assert got[name].dtype == torch.int64 and tuple(got[name].shape) == (B * (K + 1),)
                assert np.array_equal(got[name].cpu().numpy(), w), (case, epoch, i, name)
            assert torch.equal(s.neg, s.batch_t[B:].view(B, K))
            launches += 1
        assert s.step.tolist() == [launches, 3]


def _epoch(sampler, gen):
    sampler.new_epoch(gen)
    out = []
    for _ in range(len(sampler)):
        d = sampler.next_batch()
        out.append(torch.stack((d["batch_h"], d["batch_r"], d["batch_t"])).cpu().numpy())
    with pytest.raises(StopIteration):
        sampler.next_batch()
    return np.stack(out), sampler.perm.cpu().numpy()


def _codes(triples, num_ent):
    """Sorted codes of the true (h, r, t): membership of a candidate tail is one np.isin."""
    nrel = int(triples[:, 1].max()) + 1
    return nrel, np.unique((triples[:, 0] * nrel + triples[:, 1]) * num_ent + triples[:, 2])


def _false_negatives_and_repeats(h, r, neg, nrel, num_ent, true_codes):
    """(negatives that are a true tail of their row's (h, r), repeats inside a row) of one batch: h, r [B], neg [B, K]."""
    hit = np.isin((h[:, None] * nrel + r[:, None]) * num_ent + neg, true_codes)
    s = np.sort(neg, axis=1)
    return int(hit.sum()), int((s[:, 1:] == s[:, :-1]).sum())


@pytest.mark.parametrize("lang", ["ja", "el"])
def test_an_epoch_on_the_real_triples_has_the_reference_samplers_properties(lang):
    from jmac_amd import data
    from jmac_amd.sampling import CompletionSampler
    triples, num_ent = _real(lang)
    B, K, T = 1000, 25, len(triples)
    ep, perm = _epoch(CompletionSampler(triples, num_ent, B, K, "cuda", seed=(11, 22)), torch.Generator(device="cuda").manual_seed(5))
    assert ep.shape == (T // B, 3, B * (K + 1))
    nrel, true_codes = _codes(triples, num_ent)
    tt = data.true_tail_dict(triples)
    for i, (bh, br, bt) in enumerate(ep):
        pos = triples[perm[i * B:(i + 1) * B]]                            # the positives: triples[perm[: (T // B) * B]] in order
        assert np.array_equal(bh, np.tile(pos[:, 0], K + 1)) and np.array_equal(br, np.tile(pos[:, 1], K + 1))
        assert np.array_equal(bt[:B], pos[:, 2])
        neg = bt[B:].reshape(B, K)
        assert neg.min() >= 0 and neg.max() < num_ent
        assert _false_negatives_and_repeats(pos[:, 0], pos[:, 1], neg, nrel, num_ent, true_codes) == (0, 0)
        for b in range(0, B, 97):                                         # the vectorised membership test against the dictionary itself
            assert not np.isin(neg[b], tt[(int(pos[b, 0]), int(pos[b, 1]))]).any()
    ep2, perm2 = _epoch(CompletionSampler(triples, num_ent, B, K, "cuda", seed=(11, 22)), torch.Generator(device="cuda").manual_seed(5))
    assert np.array_equal(perm, perm2) and np.array_equal(ep, ep2)       # same seed, same generator state: the same epoch
    ep3, perm3 = _epoch(CompletionSampler(triples, num_ent, B, K, "cuda", seed=(11, 23)), torch.Generator(device="cuda").manual_seed(5))
    assert np.array_equal(perm, perm3) and np.array_equal(ep[:, :2], ep3[:, :2])
    assert not np.array_equal(ep[:, 2, B:], ep3[:, 2, B:])                # another seed: other negatives


def test_the_filtered_sampler_removes_the_false_negatives_and_repeats_of_the_uniform_batches():
    """One epoch on the ja training triples at B = 1000, K = 25.  harness.completion_batches (the "uniform" mode) draws with
    replacement and only looks at the gold tail, so it is expected to hand the loss about B K (K - 1) / (2 num_ent) repeats and
    K (sum over the batch of the other true tails of (h, r)) / num_ent true tails per batch; the sampler hands it none."""
    from jmac_amd import data, harness
    from jmac_amd.sampling import CompletionSampler
    triples, num_ent = _real("ja")
    B, K, T = 1000, 25, len(triples)
    tt = data.true_tail_dict(triples)
    others = np.array([len(tt[(int(h), int(r))]) - 1 for h, r in triples[:, :2]])
    steps = T // B
    exp_repeats = steps * B * K * (K - 1) / (2.0 * num_ent)
    exp_true = steps * B * K * others.mean() / num_ent
    print("expected in one uniform epoch: %.0f repeats, %.1f true tails (%.0f %% of the triples have other true tails, longest list %d)"
          % (exp_repeats, exp_true, 100.0 * (others > 0).mean(), others.max() + 1))
    assert exp_repeats > 100 and exp_true > 1
    nrel, true_codes = _codes(triples, num_ent)
    found = [0, 0]
    for tr, neg in harness.completion_batches(triples, num_ent, B, K, torch.device("cuda"), torch.Generator(device="cuda").manual_seed(1)):
        tr, neg = tr.cpu().numpy(), neg.cpu().numpy()
        f, r = _false_negatives_and_repeats(tr[:, 0], tr[:, 1], neg, nrel, num_ent, true_codes)
        found[0] += f
        found[1] += r
    print("found in one uniform epoch: %d true tails, %d repeats" % tuple(found))
    assert found[0] + found[1] > 0
    ep, perm = _epoch(CompletionSampler(triples, num_ent, B, K, "cuda", seed=4), torch.Generator(device="cuda").manual_seed(1))
    mine = [0, 0]
    for i, (bh, br, bt) in enumerate(ep):
        f, r = _false_negatives_and_repeats(bh[:B], br[:B], bt[B:].reshape(B, K), nrel, num_ent, true_codes)
        mine[0] += f
        mine[1] += r
    assert mine[0] + mine[1] == 0


def test_a_captured_next_batch_replays_the_epoch():
    """Replaying a captured launch N times produces the N batches of N eager calls: the step words advance on the device."""
    from jmac_amd.sampling import CompletionSampler
    triples, num_ent = _real("ja")
    B, K = 1000, 25
    want, perm = _epoch(CompletionSampler(triples, num_ent, B, K, "cuda", seed=(8, 9)), torch.Generator(device="cuda").manual_seed(2))
    s = CompletionSampler(triples, num_ent, B, K, "cuda", seed=(8, 9))
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
    with pytest.raises(StopIteration):
        s.next_batch()
    # one replay too many wraps to batch 0 of the same order: nothing past perm[T) is read
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(s.batch_h.cpu().numpy(), want[0, 0]) and np.array_equal(s.batch_t[:B].cpu().numpy(), want[0, 2, :B])


def _mini_pair(capture):
    """A model, its optimizer and the inputs of train_completion_component on the (ja, en) pair of the mini dataset."""
    from jmac_amd import data, entr, harness, optim
    from jmac_amd.model import JMAC
    kgs, s_train, _, n_ent = data.load_dbp5l(MINI, "ja")
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, dropout=0.0, neg_sampler="filtered", capture_completion=capture)
    torch.manual_seed(0)
    name_emb = np.random.default_rng(0).standard_normal((n_ent, 24)).astype(np.float32)
    model = JMAC(args, name_emb, sum(kg.num_relation for kg in kgs.values()), n_ent).cuda()
    model.train()
    opt = optim.Adam(model.parameters(), lr=5e-3)
    k1, k2 = kgs["ja"], kgs["en"]
    dev = torch.device("cuda")
    (ei1, et1), (ei2, et2) = entr.align_data_processing(k1.train_data, dev), entr.align_data_processing(k2.train_data, dev)
    feed = {"links": torch.from_numpy(s_train[("ja", "en")]).to(dev),
            "ent_bases1": [k1.entity_id_base, k1.upper_entity_base], "rel_bases1": [k1.relation_id_base, k1.upper_relation_base],
            "ent_bases2": [k2.entity_id_base, k2.upper_entity_base], "rel_bases2": [k2.relation_id_base, k2.upper_relation_base]}
    return model, opt, (ei1, et1, ei2, et2, feed, k1.train_data, k2.train_data, k1.num_entity, k2.num_entity, args)


def test_a_captured_epoch_equals_the_eager_epoch_bitwise():
    """Two models from the same state, two epochs each of harness.train_completion_component with the "filtered" sampler: eager,
    and with capture_completion (three eager steps, then one captured step per side replayed; the second epoch replays only).
    The step is bitwise reproducible (tests/test_gpu_determinism.py), so losses and parameters are compared with ==."""
    from jmac_amd import harness
    runs = []
    for capture in (False, True):
        model, opt, inputs = _mini_pair(capture)
        torch.manual_seed(7)                                              # the samplers take their seed words from this generator
        gen = torch.Generator(device="cuda").manual_seed(1)
        state, losses, means = {}, [], []
        for _ in range(2):
            means.append(harness.train_completion_component(model, opt, *inputs, generator=gen, state=state))
            losses.append(state["step_losses"].clone())
        torch.cuda.synchronize()
        sides = state["completion_sides"]
        assert [len(s["sampler"]) for s in sides] == [131 // 32, (168 + 70) // 32]
        assert all((s["graph"] is not None) == capture for s in sides)
        runs.append((torch.cat(losses).cpu(), {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, means))
    (l0, p0, m0), (l1, p1, m1) = runs
    assert l0.numel() == 2 * (4 + 7) and torch.isfinite(l0).all() and (l0 > 0).all()       # every step's slot was written
    assert torch.equal(l0, l1), (l0, l1)
    assert m0 == m1
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
def test_train_two_epochs_on_mini_dataset_with_the_filtered_sampler(capture):
    """tests/test_gpu_harness.py:test_train_two_epochs_on_mini_dataset with neg_sampler="filtered" (and, captured, with the
    optimizer whose step captures): the completion loss falls and the train-split MRR rises."""
    from jmac_amd import data, harness, optim
    from jmac_amd.model import JMAC
    torch.manual_seed(0)
    kgs, s_train, s_test, n_ent = data.load_dbp5l(MINI, "ja")
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, dropout=0.0, lr=5e-3, pair_sample_weight=2.0,
                             neg_sampler="filtered", capture_completion=capture)
    rng = np.random.default_rng(0)
    name_emb = rng.standard_normal((n_ent, 24)).astype(np.float32)
    n_rel_total = sum(kg.num_relation for kg in kgs.values())
    model = JMAC(args, name_emb, n_rel_total, n_ent).cuda()
    make = optim.Adam if capture else torch.optim.Adam
    opt_c = make(model.parameters(), lr=args.lr)
    opt_a = make(model.parameters(), lr=args.lr)
    gen = torch.Generator(device="cuda").manual_seed(1)
    ja = kgs["ja"]
    ei = torch.from_numpy(ja.edge_index).cuda()
    et = torch.from_numpy(ja.edge_type).cuda()
    h1_0, h10_0, mrr_0 = harness.evaluate_completion(model, ja, ei, et, args, "train")
    state, logs = {}, []
    model.train()
    for epoch in range(6):
        logs.append(harness.train_epoch(model, kgs, s_train, s_test, opt_c, opt_a, args, state, refresh=(epoch % 3 == 0),
                                        generator=gen))
    first = np.mean([p["completion_loss"] for p in logs[0]])
    last = np.mean([p["completion_loss"] for p in logs[-1]])
    assert np.isfinite(first) and np.isfinite(last) and last < first           # the completion loss goes down
    assert all(np.isfinite(p["align_loss"]) for e in logs for p in e)
    assert logs[-1][0]["align_loss"] < logs[0][0]["align_loss"]
    h1, h10, mrr = harness.evaluate_completion(model, ja, ei, et, args, "val")
    assert 0.0 <= h1 <= h10 <= 1.0 and 0.0 < mrr <= 1.0
    _, h10_t, mrr_t = harness.evaluate_completion(model, ja, ei, et, args, "train")
    assert mrr_t > mrr_0 and h10_t >= h10_0
    assert harness.evaluate_completion(model, ja, ei, et, args, "val") == (h1, h10, mrr)
