"""GPU: the EnTr refresh with ``matrix_free=True`` (scoring.alignment_stats instead of the softmax matrices of
scoring.alignment_quality) against the reference's captured outputs (tests/golden/entr_small.npz), against the materialised
form's properties, and through harness.train_epoch."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from util import assert_close, load_golden

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbp5l_mini")


def _setup():
    g, m = load_golden("entr_small"), load_golden("model_small")
    o1, o2 = torch.from_numpy(m["emb1_align"]).cuda(), torch.from_numpy(m["emb2_align"]).cuda()
    args = types.SimpleNamespace(num_negative=5, pair_sample_weight=0.2)
    n1, n2, nrel = int(g["n1"]), int(g["n2"]), int(g["nrel"])
    bases = ([0, n1], [0, nrel], [n1, n1 + n2], [nrel, 2 * nrel])
    return g, o1, o2, args, bases


def _run(entr, g, o1, o2, args, bases, ge, gs, **kw):
    eb1, rb1, eb2, rb2 = bases
    kg1 = types.SimpleNamespace(triple_keys=entr.encode_triples(g["triples1"]))
    kg2 = types.SimpleNamespace(triple_keys=entr.encode_triples(g["triples2"]))
    return entr.seed_enlargement_triple_transferring(
        o1, o2, g["test_src"].tolist(), g["test_dst"].tolist(), ge, 0, g["links"], g["triples1"], g["triples2"], gs,
        eb1, rb1, eb2, rb2, kg1, kg2, args, matrix_free=True, **kw)


def test_first_visit_matrix_free_matches_reference_golden():
    from jmac_amd import entr
    g, o1, o2, args, bases = _setup()
    ge, gs = [-1], [g["links"]]
    n1, n2, k1, k2, feed, _ = _run(entr, g, o1, o2, args, bases, ge, gs)
    assert abs(ge[0] - float(g["entropy"])) <= 1e-5 * float(g["entropy"])
    assert np.array_equal(n1, g["new_triples1"]) and np.array_equal(n2, g["new_triples2"])
    assert np.array_equal(np.unique(k1), np.unique(entr.encode_triples(g["keys1"])))
    assert np.array_equal(np.unique(k2), np.unique(entr.encode_triples(g["keys2"])))
    assert np.array_equal(feed["links"], g["feed_links"])
    assert np.array_equal(feed["neg_left"], g["neg_left"]) and np.array_equal(feed["neg2_right"], g["neg2_right"])
    assert torch.equal(feed["neg_right"].cpu(), torch.from_numpy(g["neg_right"]))
    assert torch.equal(feed["neg2_left"].cpu(), torch.from_numpy(g["neg2_left"]))
    assert feed["ent_bases2"] == bases[2] and feed["rel_bases1"] == bases[1]


def test_enlargement_branch_matrix_free(monkeypatch):
    from jmac_amd import entr, scoring
    g, o1, o2, args, bases = _setup()
    args.pair_sample_weight = 2.0
    H = float(g["entropy"])
    ge, gs = [H * 1.25], [g["links"]]
    gen = torch.Generator(device="cuda").manual_seed(3)
    seen = {}
    real = torch.Tensor.multinomial

    def spy(self, *a, **kw):
        seen["weights"] = self.clone()
        return real(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, "multinomial", spy)
    out = _run(entr, g, o1, o2, args, bases, ge, gs, generator=gen)
    monkeypatch.undo()
    pairs = out[4]["links"]
    extra = pairs[len(g["links"]):]
    want_pairs = len(extra)
    assert want_pairs in (9, 10)
    assert len(np.unique(extra[:, 0])) == want_pairs
    assert ge[0] == H * 1.25
    _, simi, _ = scoring.alignment_quality(o1, o2, g["test_src"].tolist(), g["test_dst"].tolist())
    assert np.array_equal(simi[extra[:, 0]].argmax(1).cpu().numpy(), extra[:, 1])
    assert_close(seen["weights"], simi.max(1)[0], 1e-4, what="multinomial weights")
    assert np.array_equal(gs[0], pairs) and len(out[4]["neg_right"]) == len(pairs) * args.num_negative
    # a worse entropy resets the stored value and adds nothing (train.py:154-156)
    ge2, gs2 = [H * 0.5], [g["links"]]
    out2 = _run(entr, g, o1, o2, args, bases, ge2, gs2)
    assert abs(ge2[0] - H) <= 1e-5 * H and len(out2[4]["links"]) == len(g["links"])


def _refresh_epoch(matrix_free):
    from jmac_amd import data, harness
    from jmac_amd.model import JMAC
    torch.manual_seed(0)
    kgs, s_train, s_test, n_ent = data.load_dbp5l(ROOT, "ja")
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, dropout=0.0, lr=5e-3, pair_sample_weight=2.0,
                             entr_matrix_free=matrix_free)
    assert args.entr_matrix_free is matrix_free
    name_emb = np.random.default_rng(0).standard_normal((n_ent, 24)).astype(np.float32)
    model = JMAC(args, name_emb, sum(kg.num_relation for kg in kgs.values()), n_ent).cuda()
    opt_c = torch.optim.Adam(model.parameters(), lr=args.lr)
    opt_a = torch.optim.Adam(model.parameters(), lr=args.lr)
    gen = torch.Generator(device="cuda").manual_seed(1)
    state = {}
    model.train()
    log = harness.train_epoch(model, kgs, s_train, s_test, opt_c, opt_a, args, state, refresh=True, generator=gen)
    return log, state


def test_harness_refresh_epoch_is_the_same_either_way():
    log_a, st_a = _refresh_epoch(False)
    log_b, st_b = _refresh_epoch(True)
    assert len(log_a) == len(log_b) > 0
    for a, b in zip(log_a, log_b):
        assert a["pair"] == b["pair"] and a["links"] == b["links"] and a["triples"] == b["triples"]
        assert abs(a["entropy"] - b["entropy"]) <= 1e-5 * abs(a["entropy"])
        assert abs(a["completion_loss"] - b["completion_loss"]) <= 1e-5 * abs(a["completion_loss"]) + 1e-12
        assert abs(a["align_loss"] - b["align_loss"]) <= 1e-5 * abs(a["align_loss"]) + 1e-12
    for idx in st_a:
        fa, fb = st_a[idx]["feeddict"], st_b[idx]["feeddict"]
        assert np.array_equal(fa["links"], fb["links"])
        assert torch.equal(fa["neg_right"], fb["neg_right"]) and torch.equal(fa["neg2_left"], fb["neg2_left"])
        assert np.array_equal(st_a[idx]["tr"][0], st_b[idx]["tr"][0]) and np.array_equal(st_a[idx]["tr"][1], st_b[idx]["tr"][1])
