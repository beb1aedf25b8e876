"""GPU: link-prediction confidence -- scoring.linkpred_stats / linkpred_stats_ensemble / linkpred_topk_prob (jmac_linkpred_stats_*,
jmac_linkpred_ens_stats_f32): the softmax statistics of -scale * dist over the tails of every query, without the [B, N] matrix.

Two kinds of check.  Against FLOAT64 (tests/linkpred_stats_ref.py) with a derived tolerance: a distance is a sequential fp32 sum
of m = layers * d * members non-negative terms, error below DELTA = (m + 2) 2^-24 max dist; a logit moves by at most scale *
DELTA, so log(sum), logp_gold and the log-sum-exp are held to 1e-4 + 2 scale DELTA (1e-4: the project's parity tolerance, the
bound jmac_sim_lse_f32 is held to) and the entropy to 1e-4 + 2 log(N) scale DELTA (its first-order sensitivity to a logit
perturbation).  The scales come from the reference per case: one with a median entropy in [1, log N - 1] (the sums matter) and
one with a median top-1 probability above 0.99; both regimes are asserted on the reference.  EXACT, device against device: the
nearest candidate and its distance are linkpred_topk's first column, nearest == gold exactly where the filtered rank is 1 and
logp_gold == -log(sum) there, two calls and any batch composition give the same bits, one member with weight 1 is the single-KG
call.

Measured maxima are printed per case (run with -s); the figures of the run that accompanied the feature are in DESIGN section 5."""
import dataclasses
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import linkpred_stats_ref as R
from conftest import GOLDEN

# (B, N, d, layers, bf16): single candidate; part boundary with the vector loader; scalar loader, ragged; 33 parts with a ragged
# last one; 129 parts through every lane of the merge and three row tiles; the bf16 form
CASES = {
    "one_b1": (1, 1, 20, 1, False), "one_b5": (5, 1, 20, 1, False),
    "n63": (70, 63, 300, 2, False), "n64": (70, 64, 300, 2, False), "n65": (70, 65, 300, 2, False),
    "scalar": (70, 200, 30, 1, False), "parts33": (70, 2100, 64, 2, False), "parts129": (130, 8200, 16, 1, False),
    "bf16": (70, 2100, 64, 2, True),
}
NREL = 11


def _index(tt):
    from jmac_amd.sampling import TrueTailIndex
    return TrueTailIndex.from_dict(tt, "cuda") if tt else None


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the float64 distances of a case, computed once and shared (read-only) by the tests."""
    B, N, d, nl, bf16 = CASES[name]
    seed = sorted(CASES).index(name) + 100
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    ent = [torch.randn(N, d, generator=gen) for _ in range(nl)]
    rel = [0.1 * torch.randn(NREL, d, generator=gen) for _ in range(nl)]
    h, r, gold = rng.integers(0, N, B), rng.integers(0, NREL, B), rng.integers(0, N, B)
    gold[::7] = h[::7]                                                      # golds that are the nearest candidate: the head itself
    tt = {}
    if N == 1:                                                              # distinct keys; the odd queries' lists hold the one candidate
        r = np.arange(B) % NREL
    for b, (hb, rb) in enumerate(zip(h[: B - B // 5], r)):                  # the last fifth of the queries: absent keys
        if (int(hb), int(rb)) not in tt and (N > 1 or b % 2):
            n = int(rng.integers(1, 40))
            tt[(int(hb), int(rb))] = np.sort(rng.choice(N, min(n, N), replace=False))
    dist = R.dist64([e.numpy() for e in ent], [x.numpy() for x in rel], h, r, bf16=bf16)
    dist.setflags(write=False)
    return dict(B=B, N=N, d=d, nl=nl, bf16=bf16, ent=[e.cuda() for e in ent], rel=[x.cuda() for x in rel], h=h, r=r, gold=gold, tt=tt,
                dist=dist, dtype=torch.bfloat16 if bf16 else torch.float32)


def _np(st):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in st._asdict().items() if k != "scale"}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    for x, y in zip(a[:5], b[:5]):
        if x is None or y is None:
            assert x is None and y is None
        else:
            assert torch.equal(_bits(x), _bits(y))


def _tolerances(c, scale, dist, members=1):
    dl = R.delta(dist, c["nl"], c["d"], members)
    return 1e-4 + 2 * scale * dl, 1e-4 + 2 * math.log(c["N"]) * scale * dl


def _check_float64(tag, got, ref, tol, tol_ent, rows=None):
    """log(sum), the log-sum-exp, logp_gold and the entropy against the reference; the nearest on the decided rows."""
    rows = np.ones(len(ref["sum"]), dtype=bool) if rows is None else rows
    some = rows & (ref["sum"] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_sum = np.abs(np.log(got["sum"].astype(np.float64)) - ref["log_sum"])[some].max(initial=0.0)
        lse = -got["scale"] * got["dist_min"].astype(np.float64) + np.log(got["sum"].astype(np.float64))
        e_lse = np.abs(lse - ref["lse"])[some].max(initial=0.0)
    e_ent = np.abs(got["entropy"] - ref["entropy"])[rows].max(initial=0.0)
    e_lp = np.abs(got["logp_gold"] - ref["logp_gold"])[rows].max(initial=0.0) if "logp_gold" in ref else 0.0
    with np.errstate(invalid="ignore"):
        decided = rows & ((ref["second"] - ref["dist_min"]) >= 1e-4 * np.abs(ref["dist_min"]))
    decided |= rows & ~(ref["sum"] > 0) | rows & np.isinf(ref["second"])      # an empty set or a single candidate: nothing to decide
    print("%s: |log sum| %.2e |lse| %.2e |logp| %.2e (tol %.2e)  |entropy| %.2e (tol %.2e)  undecided %d of %d"
          % (tag, e_sum, e_lse, e_lp, tol, e_ent, tol_ent, int((rows & ~decided).sum()), int(rows.sum())))
    assert e_sum <= tol and e_lse <= tol and e_lp <= tol and e_ent <= tol_ent
    assert (rows & ~decided).sum() <= 0.02 * rows.sum()
    assert (got["nearest"][decided] == ref["nearest"][decided]).all()
    empty = rows & ~(ref["sum"] > 0)
    assert (got["nearest"][empty] == -1).all() and np.isinf(got["dist_min"][empty]).all() and (got["sum"][empty] == 0).all()
    assert (got["entropy"][empty] == 0).all()


def _scales(c, cand):
    """{"spread": scale, "peaked": scale} from the reference, each regime asserted on the reference (a single candidate has no
    spread regime: its entropy is 0 at every scale)."""
    out = {"peaked": R.peaked_scale(c["dist"], cand)}
    assert out["peaked"] is not None
    assert np.median(1.0 / np.maximum(R.stats64(c["dist"], out["peaked"], cand)["sum"], 1.0)) > 0.99
    if c["N"] > 1:
        out["spread"] = R.spread_scale(c["dist"], cand)
        assert out["spread"] is not None
        assert 1.0 <= np.median(R.stats64(c["dist"], out["spread"], cand)["entropy"]) <= math.log(c["N"]) - 1.0
    return out


# ---- against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["predict", "evaluate"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_stats_match_float64(name, mode):
    from jmac_amd import scoring
    c = _case(name)
    gold = c["gold"] if mode == "evaluate" else None
    cand = R.candidates(c["h"], c["r"], c["tt"], c["N"], gold)
    index = _index(c["tt"])
    for regime, scale in _scales(c, cand).items():
        st = scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], scale, gold=gold, index=index, table_dtype=c["dtype"])
        assert st.nearest.dtype == torch.int64 and st.sum.dtype == torch.float32 and (st.logp_gold is None) == (gold is None)
        got = dict(_np(st), scale=st.scale)
        if gold is None:
            got.pop("logp_gold")
        ref = R.stats64(c["dist"], scale, cand, gold)
        tol, tol_ent = _tolerances(c, scale, c["dist"])
        _check_float64("%s %s %s scale %.4g" % (name, mode, regime, scale), got, ref, tol, tol_ent)
        assert (got["sum"][ref["sum"] > 0] >= 1.0).all()
        lse = st.lse.cpu().numpy().astype(np.float64)
        ok = ref["sum"] > 0
        assert np.abs(lse[ok] - ref["lse"][ok]).max(initial=0.0) <= tol + 1e-6 * np.abs(ref["lse"][ok]).max(initial=0.0)
        conf = st.confidence.cpu().numpy()
        assert np.allclose(conf[ok], 1.0 / got["sum"][ok], rtol=1e-6) and (conf[~ok] == 0).all()


# ---- exact, device against device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_b5", "n64", "n65", "scalar", "parts33", "parts129", "bf16"])
def test_exact_identities(name):
    from jmac_amd import scoring
    c = _case(name)
    index = _index(c["tt"])
    kw = dict(index=index, table_dtype=c["dtype"])
    cand = R.candidates(c["h"], c["r"], c["tt"], c["N"])
    scale = _scales(c, cand).get("spread", 1.0)
    # prediction mode: the nearest candidate and its distance are the top-k call's first column, bit for bit
    st = scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], scale, **kw)
    idx, val = scoring.linkpred_topk(c["ent"], c["rel"], c["h"], c["r"], 1, **kw)
    assert torch.equal(st.nearest, idx[:, 0]) and torch.equal(_bits(st.dist_min), _bits(val[:, 0]))
    _same_bits(st, scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], scale, **kw))                  # two calls
    # evaluation mode: rank 1 exactly where the nearest is the gold, and there logp_gold is -log(sum) bit for bit
    ev = scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], scale, gold=c["gold"], **kw)
    _same_bits(ev, scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], scale, gold=c["gold"], **kw))
    rk = scoring.linkpred_ranks(c["ent"], c["rel"], c["h"], c["r"], c["gold"], index=index, table_dtype=c["dtype"])
    gold = torch.from_numpy(c["gold"]).cuda()
    first = ev.nearest == gold
    assert torch.equal(rk == 1, first)
    # (-log(sum) as the header defines it: the correctly rounded fp32 logarithm, i.e. float64 log rounded once)
    want = torch.from_numpy(-np.log(ev.sum.cpu().numpy().astype(np.float64)).astype(np.float32)).cuda()
    ulp = (_bits(ev.logp_gold)[first].long() - _bits(want)[first].long()).abs().max().item() if first.any() else 0
    print("%s: %d of %d golds nearest, logp_gold against -log(sum): %d ulp" % (name, int(first.sum()), len(gold), ulp))
    assert torch.equal(_bits(ev.logp_gold)[first], _bits(want)[first])
    assert (ev.logp_gold <= 0).all() and (ev.sum >= 1).all()
    # a query alone, in the batch, and in a batch in another order
    perm = np.random.default_rng(5).permutation(c["B"])
    sh = scoring.linkpred_stats(c["ent"], c["rel"], c["h"][perm], c["r"][perm], scale, gold=c["gold"][perm], **kw)
    for f in range(5):
        assert torch.equal(_bits(sh[f]), _bits(ev[f][torch.from_numpy(perm).cuda()]))
    for b in (0, c["B"] - 1):
        one = scoring.linkpred_stats(c["ent"], c["rel"], c["h"][b:b + 1], c["r"][b:b + 1], scale, gold=c["gold"][b:b + 1], **kw)
        for f in range(5):
            assert torch.equal(_bits(one[f]), _bits(ev[f][b:b + 1]))
    # one member with weight 1: the single-KG call's bits
    if not c["bf16"]:
        members = [(c["ent"], c["rel"], None, 1.0)]
        _same_bits(scoring.linkpred_stats_ensemble(members, c["h"], c["r"], scale, gold=c["gold"], index=index), ev)
        _same_bits(scoring.linkpred_stats_ensemble(members, c["h"], c["r"], scale, index=index), st)


@pytest.mark.parametrize("name", ["one_b5", "n63", "n64"])
def test_topk_prob_sums_to_one(name):
    from jmac_amd import scoring
    c = _case(name)
    cand = R.candidates(c["h"], c["r"], {}, c["N"])
    for scale in _scales(c, cand).values():
        idx, dist, prob = scoring.linkpred_topk_prob(c["ent"], c["rel"], c["h"], c["r"], c["N"], scale)
        assert prob.shape == (c["B"], c["N"]) and (idx >= 0).all()
        assert (prob.double().sum(1) - 1.0).abs().max().item() <= 1e-5
        assert torch.equal(prob[:, 0], scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], scale).confidence)
        pe = scoring.linkpred_topk_prob_ensemble([(c["ent"], c["rel"], None, 1.0)], c["h"], c["r"], c["N"], scale)
        assert torch.equal(pe[0], idx) and torch.equal(pe[2], prob)


def test_topk_prob_pads_with_zero():
    from jmac_amd import scoring
    c = _case("scalar")
    h, r = c["h"][:3], c["r"][:3]
    tt = {(int(h[0]), int(r[0])): np.arange(c["N"]), (int(h[1]), int(r[1])): np.arange(2, c["N"])}     # nothing left; two left
    idx, dist, prob = scoring.linkpred_topk_prob(c["ent"], c["rel"], h, r, 4, 0.05, index=_index(tt))
    assert (idx[0] == -1).all() and (prob[0] == 0).all()
    assert (idx[1, 2:] == -1).all() and (prob[1, 2:] == 0).all() and abs(prob[1, :2].sum().item() - 1.0) <= 1e-5
    assert (idx[2] >= 0).all() and 0 < prob[2].sum().item() <= 1.0 + 1e-5


# ---- exclusions: the masking exists for these -----------------------------------------------------------------------------------
def test_exclusion_lists():
    """Absent keys, a list that covers one whole 64-column part, a list of >= 300 entries across many parts, a list of all N (the
    empty set in prediction mode, the gold alone in evaluation mode)."""
    from jmac_amd import scoring
    c = _case("parts33")
    N, h, r, gold = c["N"], c["h"][:8].copy(), c["r"][:8].copy(), c["gold"][:8].copy()
    h[:4] = [3, 4, 5, 6]                                                      # distinct keys for the four hand-made lists
    rng = np.random.default_rng(9)
    tt = {(3, int(r[0])): np.arange(64, 128),                                 # one whole part
          (4, int(r[1])): np.sort(rng.choice(N, 320, replace=False)),         # many entries, many parts
          (5, int(r[2])): np.arange(N),                                       # everything
          (6, int(r[3])): np.array([6, 2099])}                                # the head itself and the last column
    gold[0], gold[1] = 100, int(tt[(4, int(r[1]))][7])                        # listed golds
    assert all((int(a), int(b)) not in tt for a, b in zip(h[4:], r[4:]))      # absent keys
    dist = R.dist64([e.cpu().numpy() for e in c["ent"]], [x.cpu().numpy() for x in c["rel"]], h, r)
    index = _index(tt)
    for g in (None, gold):
        cand = R.candidates(h, r, tt, N, g)
        for scale in (R.spread_scale(dist, cand), R.peaked_scale(dist, cand)):
            st = scoring.linkpred_stats(c["ent"], c["rel"], h, r, scale, gold=g, index=index)
            got = dict(_np(st), scale=scale)
            if g is None:
                got.pop("logp_gold")
            tol, tol_ent = _tolerances(c, scale, dist)
            _check_float64("lists %s scale %.4g" % ("predict" if g is None else "evaluate", scale), got, R.stats64(dist, scale, cand, g),
                           tol, tol_ent)
            if g is None:
                assert got["nearest"][2] == -1 and got["sum"][2] == 0 and np.isinf(got["dist_min"][2]) and got["entropy"][2] == 0
                idx, val = scoring.linkpred_topk(c["ent"], c["rel"], h, r, 1, index=index)
                assert torch.equal(st.nearest, idx[:, 0]) and torch.equal(_bits(st.dist_min), _bits(val[:, 0]))
            else:
                assert got["nearest"][2] == gold[2] and got["sum"][2] == 1.0 and got["logp_gold"][2] == 0.0 and got["entropy"][2] == 0.0
                assert not np.isin(got["nearest"][0], np.setdiff1d(tt[(3, int(r[0]))], [100]))


def test_masked_before_the_reduction_not_subtracted_after():
    """The cancellation case: the listed tails are copies of the query row (dist = 0 exactly) and the scale puts every unlisted
    logit <= -40 relative to them.  The statistics over the unlisted set are met at the usual tolerance; the subtract-afterwards
    form -- logsumexp over everything, then the listed mass taken out -- evaluated in fp32 misses them."""
    from jmac_amd import scoring
    c = _case("parts33")
    N, nl = c["N"], c["nl"]
    h, r = c["h"][:6].copy(), c["r"][:6].copy()
    listed = np.array([3, 64, 700, 1500, 2099])
    h[0] = 10
    h[1:] = np.where(np.isin(h[1:], listed), 11, h[1:])                       # no other query's head row is overwritten below
    ent = [e.clone() for e in c["ent"]]
    for l in range(nl):
        ent[l][listed] = ent[l][10] + c["rel"][l][int(r[0])]                  # fp32, the prep kernel's query row
    tt = {(10, int(r[0])): listed}
    dist = R.dist64([e.cpu().numpy() for e in ent], [x.cpu().numpy() for x in c["rel"]], h, r)
    assert (dist[0, listed] == 0).all()
    cand = R.candidates(h, r, tt, N)
    scale = 45.0 / dist[0][cand[0]].min()
    assert (-scale * dist[0][cand[0]]).max() <= -40.0
    ref = R.stats64(dist, scale, cand)
    st = scoring.linkpred_stats(ent, c["rel"], h, r, scale, index=_index(tt))
    tol, tol_ent = _tolerances(c, scale, dist)
    got = _np(st)
    lse = -scale * float(got["dist_min"][0]) + math.log(float(got["sum"][0]))
    print("cancellation: lse %.6f reference %.6f (tol %.2e), nearest %d" % (lse, ref["lse"][0], tol, got["nearest"][0]))
    assert abs(lse - ref["lse"][0]) <= tol and abs(math.log(float(got["sum"][0])) - ref["log_sum"][0]) <= tol
    assert abs(float(got["entropy"][0]) - ref["entropy"][0]) <= tol_ent and got["nearest"][0] == ref["nearest"][0]
    # subtract afterwards, in fp32: the listed mass rounds to the whole and nothing is left
    z = torch.from_numpy((-scale * dist[0]).astype(np.float32))
    lse_all = torch.logsumexp(z, 0)
    mass_listed = torch.exp(z[torch.from_numpy(listed)] - lse_all).sum()
    sub = (lse_all + torch.log1p(-mass_listed)).item()
    print("subtract-afterwards form in fp32: %r" % sub)
    assert not abs(sub - ref["lse"][0]) <= tol


# ---- ensemble -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred_head", [False, True])
def test_ensemble_matches_float64(pred_head):
    from jmac_amd import scoring
    N, rows, d, nl, B = 200, 150, 64, 1, 70
    gen = torch.Generator().manual_seed(77)
    rng = np.random.default_rng(77)
    ent = [[torch.randn(n, d, generator=gen) for _ in range(nl)] for n in (N, rows)]
    rel = [[0.1 * torch.randn(NREL, d, generator=gen) for _ in range(nl)] for _ in range(2)]
    link = np.full(N, -1, dtype=np.int64)
    src = rng.choice(N, N // 2, replace=False)                                # about half the links missing
    link[src] = rng.choice(rows, N // 2, replace=False)
    h, r, gold = rng.integers(0, N, B), rng.integers(0, NREL, B), rng.integers(0, N, B)
    assert (link[h] >= 0).any() and (link[h] < 0).any()
    tt = {(int(a), int(b)): np.sort(rng.choice(N, 12, replace=False)) for a, b in zip(h[:50], r[:50])}
    w = (0.6, 0.4)
    dev = [([e.cuda() for e in ent[0]], [x.cuda() for x in rel[0]], None, w[0]),
           ([e.cuda() for e in ent[1]], [x.cuda() for x in rel[1]], torch.from_numpy(link).cuda(), w[1])]
    ref_m = [([e.numpy() for e in ent[0]], [x.numpy() for x in rel[0]], None, w[0]),
             ([e.numpy() for e in ent[1]], [x.numpy() for x in rel[1]], link, w[1])]
    D = R.ens_dist64(ref_m, h, r, pred_head)
    assert not np.allclose(D, R.ens_dist64(ref_m, h, r, not pred_head))       # the sign matters
    c = dict(N=N, d=d, nl=nl)
    index = _index(tt)
    for g in (None, gold):
        cand = R.candidates(h, r, tt, N, g)
        for scale in (R.spread_scale(D, cand), R.peaked_scale(D, cand)):
            assert scale is not None
            st = scoring.linkpred_stats_ensemble(dev, h, r, scale, gold=g, index=index, pred_head=pred_head)
            got = dict(_np(st), scale=scale)
            if g is None:
                got.pop("logp_gold")
            tol, tol_ent = _tolerances(c, scale, D, members=2)
            _check_float64("ensemble pred_head=%s scale %.4g" % (pred_head, scale), got, R.stats64(D, scale, cand, g), tol, tol_ent)
    idx, val = scoring.linkpred_topk_ensemble(dev, h, r, 1, index=index, pred_head=pred_head)
    st = scoring.linkpred_stats_ensemble(dev, h, r, 0.05, index=index, pred_head=pred_head)
    assert torch.equal(st.nearest, idx[:, 0]) and torch.equal(_bits(st.dist_min), _bits(val[:, 0]))
    rk = scoring.linkpred_ranks_ensemble(dev, h, r, gold, index=index, pred_head=pred_head)
    ev = scoring.linkpred_stats_ensemble(dev, h, r, 0.05, gold=gold, index=index, pred_head=pred_head)
    assert torch.equal(rk == 1, ev.nearest == torch.from_numpy(gold).cuda())


# ---- model and harness ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ja_model():
    from jmac_amd import data, harness
    from jmac_amd.model import JMAC
    kgs, _, _, n_ent = data.kgs_from_arrays(data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz")), "ja")
    torch.manual_seed(0)
    args = harness.make_args(dim=32, batch_size=256, num_negative=5, dropout=0.0)
    name_emb = np.random.default_rng(0).standard_normal((n_ent, 24)).astype(np.float32)
    model = JMAC(args, name_emb, sum(kg.num_relation for kg in kgs.values()), n_ent).cuda()
    ja = kgs["ja"]
    sub = dataclasses.replace(ja, val_data=ja.val_data[:500])                 # the first 500 validation queries, the real index
    ei, et = torch.from_numpy(ja.edge_index).cuda(), torch.from_numpy(ja.edge_type).cuda()
    model.eval()
    with torch.no_grad():
        cached = model.forward_base(ei, et, [ja.entity_id_base, ja.upper_entity_base], [ja.relation_id_base, ja.upper_relation_base])
    layers = range(args.num_gcn_layer)
    ent, rel = [cached[1][l] for l in layers], [cached[2][l] for l in layers]
    q = sub.val_data
    dist = R.dist64([e.cpu().numpy() for e in ent], [x.cpu().numpy() for x in rel], q[:, 0], q[:, 1])
    cand = R.candidates(q[:, 0], q[:, 1], ja.true_tail, ja.num_entity, q[:, 2])
    return dict(model=model, kg=sub, ei=ei, et=et, args=args, ent=ent, rel=rel, dist=dist, cand=cand, cached=cached)


def test_evaluate_completion_confidence_on_the_real_ja_kg():
    from jmac_amd import harness
    m = _ja_model()
    q, N = m["kg"].val_data, m["kg"].num_entity
    scale = R.spread_scale(m["dist"], m["cand"])
    assert scale is not None
    ref = R.stats64(m["dist"], scale, m["cand"], q[:, 2])
    got = harness.evaluate_completion_confidence(m["model"], m["kg"], m["ei"], m["et"], m["args"], scale, split="val")
    assert sorted(got) == ["confidence", "ece", "entropy", "hits1", "nll"]
    c = dict(N=N, d=m["ent"][0].shape[1], nl=len(m["ent"]))
    tol, tol_ent = _tolerances(c, scale, m["dist"])
    conf64 = 1.0 / ref["sum"]
    hit64 = ref["nearest"] == q[:, 2]
    undecided = ((ref["second"] - ref["dist_min"]) < 1e-4 * np.abs(ref["dist_min"])).sum()
    print("ja: scale %.4g nll %.6f (ref %.6f) entropy %.6f (ref %.6f) confidence %.6f (ref %.6f) hits1 %.4f (ref %.4f) ece %.6f (ref %.6f)"
          % (scale, got["nll"], -ref["logp_gold"].mean(), got["entropy"], ref["entropy"].mean(), got["confidence"], conf64.mean(),
             got["hits1"], hit64.mean(), got["ece"], R.ece(conf64, hit64)))
    assert abs(got["nll"] + ref["logp_gold"].mean()) <= tol and abs(got["entropy"] - ref["entropy"].mean()) <= tol_ent
    assert abs(got["hits1"] - hit64.mean()) <= undecided / len(q) + 1e-12 and undecided <= 0.02 * len(q)
    assert abs(got["confidence"] - conf64.mean()) <= tol                      # |d(1/sum)| <= |d log sum| for sum >= 1
    assert 0.0 <= got["ece"] <= 1.0
    hits1 = harness.evaluate_completion(m["model"], m["kg"], m["ei"], m["et"], m["args"], "val", filtered=True, fused=True)[0]
    assert got["hits1"] == hits1
    assert harness.evaluate_completion_confidence(m["model"], m["kg"], m["ei"], m["et"], m["args"], scale, eval_batch=130) == got


def test_calibrate_link_scale_returns_the_arg_min_of_its_table():
    from jmac_amd import harness
    m = _ja_model()
    s0 = R.spread_scale(m["dist"], m["cand"])
    scales = [s0 * f for f in (0.25, 0.5, 1.0, 2.0, 4.0)]
    best, table = harness.calibrate_link_scale(m["model"], m["kg"], m["ei"], m["et"], m["args"], scales, split="val")
    assert sorted(table) == sorted(scales) and best in table
    assert all(table[best] <= v for v in table.values()) and all(math.isfinite(v) and v > 0 for v in table.values())
    one = harness.evaluate_completion_confidence(m["model"], m["kg"], m["ei"], m["et"], m["args"], best)
    assert one["nll"] == table[best]


def test_model_methods_honour_the_table_dtype(monkeypatch):
    from jmac_amd import scoring
    m = _ja_model()
    model, kg = m["model"], m["kg"]
    model.eval()
    q = kg.val_data[:64]
    eb, rb = [kg.entity_id_base, kg.upper_entity_base], [kg.relation_id_base, kg.upper_relation_base]
    index = _index(kg.true_tail)
    real, seen = scoring.lib(), []

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(scoring, "lib", lambda: Spy())
    args = (m["ei"], m["et"], eb, rb)
    with torch.no_grad():
        f32 = model.linkpred_stats(q[:, 0], q[:, 1], 0.1, *args, gold=q[:, 2], index=index, cached=m["cached"])
        assert "jmac_linkpred_stats_f32" in seen and "jmac_linkpred_stats_bf16" not in seen
        _same_bits(f32, scoring.linkpred_stats(m["ent"], m["rel"], q[:, 0], q[:, 1], 0.1, gold=q[:, 2], index=index))
        _same_bits(f32, model.linkpred_stats(q[:, 0], q[:, 1], 0.1, *args, gold=q[:, 2], index=index))          # encodes itself
        model.set_table_dtype(torch.bfloat16)
        try:
            del seen[:]
            b16 = model.linkpred_stats(q[:, 0], q[:, 1], 0.1, *args, gold=q[:, 2], index=index, cached=m["cached"])
            assert "jmac_linkpred_stats_bf16" in seen and "jmac_linkpred_stats_f32" not in seen
            _same_bits(b16, scoring.linkpred_stats(m["ent"], m["rel"], q[:, 0], q[:, 1], 0.1, gold=q[:, 2], index=index,
                                                   table_dtype=torch.bfloat16))
            idx, dist, prob = model.linkpred_topk_prob(q[:, 0], q[:, 1], 5, 0.1, *args, index=index, cached=m["cached"])
            assert "jmac_linkpred_topk_bf16" in seen and prob.shape == (64, 5) and (prob.sum(1) <= 1 + 1e-5).all()
        finally:
            model.set_table_dtype(torch.float32)
        blocks = [(m["ei"], m["et"], eb, rb)]
        ens = model.linkpred_stats_ensemble(q[:, 0], q[:, 1], 0.1, blocks, [], (1.0,), gold=q[:, 2], index=index, cached=[m["cached"]])
        _same_bits(ens, f32)
        pe = model.linkpred_topk_prob_ensemble(q[:, 0], q[:, 1], 5, 0.1, blocks, [], (1.0,), index=index, cached=[m["cached"]])
        ps = model.linkpred_topk_prob(q[:, 0], q[:, 1], 5, 0.1, *args, index=index, cached=m["cached"])
        assert torch.equal(pe[0], ps[0]) and torch.equal(pe[2], ps[2])


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors():
    import ctypes
    from jmac_amd import _lib, scoring
    c = _case("scalar")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], bad)
    with pytest.raises(ValueError):
        scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"][:-1], 1.0)
    with pytest.raises(IndexError):
        scoring.linkpred_stats(c["ent"], c["rel"], c["h"], c["r"], 1.0, gold=np.full(c["B"], c["N"]))
    with pytest.raises(ValueError):
        scoring.linkpred_stats([c["ent"][0]] * 5, [c["rel"][0]] * 5, c["h"], c["r"], 1.0)
    wide = [torch.zeros(8, 516, device="cuda")], [torch.zeros(2, 516, device="cuda")]
    with pytest.raises(_lib.JmacError):
        scoring.linkpred_stats(wide[0], wide[1], [0], [0], 1.0)
    # the C level, on real buffers
    L = _lib.lib()
    arr, keep, N, d = scoring._link_layers(c["ent"], c["rel"], False)
    h = torch.from_numpy(c["h"]).int().cuda()
    r = torch.from_numpy(c["r"]).int().cuda()
    B = h.numel()
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    nbytes = L.jmac_linkpred_stats_workspace_bytes(B, N, d, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call(nl=1, dd=d, scale=1.0, gold=None, logp=None, ws_bytes=nbytes):
        return L.jmac_linkpred_stats_f32(arr, nl, h.data_ptr(), r.data_ptr(), 0, gold, None, B, N, dd, scale, None, None, out.data_ptr(),
                                         None, logp, ws.data_ptr(), ws_bytes, _lib.stream())

    assert call() == 0
    assert call(logp=out.data_ptr()) == -1                                    # logp_gold without gold
    assert call(scale=0.0) == -1 and call(scale=float("nan")) == -1 and call(scale=float("inf")) == -1 and call(scale=-3.0) == -1
    assert call(ws_bytes=nbytes - 1) == -3
    assert call(nl=5) == -1 and call(dd=516) == -4
    torch.cuda.synchronize()
