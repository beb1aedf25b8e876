"""CPU: the float64 reference of the link-prediction softmax statistics (tests/linkpred_stats_ref.py) against a brute-force
softmax on tiny cases, and the host side of the feature: the ABI, the ValueErrors, LinkStats' properties, the ECE binning."""
import math

import numpy as np
import pytest
import torch

import linkpred_stats_ref as R


def _tiny(seed, N=7, d=5, nl=2, B=4, nrel=3):
    rng = np.random.default_rng(seed)
    ent = [rng.standard_normal((N, d)).astype(np.float32) for _ in range(nl)]
    rel = [(0.1 * rng.standard_normal((nrel, d))).astype(np.float32) for _ in range(nl)]
    return ent, rel, rng.integers(0, N, B), rng.integers(0, nrel, B), rng


def _brute(ent, rel, h, r, scale, listed, gold, pred_head):
    """Plain Python, one query at a time: math.fsum over explicit loops."""
    out = []
    for b in range(len(h)):
        dist = []
        for n in range(ent[0].shape[0]):
            acc = 0.0
            for e, x in zip(ent, rel):
                q = (e[h[b]] - x[r[b]]) if pred_head else (e[h[b]] + x[r[b]])          # fp32
                acc += math.fsum(abs(float(a) - float(c)) for a, c in zip(q, e[n]))
            dist.append(acc)
        cset = [n for n in range(len(dist)) if n not in listed[b] or (gold is not None and n == gold[b])]
        if not cset:
            out.append(dict(nearest=-1, dist_min=math.inf, sum=0.0, entropy=0.0))
            continue
        near = min(cset, key=lambda n: (dist[n], n))
        p = [math.exp(-scale * (dist[n] - dist[near])) for n in cset]
        s = math.fsum(p)
        o = dict(nearest=near, dist_min=dist[near], sum=s, entropy=-math.fsum(x / s * math.log(x / s) for x in p if x > 0))
        if gold is not None:
            o["logp_gold"] = math.log(math.exp(-scale * (dist[gold[b]] - dist[near])) / s)
        out.append(o)
    return out


@pytest.mark.parametrize("pred_head", [False, True])
@pytest.mark.parametrize("mode", ["predict", "evaluate"])
def test_reference_equals_brute_force_softmax(mode, pred_head):
    ent, rel, h, r, rng = _tiny(3)
    N = ent[0].shape[0]
    tt = {(int(h[0]), int(r[0])): np.array([1, 4]), (int(h[1]), int(r[1])): np.arange(N)}      # a list, and everything listed
    gold = rng.integers(0, N, len(h)) if mode == "evaluate" else None
    if gold is not None:
        gold[0] = 4                                                           # a listed gold stays in its set
    listed = [set(tt.get((int(a), int(b)), [])) for a, b in zip(h, r)]
    dist = R.dist64(ent, rel, h, r, pred_head)
    got = R.stats64(dist, 0.7, R.candidates(h, r, tt, N, gold), gold)
    want = _brute(ent, rel, h, r, 0.7, listed, gold, pred_head)
    for b, w in enumerate(want):
        assert got["nearest"][b] == w["nearest"]
        for key in w:
            if key != "nearest":
                assert got[key][b] == pytest.approx(w[key], rel=1e-12, abs=1e-12), (b, key)
    if mode == "predict":
        assert got["nearest"][1] == -1 and got["sum"][1] == 0 and np.isinf(got["dist_min"][1]) and got["entropy"][1] == 0
    else:
        assert got["sum"][1] == 1 and got["logp_gold"][1] == 0 and got["nearest"][1] == gold[1]      # the gold alone


def test_reference_bf16_rounds_query_and_table():
    ent, rel, h, r, _ = _tiny(5, nl=1)
    d32, d16 = R.dist64(ent, rel, h, r), R.dist64(ent, rel, h, r, bf16=True)
    e16 = torch.from_numpy(ent[0]).to(torch.bfloat16)
    q16 = (torch.from_numpy(ent[0])[h] + torch.from_numpy(rel[0])[r]).to(torch.bfloat16)
    assert np.array_equal(d16, torch.cdist(q16.double(), e16.double(), p=1).numpy())
    assert not np.array_equal(d16, d32)


def test_reference_ensemble_fold():
    ent, rel, h, r, rng = _tiny(7)
    N = ent[0].shape[0]
    ent2 = [rng.standard_normal((5, ent[0].shape[1])).astype(np.float32) for _ in ent]
    link = np.array([2, -1, 0, 4, -1, 9, 1])                                  # 9: outside the member's rows, counts as absent
    h[0], h[1] = 0, 1                                                         # a linked and an unlinked head
    D = R.ens_dist64([(ent, rel, None, 0.25), (ent2, rel, link, 0.75)], h, r)
    d0 = R.dist64(ent, rel, h, r)
    assert np.allclose(D[1], d0[1], rtol=1e-15)                               # unlinked head: the target's distance, weights sum to 1
    d1 = R.dist64(ent2, rel, [2], [r[0]])[0]
    for n in range(N):
        want = 0.25 * d0[0, n] + 0.75 * (d1[link[n]] if 0 <= link[n] < 5 else d0[0, n])
        assert D[0, n] == pytest.approx(want, rel=1e-14)
    one = R.ens_dist64([(ent, rel, None, 1.0)], h, r)
    assert np.array_equal(one, d0)


def test_scale_pickers_reach_both_regimes():
    ent, rel, h, r, _ = _tiny(11, N=65, d=20, B=16)
    dist = R.dist64(ent, rel, h, r)
    cand = R.candidates(h, r, {}, 65)
    s1, s2 = R.spread_scale(dist, cand), R.peaked_scale(dist, cand)
    assert s1 is not None and s2 is not None and s1 < s2
    assert 1.0 <= np.median(R.stats64(dist, s1, cand)["entropy"]) <= np.log(65) - 1
    assert np.median(1 / R.stats64(dist, s2, cand)["sum"]) > 0.99


def test_abi_has_the_statistics_entry_points():
    from jmac_amd import _lib
    L = _lib.lib()
    assert L.jmac_version() >= 140
    for name in ("jmac_linkpred_stats_workspace_bytes", "jmac_linkpred_stats_f32", "jmac_linkpred_stats_bf16",
                 "jmac_linkpred_ens_stats_workspace_bytes", "jmac_linkpred_ens_stats_f32"):
        assert name in _lib._SIGS and hasattr(L, name)
    B, N, d, nl = 8633, 11805, 300, 2
    ws = L.jmac_linkpred_stats_workspace_bytes(B, N, d, nl)
    rank = L.jmac_linkpred_rank_workspace_bytes(B, d, nl)
    parts = (N + 63) // 64
    assert rank + parts * B * 16 <= ws <= rank + parts * B * 16 + 64 * B + 4096 and ws < B * N       # never B x N
    assert L.jmac_linkpred_ens_stats_workspace_bytes(B, N, d, nl, 3) > L.jmac_linkpred_ens_rank_workspace_bytes(B, d, nl, 3)
    assert L.jmac_linkpred_stats_workspace_bytes(B, 0, d, nl) == 0


def test_argument_errors_need_no_device():
    """The checks that come before any pointer is read: sizes, the scale, logp_gold without gold, the workspace."""
    import ctypes
    from jmac_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                                                  # never dereferenced by the calls below
    lay = (_lib.LinkLayer * 5)()

    def call(nl=1, d=8, scale=1.0, gold=None, near=p, logp=None, ws=p, ws_bytes=1 << 30, fn=L.jmac_linkpred_stats_f32):
        return fn(lay, nl, p, p, 0, gold, None, 4, 10, d, scale, near, None, None, None, logp, ws, ws_bytes, None)

    for fn in (L.jmac_linkpred_stats_f32, L.jmac_linkpred_stats_bf16):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(scale=bad, fn=fn) == -1
        assert call(logp=p, fn=fn) == -1                                      # logp_gold without gold
        assert call(near=None, fn=fn) == -1                                   # no output at all
        assert call(nl=5, fn=fn) == -1
        assert call(d=516, fn=fn) == -4
        assert call(ws_bytes=L.jmac_linkpred_stats_workspace_bytes(4, 10, 8, 1) - 1, fn=fn) == -3
        assert call(ws=None, fn=fn) == -3
    mem = (_lib.LinkMember * 1)()
    mem[0] = _lib.LinkMember(lay, None, 10, 1.0)

    def ens(nl=1, d=8, scale=1.0, logp=None, ws_bytes=1 << 30, ng=1):
        return L.jmac_linkpred_ens_stats_f32(mem, ng, nl, p, p, 0, None, None, 4, 10, d, scale, p, None, None, None, logp, p, ws_bytes, None)

    assert ens(scale=0.0) == -1 and ens(scale=float("nan")) == -1 and ens(logp=p) == -1 and ens(nl=5) == -1 and ens(ng=5) == -1
    assert ens(d=516) == -4


def test_host_side_value_errors():
    from jmac_amd import scoring
    ent, rel = [torch.zeros(4, 8)], [torch.zeros(2, 8)]
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            scoring.linkpred_stats(ent, rel, [0], [0], bad)
        with pytest.raises(ValueError):
            scoring.linkpred_stats_ensemble([(ent, rel, None, 1.0)], [0], [0], bad)
        with pytest.raises(ValueError):
            scoring.linkpred_topk_prob(ent, rel, [0], [0], 1, bad)
        with pytest.raises(ValueError):
            scoring.linkpred_topk_prob_ensemble([(ent, rel, None, 1.0)], [0], [0], 1, bad)


def test_linkstats_properties():
    from jmac_amd.scoring import LinkStats
    st = LinkStats(torch.tensor([3, -1]), torch.tensor([2.0, float("inf")]), torch.tensor([4.0, 0.0]), torch.tensor([0.5, 0.0]),
                   None, 0.5)
    assert st.confidence.tolist() == [0.25, 0.0]
    assert st.lse[0].item() == pytest.approx(-1.0 + math.log(4.0)) and st.lse[1].item() == -math.inf
    assert st.logp_gold is None and st.scale == 0.5 and st._fields[0] == "nearest"


def test_calibration_error_bins():
    from jmac_amd.harness import calibration_error
    # bins [0.2, 0.3): two queries, one right; [0.9, 1.0]: three queries (1.0 falls into the last bin), two right; the rest empty
    conf = torch.tensor([0.25, 0.25, 0.95, 0.95, 1.0])
    hit = torch.tensor([True, False, True, True, False])
    want = (2 * abs(0.5 - 0.25) + 3 * abs(2 / 3 - (0.95 + 0.95 + 1.0) / 3)) / 5
    assert calibration_error(conf, hit).item() == pytest.approx(want, abs=1e-7)
    assert R.ece(conf.numpy(), hit.numpy()) == pytest.approx(want, abs=1e-7)
    assert calibration_error(torch.tensor([0.05, 0.15]), torch.tensor([False, False])).item() == pytest.approx(0.1, abs=1e-7)
    assert calibration_error(torch.zeros(0), torch.zeros(0, dtype=torch.bool)).item() == 0.0
