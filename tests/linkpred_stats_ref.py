"""Float64 restatement of the link-prediction softmax statistics for the tests (not a test itself).  The definition is
include/jmac_hip.h's (jmac_linkpred_stats_*): logits z = -scale * dist over the candidate set C_b -- the n the index does not
list, plus the gold in evaluation mode -- and per query the nearest candidate, its distance, sum exp(z - zmax), the entropy and
the gold's log-probability.

The query rows are formed in fp32 as the prep kernel forms them (E[h] +/- R[r], one fp32 add), rounded to bf16 together with the
table for the bf16 form; everything after that is float64.  The ensemble fold follows tests/ensemble_ref.py: D = w_0 d_0 +
sum_s w_s (d_s where head and candidate are both linked into member s, d_0 otherwise)."""
import numpy as np
import torch

from linkpred_ref import listed_mask


def dist64(ent_layers, rel_layers, h, r, pred_head=False, bf16=False):
    """float64 [B, N]: sum over layers of the L1 distance between the fp32-formed query row and every table row."""
    h = torch.as_tensor(np.asarray(h, dtype=np.int64))
    r = torch.as_tensor(np.asarray(r, dtype=np.int64))
    total = None
    for ent, rel in zip(ent_layers, rel_layers):
        e, rl = torch.as_tensor(np.asarray(ent)).float(), torch.as_tensor(np.asarray(rel)).float()
        q = e[h] - rl[r] if pred_head else e[h] + rl[r]                      # fp32, as the prep kernel
        if bf16:
            q, e = q.to(torch.bfloat16), e.to(torch.bfloat16)
        d = torch.cdist(q.double(), e.double(), p=1)
        total = d if total is None else total + d
    return total.numpy()


def ens_dist64(members, h, r, pred_head=False):
    """The ensemble distance D, float64 [B, N]; ``members`` = [(ent layers, rel layers, link or None, weight), ...] as numpy."""
    h = np.asarray(h, dtype=np.int64)
    ent0, rel0, _, w0 = members[0]
    d0 = dist64(ent0, rel0, h, r, pred_head)
    total = float(w0) * d0
    for ent, rel, link, w in members[1:]:
        link = np.asarray(link, dtype=np.int64)
        ok = (link >= 0) & (link < np.asarray(ent[0]).shape[0])
        ds = dist64(ent, rel, np.where(ok[h], link[h], 0), r, pred_head)[:, np.where(ok, link, 0)]
        total = total + float(w) * np.where(ok[h][:, None] & ok[None, :], ds, d0)
    return total


def candidates(h, r, true_tail, n, gold=None):
    """bool [B, N]: the candidate set C_b.  Prediction mode (gold None): what the index does not list; evaluation mode: plus the gold."""
    c = ~listed_mask(h, r, true_tail or {}, n)
    if gold is not None:
        c[np.arange(len(h)), np.asarray(gold, dtype=np.int64)] = True
    return c


def stats64(dist, scale, cand, gold=None):
    """dict of float64 / int64 [B] arrays: nearest (-1: empty set), dist_min (+inf), sum (0), log_sum (-inf), entropy (0), lse =
    log sum_n exp(z) (-inf), second = the runner-up distance (+inf), and with gold logp_gold."""
    dist = np.asarray(dist, dtype=np.float64)
    B = dist.shape[0]
    d = np.where(cand, dist, np.inf)
    near = d.argmin(1)                                                        # the first minimum: the lowest index on ties
    dmin = d[np.arange(B), near]
    some = np.isfinite(dmin)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = np.where(cand, -scale * (dist - np.where(some, dmin, 0.0)[:, None]), -np.inf)
        e = np.exp(u)
        l = e.sum(1)
        t = np.where(e > 0, e * np.where(cand, u, 0.0), 0.0).sum(1)
        ent = np.where(some, np.log(np.where(some, l, 1.0)) - t / np.where(some, l, 1.0), 0.0)
        log_sum = np.where(some, np.log(np.where(some, l, 1.0)), -np.inf)
    d2 = d.copy()
    d2[np.arange(B), near] = np.inf
    out = dict(nearest=np.where(some, near, -1).astype(np.int64), dist_min=dmin, sum=np.where(some, l, 0.0), log_sum=log_sum,
               entropy=ent, lse=np.where(some, -scale * np.where(some, dmin, 0.0) + log_sum, -np.inf), second=d2.min(1))
    if gold is not None:
        g = np.asarray(gold, dtype=np.int64)
        out["logp_gold"] = -scale * (dist[np.arange(B), g] - dmin) - log_sum
    return out


def delta(dist, n_layers, d, members=1):
    """The worst-case error of a distance: a length-(layers * d * members) fp32 running sum of non-negative terms."""
    return (n_layers * d * members + 2) * 2.0 ** -24 * float(np.max(dist))


def pick_scale(dist, cand, accept, lo=1e-4, hi=1e4, steps=160):
    """The first scale of a geometric grid on [lo, hi] for which accept(stats64(dist, scale, cand)) holds; None if none does."""
    for s in np.geomspace(lo, hi, steps):
        if accept(stats64(dist, float(s), cand)):
            return float(s)
    return None


def spread_scale(dist, cand):
    """A scale whose median reference entropy lies in [1, log N - 1] (the sums matter)."""
    n = dist.shape[1]
    return pick_scale(dist, cand, lambda s: 1.0 <= np.median(s["entropy"]) <= np.log(n) - 1.0)


def peaked_scale(dist, cand):
    """A scale whose median reference top-1 probability exceeds 0.99."""
    return pick_scale(dist, cand, lambda s: np.median(1.0 / np.maximum(s["sum"], 1.0)) > 0.99)


def ece(conf, correct, bins=10):
    """Expected calibration error over equal-width confidence bins, in plain Python."""
    conf, correct = np.asarray(conf, dtype=np.float64), np.asarray(correct, dtype=np.float64)
    total = 0.0
    for j in range(bins):
        lo, hi = j / bins, (j + 1) / bins
        m = (conf >= lo) & ((conf < hi) | (j == bins - 1))
        if m.any():
            total += m.sum() * abs(correct[m].mean() - conf[m].mean())
    return total / max(len(conf), 1)
