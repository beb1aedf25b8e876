"""Float64 restatement of cross-KG ensemble link prediction for the tests (not a test itself).

Members g = 0 .. S: (entity layers, relation layers, link or None, weight); member 0 is the target.  d_g is linkpred_ref.dist64
in member g's tables -- for a supporting member at the rows link[h] and link[n], a column gather of its [B, n_rows] distances --
and D = w_0 d_0 + sum_s w_s where(link_s[h] >= 0 and link_s[n] >= 0, d_s, d_0).  The filter and the stable top-k are
linkpred_ref.listed_mask / linkpred_ref.topk on D."""
import numpy as np

import linkpred_ref
from linkpred_ref import listed_mask, topk  # noqa: F401  (the ensemble's filter and top-k are the single-KG ones, on D)


def member_dists(members, h, r, pred_head=False):
    """[d_0, d_1 or d_0 where absent, ...] as float64 [B, N] arrays, and the presence masks (None for member 0)."""
    h = np.asarray(h, dtype=np.int64)
    ent0, rel0, _, _ = members[0]
    d0 = linkpred_ref.dist64(ent0, rel0, h, r, pred_head)
    out, present = [d0], [None]
    for ent, rel, link, _ in members[1:]:
        link = np.asarray(link, dtype=np.int64)
        n_rows = np.asarray(ent[0]).shape[0]
        ok = (link >= 0) & (link < n_rows)
        hq = np.where(ok[h], link[h], 0)
        ds = linkpred_ref.dist64(ent, rel, hq, r, pred_head)[:, np.where(ok, link, 0)]        # the column gather through the link
        p = ok[h][:, None] & ok[None, :]
        out.append(np.where(p, ds, d0))
        present.append(p)
    return out, present


def D64(members, h, r, pred_head=False):
    """The ensemble distance, float64 [B, N]."""
    ds, _ = member_dists(members, h, r, pred_head)
    total = float(members[0][3]) * ds[0]
    for (_, _, _, w), d in zip(members[1:], ds[1:]):
        total = total + float(w) * d
    return total


def ranks(D, gold, listed=None):
    """1 + #{unlisted n != gold before the gold}: smaller, or equal with the lower index."""
    D = np.asarray(D, dtype=np.float64)
    gold = np.asarray(gold, dtype=np.int64)
    rows = np.arange(len(gold))
    g = D[rows, gold][:, None]
    before = (D < g) | ((D == g) & (np.arange(D.shape[1])[None, :] < gold[:, None]))
    if listed is not None:
        before &= ~listed
    before[rows, gold] = False
    return 1 + before.sum(1)
