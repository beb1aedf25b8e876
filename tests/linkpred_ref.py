"""Float64 restatement of link prediction for the tests (not a test itself): the distance of src/jmac_model.py:302-313,
the dictionary filter of src/validate.py:52-57, and a stable ascending top-k (equal distances: lower index first)."""
import numpy as np
import torch


def dist64(ent_layers, rel_layers, h, r, pred_head=False, bf16=False):
    """sum over layers of cdist(E_l[h] +/- R_l[r], E_l, p=1) in float64 -> numpy [B, N].  ``bf16``: the bf16-table form's inputs
    -- the fp32 query rows and the candidate table each rounded to bf16 first (BASELINE config 3) -- then float64 as well."""
    h = torch.as_tensor(np.asarray(h, dtype=np.int64))
    r = torch.as_tensor(np.asarray(r, dtype=np.int64))
    total = None
    for ent, rel in zip(ent_layers, rel_layers):
        e, rl = torch.as_tensor(np.asarray(ent)), torch.as_tensor(np.asarray(rel))
        if bf16:
            q = (e.float()[h] - rl.float()[r] if pred_head else e.float()[h] + rl.float()[r]).to(torch.bfloat16).double()
            e = e.float().to(torch.bfloat16).double()
        else:
            e, rl = e.double(), rl.double()
            q = e[h] - rl[r] if pred_head else e[h] + rl[r]
        d = torch.cdist(q, e, p=1)
        total = d if total is None else total + d
    return total.numpy()


def listed_mask(h, r, true_tail, n):
    """bool [B, N]: entry (b, t) is set iff t is a known tail of (h_b, r_b)."""
    m = np.zeros((len(h), n), dtype=bool)
    for b, (hb, rb) in enumerate(zip(h, r)):
        tails = np.asarray(true_tail.get((int(hb), int(rb)), []), dtype=np.int64)
        m[b, tails[(tails >= 0) & (tails < n)]] = True
    return m


def topk(dist, k, listed=None):
    """(idx int64 [B, k], val float64 [B, k]): the k smallest unlisted distances of every row, ascending, equal distances
    by ascending index (a stable sort); rows with fewer than k unlisted entries end with (-1, +inf)."""
    d = np.array(dist, dtype=np.float64)
    if listed is not None:
        d[listed] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    val = np.take_along_axis(d, order, 1)
    idx = np.where(np.isinf(val), -1, order).astype(np.int64)
    return idx, val
