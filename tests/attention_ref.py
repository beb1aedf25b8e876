"""numpy float64 restatement of the attention export's definition (include/jmac_hip.h, jmac_rel_attn_edge_weights_*):

    h_e = P[i] + Q[j] - Rq[t]      s_e = sum_k a_k LeakyReLU(h_e[k])      alpha = softmax of s over the in-edges of i

from GIVEN tables, for the tests.  No torch, no device."""
from collections import namedtuple

import numpy as np

AttentionRef = namedtuple("AttentionRef", "alpha alpha_scaled logit entropy argmax A deg")


def attention_ref(P, Q, Rq, a, dst, src, typ, slope, n):
    """P [n, d], Q [nsrc, d], Rq [nrel, d], a [d]; dst / src / typ [E] in the caller's edge order.  Returns, all float64 and in
    that order: alpha, alpha * sqrt(deg), the logits, the entropy per destination (0 where empty), the argmax edge per destination
    (largest alpha, lowest edge id among exact ties, -1 where empty), A_e = sum_k |a_k| |LeakyReLU(h_e[k])| (the magnitude an
    fp32 evaluation of s_e rounds against) and the in-degrees."""
    P, Q, Rq, a = (np.asarray(x, dtype=np.float64) for x in (P, Q, Rq, a))
    dst, src, typ = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (dst, src, typ))
    E = dst.shape[0]
    deg = np.bincount(dst, minlength=n).astype(np.int64)
    if E == 0:
        z = np.zeros(0)
        return AttentionRef(z, z, z, np.zeros(n), np.full(n, -1, dtype=np.int64), z, deg)
    h = P[dst] + Q[src] - Rq[typ]
    act = np.where(h > 0, h, slope * h)
    s = act @ a
    A = np.abs(act) @ np.abs(a)
    m = np.full(n, -np.inf)
    np.maximum.at(m, dst, s)
    t = s - m[dst]
    e = np.exp(t)
    den = np.zeros(n)
    np.add.at(den, dst, e)
    alpha = e / den[dst]
    H = np.zeros(n)
    np.add.at(H, dst, -alpha * (t - np.log(den[dst])))              # log alpha without the 0 * log 0 of an underflown weight
    order = np.lexsort((np.arange(E), -alpha, dst))                  # by destination, then weight descending, then edge id
    first = np.ones(E, dtype=bool)
    first[1:] = dst[order][1:] != dst[order][:-1]
    argmax = np.full(n, -1, dtype=np.int64)
    argmax[dst[order][first]] = order[first]
    return AttentionRef(alpha, alpha * np.sqrt(deg[dst]), s, H, argmax, A, deg)


def reference_tables(params, X, R, slope, rel_act="leaky_relu"):
    """The factorised tables (P, Q, Rq, a) of the layer in float64 from the reference layer's parameters (``params``: name ->
    array, state_dict names) and inputs: src/jmac_model.py:39-42 for the relation transform, [Wt; Wb] = w_att (:75-76)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    X, R = np.asarray(X, dtype=np.float64), np.asarray(R, dtype=np.float64)
    d_in = X.shape[1]
    rel = np.concatenate([R, p["loop_rel"]], axis=0) @ p["rel_transform_weight1"]
    rel = np.where(rel > 0, rel, (slope if rel_act == "leaky_relu" else 0.0) * rel) @ p["rel_transform_weight2"]
    wt, wb = p["w_att"][:d_in], p["w_att"][d_in:]
    return X @ wt, X @ wb, rel @ wb, p["a_att"].reshape(-1)
