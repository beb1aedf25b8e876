"""Float64 restatement, in plain torch, of what scoring.sim_softmax_stats / scoring.alignment_stats compute: the expected values
of the matrix-free EnTr tests (host and GPU).  The closed form for the masked matrix is written out here a second time, on
purpose independent of jmac_amd/scoring.py."""
import numpy as np
import torch


def first_argmax(m, dim: int) -> np.ndarray:
    """Index of the FIRST maximum along ``dim`` (stable rule, numpy)."""
    a = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    return (a == a.max(axis=dim, keepdims=True)).argmax(axis=dim)


def softmax_stats(S: torch.Tensor, scale: float = 20.0):
    """(max, first arg-max, sum e^(scale (s - max)), entropy of softmax(scale s)) along the rows of the float64 matrix S."""
    S = S.double()
    mx = S.max(1, keepdim=True)[0]
    x = scale * (S - mx)
    e = torch.exp(x)
    l = e.sum(1)
    t = (e * x).sum(1)
    return mx[:, 0], torch.from_numpy(first_argmax(S, 1)), l, torch.log(l) - t / l


def sliced_softmax_stats(a: torch.Tensor, b: torch.Tensor, scale: float = 20.0, rows: int = 500):
    """Row AND column statistics of a b^T in float64, the product evaluated ``rows`` rows at a time; also the gap between the two
    largest entries of every row.  Returns (row (max, arg, l, ent), col (max, arg, l, ent), row_gap)."""
    a, b = a.double(), b.double()
    n2 = b.shape[0]
    r_out, gaps = [], []
    cm = torch.full((n2,), -np.inf, dtype=torch.float64)
    ca = torch.zeros(n2, dtype=torch.long)
    for r0 in range(0, a.shape[0], rows):
        S = a[r0:r0 + rows] @ b.t()
        r_out.append(softmax_stats(S, scale))
        top = torch.topk(S, 2, dim=1).values
        gaps.append(top[:, 0] - top[:, 1])
        m, i = S.max(0)[0], torch.from_numpy(first_argmax(S, 0)) + r0
        ca = torch.where(m > cm, i, ca)
        cm = torch.maximum(cm, m)
    cl, ct = torch.zeros(n2, dtype=torch.float64), torch.zeros(n2, dtype=torch.float64)
    for r0 in range(0, a.shape[0], rows):
        x = scale * (a[r0:r0 + rows] @ b.t() - cm)
        e = torch.exp(x)
        cl += e.sum(0)
        ct += (e * x).sum(0)
    row = tuple(torch.cat([o[k] for o in r_out]) for k in range(4))
    return row, (cm, ca, cl, torch.log(cl) - ct / cl), torch.cat(gaps)


def _masked_best(x, l, arg, ids, c, first_masked, fill, scale):
    """Largest softmax entry and its first index of a line whose kept entries (ids ``ids``, ascending) have maximum x, sum l and
    arg-max position arg, and whose c other entries all equal ``fill``."""
    idx = torch.as_tensor(ids)[arg]
    if c == 0:
        return 1.0 / l, idx
    M = torch.clamp(x, min=fill)
    denom = l * torch.exp(scale * (x - M)) + c * torch.exp(scale * (fill - M))
    fm = torch.full_like(idx, first_masked)
    idx = torch.where(x < fill, fm, torch.where(x == fill, torch.minimum(idx, fm), idx))
    return 1.0 / denom, idx


def alignment_stats(emb1, emb2, list1, list2, scale: float = 20.0, fill: float = -1.0):
    """(entropy, row_best_prob [N1], row_best [N1], col_best_prob [N2], col_best [N2]) of compute_alignment_quality
    (train.py:231-259) in float64 from the |list1| x |list2| sub-product alone."""
    e1, e2 = torch.as_tensor(emb1).double(), torch.as_tensor(emb2).double()
    N1, N2 = e1.shape[0], e2.shape[0]
    l1, l2 = np.asarray(list1, dtype=np.int64), np.asarray(list2, dtype=np.int64)
    S = e1[l1] @ e2[l2].t()                                           # as listed: repeats count in the entropy
    entropy = softmax_stats(S, scale)[3].mean() + softmax_stats(S.t(), scale)[3].mean()
    u1, u2 = np.unique(l1), np.unique(l2)
    S = e1[u1] @ e2[u2].t()

    def first_missing(u, n):
        rest = np.setdiff1d(np.arange(n), u)
        return int(rest[0]) if len(rest) else n
    row_p, row_i = torch.full((N1,), 1.0 / N2, dtype=torch.float64), torch.zeros(N1, dtype=torch.long)
    col_p, col_i = torch.full((N2,), 1.0 / N1, dtype=torch.float64), torch.zeros(N2, dtype=torch.long)
    x, arg, l, _ = softmax_stats(S, scale)
    row_p[u1], row_i[u1] = _masked_best(x, l, arg, u2, N2 - len(u2), first_missing(u2, N2), fill, scale)
    x, arg, l, _ = softmax_stats(S.t(), scale)
    col_p[u2], col_i[u2] = _masked_best(x, l, arg, u1, N1 - len(u1), first_missing(u1, N1), fill, scale)
    return entropy, row_p, row_i, col_p, col_i


def seeded_case(seed: int = 11, N1: int = 90, N2: int = 75, d: int = 48):
    """fp32 tables and lists with repeated entries, an antipodal row (every listed similarity == -1 exactly, the fill value), a
    row and a column below the fill value.  Products involved in those lines are exact in fp32 and float64 alike."""
    g = torch.Generator().manual_seed(seed)
    emb1 = torch.nn.functional.normalize(torch.randn(N1, d, generator=g), dim=1)
    emb2 = torch.nn.functional.normalize(torch.randn(N2, d, generator=g), dim=1)
    list1 = [3, 5, 8, 9, 12, 5, 20, 33, 41, 41, 57, 60, 71, 88, 1]          # 0, 2 not listed; 5 and 41 twice
    list2 = [0, 1, 4, 7, 7, 10, 19, 22, 30, 44, 51, 63, 74, 0]             # 2 not listed; 7 and 0 twice
    emb1[list1, 1] = 0.5
    emb2[list2, 0] = 0.5
    emb2[list2, 1] = 0.0
    ia, ib, jc = 9, 33, 22
    emb1[ia] = 0.0
    emb1[ia, 0], emb1[ia, 1] = -2.0, 0.5            # . listed column = -1 exactly (jc: -2): x == fill
    emb1[ib] = 0.0
    emb1[ib, 0], emb1[ib, 1] = -4.0, 0.5            # . listed column = -2: x < fill
    emb2[jc] = 0.0
    emb2[jc, 1] = -4.0                              # listed row . jc = -2: column maximum below fill
    return emb1, emb2, list1, list2, (ia, ib, jc)
