"""numpy float64 restatement of the alignment evaluator's Manhattan similarity (modules/finding/similarity.py:47-49, :58-84 and the
rank rule of alignment.py:87-112), shared by the host and GPU tests of the manhattan metric:

    s(i, j) = 1 - sum_k |a[i, k] - b[j, k]|            (rows L2-normalised first under ``normalize``)
    c(i, j) = 2 s(i, j) - r1[i] - r2[j],  r1[i] / r2[j] = the EXACT mean of the csls_k largest s of row i / column j
    rank[i] = 1 + #{j : c(i, j) > c(i, gold[i]) or (== and j < gold[i])}

(the reference's np.partition(-s, k + 1)[:, :k] takes *some* k of the k + 1 largest: scoring.csls_sim's docstring)."""
import numpy as np


def manhattan_sim(a, b, normalize=False, block=256):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if normalize:
        a = a / np.linalg.norm(a, axis=1, keepdims=True)
        b = b / np.linalg.norm(b, axis=1, keepdims=True)
    s = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    for lo in range(0, b.shape[0], block):                      # [n1, block, d] at a time
        s[:, lo:lo + block] = 1.0 - np.abs(a[:, None, :] - b[None, lo:lo + block, :]).sum(-1)
    return s


def csls(s, csls_k):
    """c of the definition above (csls_k = 0: s itself)."""
    if csls_k <= 0:
        return s
    r1 = -np.sort(-s, axis=1)[:, :csls_k].mean(1)
    r2 = -np.sort(-s.T, axis=1)[:, :csls_k].mean(1)
    return 2.0 * s - r1[:, None] - r2[None, :]


def ranks(c, gold):
    gold = np.asarray(gold, dtype=np.int64)
    g = c[np.arange(c.shape[0]), gold][:, None]
    col = np.arange(c.shape[1])[None, :]
    return ((c > g) | ((c == g) & (col < gold[:, None]))).sum(1) + 1


def summary(rank, top_k=(1, 5, 10)):
    """(hits [%], mr, mrr) as greedy_alignment reports them (alignment.py:87-112)."""
    rank = np.asarray(rank, dtype=np.float64)
    return [float((rank <= k).mean() * 100.0) for k in top_k], float(rank.mean()), float((1.0 / rank).mean())
