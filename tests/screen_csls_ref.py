"""A numpy restatement of the screened alignment top-k (jmac_sim_csls_topk_screened_f32 and its _viable_ form, jmac_amd/csrc/screen.hip;
DESIGN section 5), built on screen_ref.screen.

The kernels decide on c = csls_value(s, r1, r2) = fl(fl(2 s - r1) - r2) in float32.  2 s is exact and rounding is monotone, so for
finite r1, r2 the value is a non-decreasing function of s, its own roundings included; the screen's bounds lo = fl(sh - e) <= s <=
fl(sh + e) = hi therefore give c_lo = csls_value(lo) <= c <= csls_value(hi) = c_hi, and sample -> filter -> prune run on c_lo and
c_hi as screen_ref.screen runs them on sh - e and sh + e.  r1 = r2 = None: c = s.

The viable predicate of row i (suitor id[i]) at column j is "c beats what the reviewer holds": held[j] is the held value, held_id[j]
the suitor holding it (free[j]: nothing is held, every suitor is viable) and a suitor is viable iff c > held, or c == held and its
id is lower.  It is monotone in c: viable at c_lo = certainly viable (only those may raise a threshold), not viable at c_hi =
certainly not (only those are dropped unseen)."""
import numpy as np

import screen_ref as R


def csls_value(s, r1, r2):
    """float32, in the kernels' order; s [L, N] float32, r1 [L], r2 [N] (both None: s itself)"""
    s = np.asarray(s, dtype=np.float32)
    if r1 is None:
        return s
    r1, r2 = np.asarray(r1, dtype=np.float32), np.asarray(r2, dtype=np.float32)
    return ((np.float32(2.0) * s - r1[:, None]).astype(np.float32) - r2[None, :]).astype(np.float32)


def terms32(a, b, csls_k):
    """csls_sim's terms of the float32 product: the mean of the csls_k largest entries of every row / column"""
    s = a @ b.T
    r1 = -np.partition(-s, csls_k - 1, axis=1)[:, :csls_k]
    r2 = -np.partition(-s.T, csls_k - 1, axis=1)[:, :csls_k]
    return r1.mean(1).astype(np.float32), r2.mean(1).astype(np.float32)


class Held:
    """What the reviewers hold: value [N] float32, holder id [N], free [N] bool."""

    def __init__(self, value, holder, free):
        self.value = np.asarray(value, dtype=np.float32)
        self.holder = np.asarray(holder, dtype=np.int64)
        self.free = np.asarray(free, dtype=bool)

    def viable(self, c, row_id):
        """[L, N] bool: the suitor row_id[i] at value c[i, j] beats what column j holds"""
        rid = np.asarray(row_id, dtype=np.int64)[:, None]
        return self.free[None, :] | (c > self.value[None, :]) | ((c == self.value[None, :]) & (rid < self.holder[None, :]))


def third_best_held(c, row_id, share, seed):
    """`share` of the columns hold their third-best c over the rows (and that row's id); the others are free"""
    rng = np.random.default_rng(seed)
    n = c.shape[1]
    # order of the rows per column: value descending, equal values -> lower id first
    order = np.lexsort((np.broadcast_to(np.asarray(row_id)[:, None], c.shape), -c.astype(np.float64)), axis=0)
    third = order[2]
    free = np.ones(n, dtype=bool)
    free[rng.permutation(n)[:int(share * n)]] = False
    cols = np.arange(n)
    return Held(c[third, cols], np.asarray(row_id)[third], free)


def screen(a, b, k, r1=None, r2=None, held=None, row_id=None):
    """sample -> filter -> prune on c_lo / c_hi.  Returns screen_ref.screen's fields plus c_lo, c_hi."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    sc = R.screen(a, b, k)
    lo = (sc["sh"] - sc["e"]).astype(np.float32)
    hi = (sc["sh"] + sc["e"]).astype(np.float32)
    c_lo, c_hi = csls_value(lo, r1, r2), csls_value(hi, r1, r2)
    if held is None:
        certain = possible = np.ones(c_lo.shape, dtype=bool)
    else:
        rid = np.arange(len(a)) if row_id is None else row_id
        certain, possible = held.viable(c_lo, rid), held.viable(c_hi, rid)
    ns = R.sample(b.shape[0])
    lower = R.kth_largest(np.where(certain, c_lo, -np.inf)[:, :ns].astype(np.float64), k)
    listed = possible & ~(c_hi < lower[:, None])
    lower2 = R.kth_largest(np.where(listed & certain, c_lo, -np.inf).astype(np.float64), k)
    kept = listed & ~(c_hi < lower2[:, None])
    return dict(sh=sc["sh"], e=sc["e"], c_lo=c_lo, c_hi=c_hi, listed=listed, kept=kept, list_len=listed.sum(1),
                overflow=listed.sum(1) > R.CAP)


def topk_of(c, k, viable=None):
    """the k best columns of c per row (ties -> lower index), -1 where a row has fewer than k viable ones [L, k]"""
    v = c.astype(np.float64) if viable is None else np.where(viable, c.astype(np.float64), -np.inf)
    idx = np.argsort(-v, axis=1, kind="stable")[:, :k]
    if viable is not None:
        idx = np.where(np.take_along_axis(viable, idx, axis=1), idx, -1)
    return idx


def must_overflow(c, k, viable=None):
    """rows with more than CAP (viable) columns at or above their k-th best value: no exact method can list fewer"""
    v = c.astype(np.float64) if viable is None else np.where(viable, c.astype(np.float64), -np.inf)
    kth = R.kth_largest(v, k)
    return ((v >= kth[:, None]) & np.isfinite(v)).sum(1) > R.CAP


def key(v):
    """the kernels' order-preserving 32-bit key of a float32 (-0 and +0 share one)"""
    v = np.asarray(v, dtype=np.float32)
    u = np.where(v == 0, np.float32(0), v).astype(np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000)).astype(np.uint64)


def word(v, i):
    """the 64-bit word of (value, id): key << 32 | ~id; descending word order = larger value first, then lower id"""
    return (key(v) << np.uint64(32)) | (~np.asarray(i, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))


def best_words(held):
    """the reviewers' words [N] uint64 of a Held (0 = free)"""
    return np.where(held.free, np.uint64(0), word(held.value, held.holder)).astype(np.uint64)
