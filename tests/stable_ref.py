"""CPU reference of the stable one-to-one alignment: textbook sequential Gale-Shapley (suitors propose, one at a time), on a
dense score matrix or on incomplete candidate lists, under the project's strict order --

    suitor i prefers j to j'    iff c(i, j) > c(i, j'), or the values are equal and j < j'
    reviewer j prefers i to i'  iff c(i, j) > c(i', j), or the values are equal and i < i'

-- and a count of blocking pairs.  Plain numpy and Python: nothing here shares code with the library."""
import numpy as np


def pack_word(v, i):
    """The 64-bit word of (value, index) whose unsigned order is "larger value first, equal values -> lower index first"
    (an order-preserving key of the fp32 value in the high half, the complemented index in the low half), as np.uint64."""
    v = np.asarray(v, dtype=np.float32)
    u = np.where(v == 0, np.float32(0), v).view(np.uint32).astype(np.uint64)                 # -0 and +0: one key
    key = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000))
    return (key << np.uint64(32)) | (~np.asarray(i).astype(np.uint64) & np.uint64(0xffffffff))


def _deferred_acceptance(n1, n2, candidate, order=None):
    """candidate(i, p) -> (j, c(i, j)) of suitor i's p-th choice, or None past the end of its list.  ``order``: the suitors in the
    order in which they are first taken up (the result must not depend on it)."""
    match1 = np.full(n1, -1, dtype=np.int64)
    match2 = np.full(n2, -1, dtype=np.int64)
    held = np.zeros(n2, dtype=np.float64)                        # c(match2[j], j)
    pos = np.zeros(n1, dtype=np.int64)
    free = list(reversed(list(range(n1) if order is None else order)))
    while free:
        i = free.pop()
        while True:
            cand = candidate(i, int(pos[i]))
            if cand is None:
                break                                            # unmatched for good
            j, v = cand
            h = match2[j]
            if h < 0 or v > held[j] or (v == held[j] and i < h):
                if h >= 0:
                    match1[h] = -1
                    pos[h] += 1
                    free.append(int(h))
                match1[i], match2[j], held[j] = j, i, v
                break
            pos[i] += 1
    return match1, match2


def stable_dense(c, order=None):
    """(match1 [n1], match2 [n2]) of the full instance c [n1, n2]; -1 = unmatched / free."""
    c = np.asarray(c)
    n1, n2 = c.shape
    prefs = {}

    def candidate(i, p):
        if p >= n2:
            return None
        if i not in prefs:
            prefs[i] = np.argsort(-c[i], kind="stable")          # descending, equal values in ascending index order
        j = int(prefs[i][p])
        return j, float(c[i, j])

    return _deferred_acceptance(n1, n2, candidate, order)


def stable_lists(idx, val, n2, order=None):
    """The same on incomplete lists: idx [n1, k] reviewer ids best first (-1 ends a list), val [n1, k] their scores."""
    idx, val = np.asarray(idx), np.asarray(val)
    n1, k = idx.shape

    def candidate(i, p):
        if p >= k or idx[i, p] < 0:
            return None
        return int(idx[i, p]), float(val[i, p])

    return _deferred_acceptance(n1, n2, candidate, order)


def blocking_pairs(c, match1):
    """Number of pairs (i, j), j != match1[i], where i prefers j to its partner (or has none) and j prefers i to its partner (or
    has none)."""
    c = np.asarray(c)
    match1 = np.asarray(match1)
    n1, n2 = c.shape
    match2 = np.full(n2, -1, dtype=np.int64)
    match2[match1[match1 >= 0]] = np.nonzero(match1 >= 0)[0]
    ii, jj = np.arange(n1)[:, None], np.arange(n2)[None, :]
    m1 = np.where(match1 >= 0, match1, 0)
    mine = np.where(match1 >= 0, c[np.arange(n1), m1], -np.inf)[:, None]
    suitor_wants = (match1 < 0)[:, None] | (c > mine) | ((c == mine) & (jj < match1[:, None]))
    m2 = np.where(match2 >= 0, match2, 0)
    theirs = np.where(match2 >= 0, c[m2, np.arange(n2)], -np.inf)[None, :]
    reviewer_wants = (match2 < 0)[None, :] | (c > theirs) | ((c == theirs) & (ii < match2[None, :]))
    return int((suitor_wants & reviewer_wants & (jj != match1[:, None])).sum())
