"""CPU reference of the auction assignment (Bertsekas' auction algorithm on candidate lists), in numpy fp32, and the checks the
tests share.  Plain numpy and Python: nothing here shares code with the library.

State of an instance with n1 <= n2 (rows bid for columns):
    price [n2] fp32 (start 0), owner [n2] int32 (start -1), match1 [n1] int32: >= 0 the column held, -1 open, -2 open and
    waiting for a refill
Lists: idx / val / pref [n1, k]: column ids, c - price as of the refill (best first, equal values -> lower column), the price then.

One synchronous round (``run_rounds``): every row at -1 at its start takes cur = val - (price[idx] - pref) in fp32, w1 = the
largest (equal values -> lower column), w2 = the largest of the others, bound = val[k - 1] (k == n2: -inf).  w2 < bound: the row
becomes -2.  Otherwise it bids (price[j1] + (w1 - w2)) + eps (nextafter(price[j1], +inf) if that is no raise); per column the
highest bid wins, equal bids -> the lower row; the previous owner gets -1."""
import numpy as np

F = np.float32


def pack_word(v, i):
    """The 64-bit word of (value, index) whose unsigned order is "larger value first, equal values -> lower index first"."""
    v = np.asarray(v, dtype=np.float32)
    u = np.where(v == 0, np.float32(0), v).view(np.uint32).astype(np.uint64)
    key = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000))
    return (key << np.uint64(32)) | (~np.asarray(i).astype(np.uint64) & np.uint64(0xffffffff))


class State:
    def __init__(self, n1, n2):
        self.price = np.zeros(n2, dtype=np.float32)
        self.owner = np.full(n2, -1, dtype=np.int32)
        self.match1 = np.full(n1, -1, dtype=np.int32)


def run_rounds(idx, val, pref, st, eps, rounds):
    """Up to ``rounds`` rounds on the state, in place; stops early once a round has no bidder.  Returns the counters
    [rows open (-1 or -2), rows at -2, rounds with a bidder, bids made]."""
    n1, k = idx.shape
    n2 = st.price.shape[0]
    eps = F(eps)
    price, owner, match1 = st.price, st.owner, st.match1
    done = made = 0
    for _ in range(int(rounds)):
        bids = {}                                                # column -> (word, bid, row) of the best bid so far
        n = 0
        for i in np.nonzero(match1 == -1)[0]:
            j = idx[i]
            cur = val[i] - (price[j] - pref[i])                  # two fp32 subtractions
            m1 = int(np.argmax(pack_word(cur, j)))
            w1, j1 = cur[m1], int(j[m1])
            w2 = np.delete(cur, m1).max()
            bound = val[i, k - 1] if k < n2 else F(-np.inf)
            if w2 < bound:
                match1[i] = -2
                continue
            bid = F(F(price[j1] + F(w1 - w2)) + eps)
            if not bid > price[j1]:
                bid = np.nextafter(price[j1], F(np.inf))
            word = int(pack_word(bid, i))
            if j1 not in bids or word > bids[j1][0]:
                bids[j1] = (word, bid, int(i))
            n += 1
        if n == 0:
            break
        for j1, (_, bid, i) in bids.items():
            if owner[j1] >= 0:
                match1[owner[j1]] = -1
            owner[j1], match1[i], price[j1] = i, j1, bid
        done += 1
        made += n
    return [int((match1 < 0).sum()), int((match1 == -2).sum()), done, made]


def topk_lists(m, k):
    """(idx int32 [rows, k], val fp32 [rows, k]) of the k largest entries per row of m, best first, equal values -> lower column."""
    m = np.asarray(m, dtype=np.float32)
    order = np.argsort(-m, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(m, order, 1)


def refill(c, idx, val, pref, st, k):
    """New lists under the current prices for the rows at -2 (ascending), from the stored matrix; returns how many."""
    rows = np.nonzero(st.match1 == -2)[0]
    if len(rows):
        idx[rows], val[rows] = topk_lists(c[rows] - st.price[None, :], k)
        pref[rows] = st.price[idx[rows]]
        st.match1[rows] = -1
    return len(rows)


def auction_dense(c, k, eps=1e-3, batch=64, max_rounds=None):
    """The driver loop with the full-matrix refill on c [n1, n2] fp32, n1 <= n2: (match1 int64 [n1], val1 fp32 [n1], price fp32
    [n2], stats)."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    n1, n2 = c.shape
    assert n1 <= n2 and 2 <= k <= min(64, n2)
    st = State(n1, n2)
    idx, val = topk_lists(c, k)
    pref = np.zeros_like(val)
    stats = {"rounds": 0, "bids": 0, "batches": 0, "refills": 0, "refill_rows": 0, "complete": True}
    while True:
        rounds = batch if max_rounds is None else min(batch, int(max_rounds) - stats["rounds"])
        n_open, _, done, made = run_rounds(idx, val, pref, st, eps, rounds)
        stats["rounds"] += done
        stats["bids"] += made
        stats["batches"] += 1
        if n_open == 0:
            break
        if max_rounds is not None and stats["rounds"] >= int(max_rounds):
            stats["complete"] = False
            break
        rows = refill(c, idx, val, pref, st, k)
        stats["refills"] += 1 if rows else 0
        stats["refill_rows"] += rows
    m1 = np.where(st.match1 >= 0, st.match1, -1).astype(np.int64)
    held = idx == m1[:, None]
    val1 = np.where(m1 >= 0, ((val + pref) * held).sum(1, dtype=np.float32), F(-np.inf)).astype(np.float32)
    stats["unmatched"] = int((m1 < 0).sum())
    return m1, val1, st.price.copy(), stats


# ---- data and checks the tests share -----------------------------------------------------------------------------------------------
def planted(n1, n2, d=8, noise=2.0, seed=0):
    """(a [n1, d], b [n2, d], perm) fp32 unit rows: min(n1, n2) planted pairs b[perm[i]] = a[i] + noise N(0, I) on the smaller side's
    terms (n1 <= n2: every row of a has a partner, the other rows of b are random; n1 > n2: row perm[j] of a is column j's)."""
    rng = np.random.default_rng(seed)
    if n1 > n2:
        b, a, perm = planted(n2, n1, d, noise, seed)
        return a, b, perm
    a = rng.standard_normal((n1, d))
    b = rng.standard_normal((n2, d))
    perm = rng.permutation(n2)[:n1]
    b[perm] = a + noise * rng.standard_normal((n1, d))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a.astype(np.float32), b.astype(np.float32), perm


def csls_matrix(a, b, csls_k):
    """2 S - r1 - r2 in fp32 (csls_k = 0: S), S = a b^T."""
    s = (a.astype(np.float32) @ b.astype(np.float32).T).astype(np.float32)
    if csls_k <= 0:
        return s
    r1 = (-np.sort(-s, axis=1)[:, :csls_k]).mean(1, dtype=np.float32)
    r2 = (-np.sort(-s, axis=0)[:csls_k]).mean(0, dtype=np.float32)
    return ((F(2) * s - r1[:, None]) - r2[None, :]).astype(np.float32)


def tolerance(c, price):
    """8 * 2^-24 * (max |C| + max price): a value passes through three rounded fp32 operations, each within 2^-24 of that
    magnitude; the factor 8 gives more than twice that."""
    return 8.0 * 2.0 ** -24 * (float(np.abs(c).max()) + float(np.max(price)))


def certificate(c, match1, price, eps):
    """The optimality certificate of an assignment of the rows of c [n1, n2], n1 <= n2, in float64 from the stored matrix and the
    prices: asserts 1 .. 4 and returns (largest slack of 3, duality gap of 4, tol)."""
    c64 = np.asarray(c, dtype=np.float64)
    n1, n2 = c64.shape
    m = np.asarray(match1).astype(np.int64)
    p = np.asarray(price, dtype=np.float64)
    assert n1 <= n2 and m.shape == (n1,) and p.shape == (n2,)
    tol = tolerance(c, price)
    assert m.min() >= 0 and m.max() < n2 and len(np.unique(m)) == n1                             # 1
    free = np.ones(n2, dtype=bool)
    free[m] = False
    assert (p >= 0).all() and (p[free] == 0).all()                                                # 2
    net = c64 - p[None, :]
    best = net.max(1)
    mine = net[np.arange(n1), m]
    slack = float((best - mine).max())
    assert slack <= eps + 2 * tol, (slack, eps, tol)                                              # 3
    gap = float(best.sum() + p.sum() - c64[np.arange(n1), m].sum())
    assert gap <= n1 * (eps + 2 * tol), (gap, n1, eps, tol)                                       # 4
    return slack, gap, tol
