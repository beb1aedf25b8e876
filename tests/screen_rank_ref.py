"""A numpy restatement of the screened alignment ranks (jmac_sim_csls_rank_screened_f32, jmac_amd/csrc/screen.hip),
built on screen_ref / screen_csls_ref, and the gold choices its CPU and GPU tests share.

rank_i = 1 + #{j : before(c(i, j), j)} with before(c, j) := c > g || (c == g && j < G), g = c(i, gold_i) and G = gold_i.  The predicate
is monotone in c and the screen bounds every element, c_lo <= c <= c_hi (screen_csls_ref), so a column is
    certainly before    before(c_lo, j): counted without rescoring;
    certainly not       c_hi < g || (c_hi == g && j > G): dropped;
    undecided           otherwise -- g lies in [c_lo, c_hi]: LISTED and put to the exact predicate (the gold column always is, and
                        its rescored value is g: it never counts).
A row whose list is longer than CAP overflows: its rank comes from a dense pass."""
import numpy as np

import screen_csls_ref as C
import screen_ref as R

CAP = 512                   # RK_CAP of screen.hip
BAND = 32                   # a row whose restated list length is within BAND of CAP is asserted on neither side
CHOICES = ("best", "r100", "median", "spread")


def exact_c(a, b, r1=None, r2=None):
    """c of the float32 product"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return C.csls_value((a @ b.T).astype(np.float32), r1, r2)


def before(c, g, gold):
    """[L, N] bool: column j comes before the gold column at value c[i, j]"""
    j = np.arange(c.shape[1])[None, :]
    return (c > g[:, None]) | ((c == g[:, None]) & (j < np.asarray(gold)[:, None]))


def golds(c, choice):
    """one gold column per row, from the order of c in the row (descending, ties -> lower index)"""
    L, N = c.shape
    if choice == "spread":
        return ((37 * np.arange(L) + 5) % N).astype(np.int32)
    at = {"best": 0, "r100": 99, "median": N // 2}[choice]
    return np.argsort(-c.astype(np.float64), axis=1, kind="stable")[:, at].astype(np.int32)


def screen_rank(a, b, gold, r1=None, r2=None, c=None):
    """c: the exact matrix the gold values and the listed columns' decisions are taken from (default: the float32 product's).
    Returns certain (the certainly-before mask) and its per-row count, never (certainly not), listed, list_len, overflow and the rank."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    gold = np.asarray(gold)
    c = exact_c(a, b, r1, r2) if c is None else c
    sh = R.bf16_rne(a).astype(np.float64) @ R.bf16_rne(b).astype(np.float64).T
    e = R.bound(a, b).astype(np.float64)
    lo, hi = (sh - e).astype(np.float32), (sh + e).astype(np.float32)
    c_lo, c_hi = C.csls_value(lo, r1, r2), C.csls_value(hi, r1, r2)
    g = c[np.arange(len(a)), gold]
    j = np.arange(b.shape[0])[None, :]
    certain = before(c_lo, g, gold)
    never = (c_hi < g[:, None]) | ((c_hi == g[:, None]) & (j > gold[:, None]))
    listed = ~certain & ~never
    rank = 1 + certain.sum(1) + (listed & before(c, g, gold)).sum(1)
    return dict(c=c, g=g, certain=certain, before_count=certain.sum(1), never=never, listed=listed, list_len=listed.sum(1), overflow=listed.sum(1) > CAP,
                rank=rank.astype(np.int32))


def must_overflow(c, gold):
    """rows with more than CAP columns exactly tied with their gold value: undecided under any bound of non-zero width"""
    g = c[np.arange(len(c)), np.asarray(gold)]
    return (c == g[:, None]).sum(1) > CAP


def in_band(ref):
    return np.abs(ref["list_len"] - CAP) <= BAND
