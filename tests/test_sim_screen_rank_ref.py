"""CPU: what the screened alignment ranks (jmac_sim_csls_rank_screened_f32) rest on, restated in numpy (screen_rank_ref.py) on every
input family the GPU test runs, with csls_k = 10 terms (sub_bound_gaps and overflow have 8 and 6 rows: that many neighbours there)
and without terms, for every gold choice:
  * containment: the certainly-before columns lie in the before-set of the float32 product's c (and of the float64 product's,
    rounded), the certainly-not columns in its complement -- so no column is decided wrongly without being rescored;
  * the restatement's rank is the rank counted on that matrix;
  * a row with more than CAP columns exactly tied with its gold overflows (the one-row-repeated family, the zero rows of the
    un-normalised one without terms): the dense pass is reachable and tested;
  * the band: n_rescored is asserted on neither side for a row whose restated list length is within 32 of CAP (the bf16 product's
    fp32 accumulation moves a few entries).  For the choices best, r100 and median at most 5 % of a case's rows may lie there, or
    the GPU test's count assertions would be hollow; spread puts 1 of 8 rows of sub_bound_gaps in the band and is used for rank
    equality only.  If RK_CAP changes, re-derive this and pick gold choices that keep it."""
import functools

import numpy as np
import pytest

import screen_csls_ref as C
import screen_rank_ref as K
import screen_ref as R

FAMILIES = R.families()
CASES = [(name, terms, choice) for name in FAMILIES for terms in ("csls", "none") for choice in K.CHOICES]


@functools.lru_cache(maxsize=None)
def setup(name, terms):
    f = FAMILIES[name]
    a, b = f["a"], f["b"]
    r1, r2 = C.terms32(a, b, min(10, len(a))) if terms == "csls" else (None, None)
    s32 = (a @ b.T).astype(np.float32)
    s64 = (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
    return a, b, r1, r2, C.csls_value(s32, r1, r2), C.csls_value(s64, r1, r2)


@pytest.mark.parametrize("name,terms,choice", CASES)
def test_containment_rank_and_band(name, terms, choice):
    a, b, r1, r2, c32, c64 = setup(name, terms)
    if r1 is not None:
        assert np.isfinite(r1).all() and np.isfinite(r2).all()
    gold = K.golds(c32, choice)
    assert gold.min() >= 0 and gold.max() < b.shape[0]
    for c, what in ((c32, "float32 product"), (c64, "float64 product")):
        ref = K.screen_rank(a, b, gold, r1, r2, c)
        exact = K.before(c, ref["g"], gold)
        assert not (ref["certain"] & ~exact).any(), (name, what)
        assert not (ref["never"] & exact).any(), (name, what)
        assert not (ref["certain"] & ref["never"]).any()
        assert np.array_equal(ref["rank"], 1 + exact.sum(1)), (name, what)
        assert ref["listed"][np.arange(len(a)), gold].all()               # the gold column is always rescored
    ref = K.screen_rank(a, b, gold, r1, r2, c32)
    if choice == "best":
        assert (ref["rank"] == 1).all()
    must = K.must_overflow(c32, gold)
    assert ref["overflow"][must].all()
    band = K.in_band(ref)
    fit = ~ref["overflow"]
    print("%s %s %s: list length mean %.1f max %d over the %d rows that fit, %d rows overflow (%d must), %d of %d rows in the band"
          % (name, terms, choice, ref["list_len"][fit].mean() if fit.any() else 0, ref["list_len"][fit].max() if fit.any() else 0,
             fit.sum(), ref["overflow"].sum(), must.sum(), band.sum(), len(a)))
    if choice != "spread":
        assert band.sum() <= 0.05 * len(a), (name, terms, choice, int(band.sum()))


def test_rows_that_must_overflow():
    """every column of the one-row-repeated family ties with the gold, with terms or without; so do the zero rows of the
    un-normalised family without terms (with terms r2 separates the columns)"""
    for terms in ("csls", "none"):
        a, b, r1, r2, c32, _ = setup("overflow", terms)
        gold = K.golds(c32, "spread")
        assert K.must_overflow(c32, gold).all()
        ref = K.screen_rank(a, b, gold, r1, r2, c32)
        assert ref["overflow"].all() and np.array_equal(ref["rank"], gold + 1)
    a, b, r1, r2, c32, _ = setup("unnormalised", "none")
    gold = K.golds(c32, "median")
    must = K.must_overflow(c32, gold)
    assert list(np.flatnonzero(must)) == FAMILIES["unnormalised"]["overflow_rows"]
    assert K.screen_rank(a, b, gold, r1, r2, c32)["overflow"][must].all()


def test_gold_choices():
    c = np.array([[0.5, 0.9, 0.9, 0.1]] * 3, dtype=np.float32)
    assert list(K.golds(c, "best")) == [1, 1, 1]                         # ties -> lower index
    assert list(K.golds(c, "median")) == [0, 0, 0]
    assert list(K.golds(c, "spread")) == [1, 2, 3]
    assert np.array_equal(K.before(c, c[np.arange(3), [2, 2, 2]], [2, 2, 2]).sum(1), [1, 1, 1])
