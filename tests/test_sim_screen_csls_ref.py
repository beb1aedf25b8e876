"""CPU: what the screened alignment top-k (jmac_sim_csls_topk_screened_f32, _viable_screened_f32) rests on, restated in numpy
(screen_csls_ref.py) on every input family its GPU test runs, with csls_k = 10 terms (sub_bound_gaps and overflow have 8 and 6 rows:
that many neighbours there, the most csls_terms takes) and with a held-value vector:
  * c_lo <= c <= c_hi element by element, c = csls_value(s) in float32 with s the float32 product AND the float64 product rounded
    to float32 (the bound is about csls_value's own roundings: the value is monotone in s with them included);
  * the pruned set contains the k best columns of c (of the viable columns, under the exact predicate), for either s;
  * a row MUST overflow when more than CAP (viable) columns tie with or beat its k-th best value -- no exact method can do with
    fewer; every other row's list stays within CAP, so the GPU test cannot pass by recomputing: under CSLS the zero rows of the
    un-normalised family no longer overflow (r2 separates the columns), the one-row-repeated family still does."""
import functools

import numpy as np
import pytest

import screen_csls_ref as C
import screen_ref as R

FAMILIES = R.families()
CASES = [(name, k) for name, f in FAMILIES.items() for k in sorted(set(f["ks"] + [16]))]


def csls_k_of(name):
    """10, or the row count where a family has fewer rows than that (csls_terms takes at most min(n1, n2) neighbours)"""
    return min(10, len(FAMILIES[name]["a"]))


@functools.lru_cache(maxsize=None)
def setup(name):
    f = FAMILIES[name]
    a, b = f["a"], f["b"]
    r1, r2 = C.terms32(a, b, csls_k_of(name))
    s32 = (a @ b.T).astype(np.float32)
    s64 = (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
    c32, c64 = C.csls_value(s32, r1, r2), C.csls_value(s64, r1, r2)
    rid = np.arange(len(a))
    held = C.third_best_held(c32, rid, 0.6, seed=5)
    return a, b, r1, r2, c32, c64, rid, held


@pytest.mark.parametrize("name", list(FAMILIES))
def test_c_bounds_against_float32_and_float64(name):
    a, b, r1, r2, c32, c64, _, _ = setup(name)
    assert np.isfinite(r1).all() and np.isfinite(r2).all()
    sc = C.screen(a, b, FAMILIES[name]["ks"][0], r1, r2)
    for c, what in ((c32, "float32 product"), (c64, "float64 product")):
        assert (sc["c_lo"] <= c).all() and (c <= sc["c_hi"]).all(), (name, what)
    width = (sc["c_hi"].astype(np.float64) - sc["c_lo"]).max()
    print("%s: max(c_hi - c_lo) = %.3e, 2 max e = %.3e" % (name, width, 2 * sc["e"].max()))


@pytest.mark.parametrize("viable", [False, True], ids=["all", "viable"])
@pytest.mark.parametrize("name,k", CASES)
def test_pruned_set_contains_topk_and_lists_fit(name, k, viable):
    a, b, r1, r2, c32, c64, rid, held = setup(name)
    sc = C.screen(a, b, k, r1, r2, held if viable else None, rid)
    for c in (c32, c64):
        ok = held.viable(c, rid) if viable else None
        top = C.topk_of(c, k, ok)
        got = np.take_along_axis(sc["kept"], np.maximum(top, 0), axis=1) | (top < 0)
        assert got.all()
        count = ok.sum(1) if viable else np.full(len(a), b.shape[0])
        assert (sc["kept"].sum(1) >= np.minimum(k, count)).all()
    must = C.must_overflow(c32, k, held.viable(c32, rid) if viable else None)
    fit = ~must
    print("%s k=%d %s: %d rows must overflow; list length mean %.1f max %d, kept mean %.1f max %d (rows that fit)"
          % (name, k, "viable" if viable else "all", must.sum(), sc["list_len"][fit].mean() if fit.any() else 0,
             sc["list_len"][fit].max() if fit.any() else 0, sc["kept"][fit].sum(1).mean() if fit.any() else 0,
             sc["kept"][fit].sum(1).max() if fit.any() else 0))
    assert (sc["list_len"][fit] <= R.CAP).all()
    assert (sc["list_len"][must] > R.CAP).all()
    # the families' own statement of it: the repeated row overflows everywhere, nothing else does under CSLS
    assert must.all() if name == "overflow" else not must.any()


def test_plain_form_is_screen_ref():
    """r1 = r2 = None decides on s: the restatement is screen_ref.screen's, zero rows of A overflowing included"""
    f = FAMILIES["unnormalised"]
    k = f["ks"][0]
    mine, ref = C.screen(f["a"], f["b"], k), R.screen(f["a"], f["b"], k)
    assert np.array_equal(mine["overflow"], ref["overflow"]) and list(np.flatnonzero(mine["overflow"])) == f["overflow_rows"]
    fit = ~ref["overflow"]
    # (lo, hi rounded to float32 here, float64 there: the sets agree up to that rounding)
    assert (np.abs(mine["list_len"][fit] - ref["list_len"][fit]) <= 2).all()


def test_held_predicate_is_the_word_order():
    """Held.viable == the 64-bit word comparison of the kernels: (order-preserving key of c) << 32 | ~id, larger wins"""
    rng = np.random.default_rng(1)
    vals = np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 3.0, -np.inf], dtype=np.float32)
    c = rng.choice(vals, (5, 40))
    held = C.Held(rng.choice(vals, 40), rng.integers(0, 9, 40), rng.random(40) < 0.2)
    rid = np.array([4, 0, 8, 2, 6])
    assert np.array_equal(held.viable(c, rid), C.word(c, rid[:, None]) > C.best_words(held)[None, :])
    assert C.word(np.float32(-0.0), 3) == C.word(np.float32(0.0), 3) and C.word(np.float32(1.0), 2) > C.word(np.float32(1.0), 3)
