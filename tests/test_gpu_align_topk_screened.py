"""GPU: the screened alignment entries (jmac_sim_csls_topk_screened_f32, jmac_sim_csls_topk_viable_screened_f32; scoring's
``screen="bf16"``) return the fp32 entries' indices AND values bit for bit on every input family of screen_ref.py -- with csls_k = 10
terms (sub_bound_gaps and overflow have 8 and 6 rows: that many neighbours, the most csls_terms takes), with csls_k = 0 and with
Sinkhorn terms -- and the screen really ran: a row's n_rescored is -1 exactly where the numpy restatement (screen_csls_ref.py) lists
more than the kernel's capacity, and at least min(k, viable columns) everywhere else.  The viable entry screens calls of 256 rows
and more (fewer run the fp32 code: measured), so its tests repeat a family's rows up to that count under ids of
their own -- duplicate rows, whose ties the ids decide.  (The restatement's list lengths are the
kernel's up to the roundings of the bf16 product: a row within 32 entries of the capacity is asserted on neither side; with
csls_k = 10 no row is, see test_sim_screen_csls_ref.py.)  N just past 8192 is the smallest width that reaches the screened path."""
import functools

import numpy as np
import pytest
import torch

import screen_csls_ref as C
import screen_ref as R

pytestmark = pytest.mark.gpu

FAMILIES = R.families()
CASES = [(name, k) for name, f in FAMILIES.items() for k in sorted(set(f["ks"] + [16]))]
BAND = 32


def _same(got, want):
    """(idx, val) pairs, bit for bit"""
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def _c(a, b, r1, r2):
    """the fp32 entries' c as a stored matrix (numpy): 2 s is exact, each subtraction rounds once -- csls_value's bits"""
    from jmac_amd import scoring
    s = scoring.sim_matrix(a, b)
    return (s if r1 is None else (2.0 * s - r1[:, None]) - r2[None, :]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def dev(name, kind="csls"):
    """a, b on the device; the terms of `kind` (csls: csls_terms with min(10, n1) neighbours; sinkhorn: sinkhorn_terms; none) and c"""
    from jmac_amd import scoring
    f = FAMILIES[name]
    a, b = torch.from_numpy(f["a"]).cuda(), torch.from_numpy(f["b"]).cuda()
    ck = min(10, a.shape[0])
    if kind == "csls":
        r1, r2 = scoring.csls_terms(a, b, ck, "inner")
    elif kind == "sinkhorn":
        r1, r2 = scoring.sinkhorn_terms(a, b, metric="inner")
        assert bool(torch.isfinite(r1).all()) and bool(torch.isfinite(r2).all())
    else:
        r1 = r2 = None
    return a, b, ck, r1, r2, _c(a, b, r1, r2)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _check_counts(n, ref, k, count, what):
    """n_rescored against the restatement: -1 where its list is over the capacity, >= min(k, viable columns) where it fits"""
    n = np.asarray(n)
    near = np.abs(ref["list_len"] - R.CAP) <= BAND
    over, fit = ref["overflow"] & ~near, ~ref["overflow"] & ~near
    print("%s: rescored per row mean %.1f max %d, overflow rows %d; restatement kept max %d, list max %d"
          % (what, n[n >= 0].mean() if (n >= 0).any() else 0, n.max(), (n == -1).sum(), ref["kept"][fit].sum(1).max() if fit.any() else 0,
             ref["list_len"].max()))
    assert (n[over] == -1).all()
    assert (n[fit] >= np.minimum(k, count)[fit]).all()
    if fit.any():
        assert n[fit].max() <= 2 * ref["kept"][fit].sum(1).max() + 8


@pytest.mark.parametrize("name,k", CASES)
def test_screened_equals_fp32_entry_csls(name, k):
    from jmac_amd import scoring
    a, b, ck, r1, r2, c = dev(name)
    want = scoring.alignment_topk(a, b, k, csls_k=ck, metric="inner")
    idx, val, st = scoring.alignment_topk(a, b, k, csls_k=ck, metric="inner", screen="bf16", return_stats=True)
    assert _same((idx, val), want)
    ref = C.screen(FAMILIES[name]["a"], FAMILIES[name]["b"], k, _np(r1), _np(r2))
    must = C.must_overflow(c, k)
    assert np.array_equal(ref["overflow"], must) and not (np.abs(ref["list_len"] - R.CAP) <= BAND).any()
    _check_counts(st["n_rescored"].numpy(), ref, k, np.full(len(c), c.shape[1]), "%s k=%d csls" % (name, k))
    assert st["screened"] and st["overflow_rows"] == int(must.sum())
    # the caller's terms give the same call
    assert _same(scoring.alignment_topk(a, b, k, csls_k=ck, metric="inner", terms=(r1, r2), screen="bf16"), want)


@pytest.mark.parametrize("name,k", CASES)
def test_screened_without_terms_is_the_screened_sim_topk(name, k):
    from jmac_amd import scoring
    a, b, _, _, _, _ = dev(name)
    idx, val, st = scoring.alignment_topk(a, b, k, csls_k=0, metric="inner", screen="bf16", return_stats=True)
    widx, wval, wst = scoring.sim_topk(a, b, k, return_values=True, screen="bf16", return_stats=True)
    assert _same((idx, val), (widx, wval)) and torch.equal(st["n_rescored"], wst["n_rescored"])
    assert _same((idx, val), scoring.alignment_topk(a, b, k, csls_k=0, metric="inner"))


@pytest.mark.parametrize("name,k", CASES)
def test_screened_equals_fp32_entry_sinkhorn_terms(name, k):
    from jmac_amd import scoring
    a, b, _, r1, r2, c = dev(name, "sinkhorn")
    want = scoring.alignment_topk(a, b, k, csls_k=1, metric="inner", terms=(r1, r2))
    idx, val, st = scoring.alignment_topk(a, b, k, csls_k=1, metric="inner", terms=(r1, r2), screen="bf16", return_stats=True)
    assert _same((idx, val), want)
    ref = C.screen(FAMILIES[name]["a"], FAMILIES[name]["b"], k, _np(r1), _np(r2))
    _check_counts(st["n_rescored"].numpy(), ref, k, np.full(len(c), c.shape[1]), "%s k=%d sinkhorn" % (name, k))


# ---- the viable form ---------------------------------------------------------------------------------------------------
VIABLE_MIN_ROWS = 256


@functools.lru_cache(maxsize=None)
def tiled(name):
    """dev(name) with the rows of a repeated until there are at least VIABLE_MIN_ROWS (ids 0 .. n-1; the terms and c repeated alike)"""
    a, b, ck, r1, r2, c = dev(name)
    reps = -(-VIABLE_MIN_ROWS // a.shape[0])
    return a.repeat(reps, 1).contiguous(), b, ck, r1.repeat(reps).contiguous(), r2, np.tile(c, (reps, 1)), np.tile(FAMILIES[name]["a"], (reps, 1))


def _words(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).cuda()


def _viable_both(a, b, k, best, ck, terms, row_id=None):
    from jmac_amd import scoring
    want = scoring.alignment_topk_viable(a, b, k, best, row_id, csls_k=ck, metric="inner", terms=terms)
    got = scoring.alignment_topk_viable(a, b, k, best, row_id, csls_k=ck, metric="inner", terms=terms, screen="bf16")
    assert _same(got, want)
    return got


def _viable_counts(a, b, k, r1, r2, rid, best):
    """n_rescored of the viable screened entry (alignment_topk_viable does not return it)"""
    from jmac_amd import scoring
    n = torch.empty(a.shape[0], dtype=torch.int32, device=a.device)
    scoring._csls_topk(a, b, k, r1, r2, "inner", torch.as_tensor(rid, dtype=torch.int32).cuda(), best, screen="bf16", n_rescored=n)
    return n.cpu().numpy()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_viable_with_nothing_held_is_the_plain_form(name):
    from jmac_amd import scoring
    a, b, ck, r1, r2, _, _ = tiled(name)
    best = torch.zeros(b.shape[0], dtype=torch.int64, device="cuda")
    got = _viable_both(a, b, 16, best, ck, (r1, r2))
    assert _same(got, scoring.alignment_topk(a, b, 16, csls_k=ck, metric="inner", terms=(r1, r2)))
    n = _viable_counts(a, b, 16, r1, r2, np.arange(a.shape[0]), best)
    assert (n == -1).all() if name == "overflow" else (n >= 16).all()
    # and without terms: c = s
    got = _viable_both(a, b, 16, best, 0, None)
    assert _same(got, scoring.sim_topk(a, b, 16, return_values=True))


@pytest.mark.parametrize("name", list(FAMILIES))
def test_viable_with_third_best_held(name):
    a, b, ck, r1, r2, c, a_np = tiled(name)
    rid = np.arange(len(c))
    held = C.third_best_held(c, rid, 0.6, seed=11)
    best = _words(C.best_words(held))
    ok = held.viable(c, rid)
    idx, val = _viable_both(a, b, 16, best, ck, (r1, r2))
    # the rows it names are viable, best first, and what is missing of the 16 is (-1, -inf)
    got = idx.cpu().numpy()
    assert np.take_along_axis(ok, np.maximum(got, 0), axis=1)[got >= 0].all()
    assert ((got >= 0).sum(1) == np.minimum(16, ok.sum(1))).all()
    assert bool((val[idx < 0] == float("-inf")).all())
    ref = C.screen(a_np, FAMILIES[name]["b"], 16, _np(r1), _np(r2), held, rid)
    must = C.must_overflow(c, 16, ok)
    assert np.array_equal(ref["overflow"], must)
    _check_counts(_viable_counts(a, b, 16, r1, r2, rid, best), ref, 16, ok.sum(1), "%s k=16 viable" % name)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_viable_with_five_columns_left(name):
    a, b, ck, r1, r2, c, _ = tiled(name)
    n2 = c.shape[1]
    free = np.zeros(n2, dtype=bool)
    left = np.sort(np.random.default_rng(3).permutation(n2)[:5])
    free[left] = True
    held = C.Held(np.full(n2, np.inf, dtype=np.float32), np.zeros(n2, dtype=np.int64), free)       # above any reachable value
    idx, val = _viable_both(a, b, 16, _words(C.best_words(held)), ck, (r1, r2))
    assert bool((idx[:, 5:] == -1).all()) and bool((val[:, 5:] == float("-inf")).all())
    assert bool((idx[:, :5].sort(1).values.cpu() == torch.from_numpy(left)).all())
    n = _viable_counts(a, b, 16, r1, r2, np.arange(a.shape[0]), _words(C.best_words(held)))
    assert (n == 5).all()                                                # five columns can be viable, five are rescored


def test_viable_gathered_rows_and_a_tie_decided_by_the_id():
    """Rows 0, 1 and 3 of the call are the same row of a under the ids 5, 2 and 7; the reviewers of that row's eight best columns
    hold exactly its value under id 5: only id 2 beats them (equal value, lower id)."""
    a, b, ck, r1, r2, c = dev("near_duplicates")
    sel = np.concatenate([[3, 3, 7, 3, 0, 12], np.arange(300) % 30])      # (256 rows and more: the call is screened)
    rid = np.concatenate([[5, 2, 9, 7, 1, 30], 100 + np.arange(300)])
    top8 = np.argsort(-c[3].astype(np.float64), kind="stable")[:8]
    n2 = c.shape[1]
    free = np.ones(n2, dtype=bool)
    free[top8] = False
    held = C.Held(c[3], np.full(n2, 5), free)
    t = torch.from_numpy(sel).cuda()
    idx, val = _viable_both(a[t].contiguous(), b, 16, _words(C.best_words(held)), ck, (r1[t].contiguous(), r2), row_id=rid)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx[1, :8], top8)                              # id 2: the tie goes to the lower id
    assert not np.isin(idx[0], top8).any() and np.array_equal(idx[0], idx[3])      # ids 5 and 7: not viable there
    ok = held.viable(c[sel], rid)
    assert np.array_equal(idx, C.topk_of(c[sel], 16, ok))
    n = _viable_counts(a[t].contiguous(), b, 16, r1[t].contiguous(), r2, rid, _words(C.best_words(held)))
    assert (n >= 16).all()
    # the same call on its first six rows runs the fp32 code, and agrees
    few = _viable_counts(a[t[:6]].contiguous(), b, 16, r1[t[:6]].contiguous(), r2, rid[:6], _words(C.best_words(held)))
    assert (few == -2).all()
    idx6, _ = _viable_both(a[t[:6]].contiguous(), b, 16, _words(C.best_words(held)), ck, (r1[t[:6]].contiguous(), r2), row_id=rid[:6])
    assert np.array_equal(idx6.cpu().numpy(), idx[:6])


# ---- the matching runs -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded(n1=300, n2=8300, d=32):
    """ten crowds of thirty near-identical suitors: every crowd wants the same few reviewers, so lists of 4 run out"""
    gen = torch.Generator().manual_seed(17)
    centres = torch.nn.functional.normalize(torch.randn(10, d, generator=gen), dim=1)
    a = torch.nn.functional.normalize(centres[torch.arange(n1) % 10] + 1e-3 * torch.randn(n1, d, generator=gen), dim=1)
    b = torch.nn.functional.normalize(torch.randn(n2, d, generator=gen), dim=1)
    return a.cuda().contiguous(), b.cuda().contiguous()


def test_stable_alignment_with_the_screen():
    from jmac_amd import scoring
    a, b = crowded()
    m0, v0, s0 = scoring.stable_alignment(a, b, k=4, csls_k=10, metric="inner")
    m1, v1, s1 = scoring.stable_alignment(a, b, k=4, csls_k=10, metric="inner", screen="bf16")
    assert s0["refills"] > 0 and "screen" not in s0
    assert torch.equal(m0, m1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    scr = s1.pop("screen")
    assert s1 == s0
    print("stable: %s; screen %s" % (s0, scr))
    # (a refill is screened when it gathers 256 rows and more: at most the first of this run)
    assert scr["rows"] == 300 and scr["overflow_rows"] == 0 and scr["rescored_mean"] >= 4 and 0 <= scr["refill_calls_screened"] <= s0["refills"]


@pytest.mark.parametrize("transposed", [False, True])
def test_auction_alignment_with_the_screen(transposed):
    """transposed (8300 rows bid for 300 columns): the run works on the transposed instance, so its lists are again 300 rows
    against 8300 columns; the row pass of csls_terms (300 columns) takes the unscreened exit"""
    from jmac_amd import scoring
    a, b = crowded()
    if transposed:
        a, b = b, a
    m0, v0, p0, s0 = scoring.auction_alignment(a, b, k=4, csls_k=10, metric="inner", eps=5e-3)
    m1, v1, p1, s1 = scoring.auction_alignment(a, b, k=4, csls_k=10, metric="inner", eps=5e-3, screen="bf16")
    assert s0["refills"] > 0 and s0["transposed"] == transposed and s0["complete"]
    assert torch.equal(m0, m1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))
    scr = s1.pop("screen")
    assert s1 == s0
    print("auction: %s; screen %s" % (s0, scr))
    # (a refill of fewer than scoring.SCREEN_REFILL_MIN_ROWS rows stays on the fp32 entry)
    assert scr["rows"] == 300 and scr["overflow_rows"] == 0 and 0 <= scr["refill_calls_screened"] <= s0["refills"]


# ---- exits, reproducibility, the model ---------------------------------------------------------------------------------
def test_narrow_exit_takes_the_fp32_code():
    from jmac_amd import scoring
    gen = torch.Generator().manual_seed(3)
    a = torch.nn.functional.normalize(torch.randn(40, 16, generator=gen), dim=1).cuda()
    b = torch.nn.functional.normalize(torch.randn(4000, 16, generator=gen), dim=1).cuda()
    want = scoring.alignment_topk(a, b, 10, csls_k=10, metric="inner")
    idx, val, st = scoring.alignment_topk(a, b, 10, csls_k=10, metric="inner", screen="bf16", return_stats=True)
    assert _same((idx, val), want)
    assert (st["n_rescored"] == -2).all() and not st["screened"] and st["overflow_rows"] == 0
    best = torch.zeros(4000, dtype=torch.int64, device="cuda")
    n = torch.zeros(40, dtype=torch.int32, device="cuda")
    rid = torch.arange(40, dtype=torch.int32, device="cuda")
    got = scoring._csls_topk(a, b, 10, None, None, "inner", rid, best, screen="bf16", n_rescored=n)
    assert _same(got, scoring._csls_topk(a, b, 10, None, None, "inner", rid, best)) and bool((n == -2).all())
    # k = 65 is rejected as it is today, with or without the screen
    big = torch.nn.functional.normalize(torch.randn(8300, 16, generator=gen), dim=1).cuda()
    for screen in (None, "bf16"):
        with pytest.raises(ValueError):
            scoring.alignment_topk(a, big, 65, csls_k=10, metric="inner", screen=screen)
    # the stable run on a narrow table: no refill call is counted as screened
    _, _, stats = scoring.stable_alignment(a, b, k=4, csls_k=10, metric="inner", screen="bf16")
    assert stats["screen"]["refill_calls_screened"] == 0 and stats["screen"]["rows"] == 40


def test_two_calls_return_identical_bits():
    from jmac_amd import scoring
    a, b, ck, r1, r2, c = dev("two_row_tiles")
    first = scoring.alignment_topk(a, b, 25, csls_k=ck, metric="inner", screen="bf16", return_stats=True)
    again = scoring.alignment_topk(a, b, 25, csls_k=ck, metric="inner", screen="bf16", return_stats=True)
    assert _same(first[:2], again[:2]) and torch.equal(first[2]["n_rescored"], again[2]["n_rescored"])
    held = C.third_best_held(c, np.arange(len(c)), 0.6, seed=11)
    best = _words(C.best_words(held))
    one = scoring.alignment_topk_viable(a, b, 25, best, csls_k=ck, metric="inner", terms=(r1, r2), screen="bf16")
    two = scoring.alignment_topk_viable(a, b, 25, best, csls_k=ck, metric="inner", terms=(r1, r2), screen="bf16")
    assert _same(one, two)


def test_model_alignment_topk_passes_the_screen_on():
    """a synthetic pair: 200 entities against 8300 (the second table reaches the screened path)"""
    from jmac_amd import harness, synth
    from jmac_amd.model import JMAC
    torch.manual_seed(0)
    sizes, nr = (200, 8300), 10
    blocks, base = [], 0
    for t, n in enumerate(sizes):
        ei, et = synth.power_law_graph(n, 6 * n, nr, seed=7 + t)[:2]
        blocks.append((torch.as_tensor(np.asarray(ei)).cuda(), torch.as_tensor(np.asarray(et)).cuda(), [base, base + n], [t * nr, (t + 1) * nr]))
        base += n
    args = harness.make_args(dim=32, batch_size=32, num_negative=5, dropout=0.0)
    name_emb = np.random.default_rng(0).standard_normal((base, 24)).astype(np.float32)
    model = JMAC(args, name_emb, 2 * nr, base).cuda().eval()
    q = np.arange(0, 200, 3)
    with torch.no_grad():
        emb = tuple(e for e, _ in model.get_emb_blocks(blocks, on_device=True))
        want = model.alignment_topk(q, 5, blocks, emb=emb)
        got = model.alignment_topk(q, 5, blocks, emb=emb, screen="bf16")
        m0 = model.alignment_stable(q, blocks, k=4, emb=emb)
        m1 = model.alignment_stable(q, blocks, k=4, emb=emb, screen="bf16")
    assert emb[1].shape[0] == 8300 and _same(got, want)
    assert torch.equal(m0[0], m1[0]) and "screen" in m1[2] and m1[2]["screen"]["rows"] == len(q)
