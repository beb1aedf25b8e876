"""CPU: the numpy restatement of the truncated sampler (tests/trunc_sampler_ref.py, what the GPU tests compare the kernel with bit
for bit) has the properties the header states: distinct negatives, none a true tail, the first want1 from the eligible neighbours
and no other, the plain sampler's bits without hard negatives, and a uniform choice among the eligible neighbours.  And the
entry point refuses bad arguments before it touches a device."""
import ctypes

import numpy as np

import sampler_ref
import trunc_sampler_ref as ref

NUM_ENT = 200
TAILS = [3, 17, 40, 41, 90]                                                  # 40 = the gold tail
# 16 lanes: 12 eligible; 17 and 40 are true tails, the second 7 repeats lane 0, 200 is out of range
ROW = [7, 17, 55, 7, 120, 199, 40, 0, 200, 63, 64, 65, 150, 151, 152, 153]
ELIGIBLE = [7, 55, 120, 199, 0, 63, 64, 65, 150, 151, 152, 153]


def test_eligibility_drops_true_tails_repeats_and_ids_out_of_range():
    e = ref.eligible(ROW, TAILS, NUM_ENT)
    assert [n for n, ok in zip(ROW, e) if ok] == ELIGIBLE and sum(e) == 12
    assert e[0] and not e[3]                                                 # the first of a repeat counts
    assert not any(ref.eligible([-1, 200, 40, 17], TAILS, NUM_ENT))


def test_negatives_are_distinct_no_true_tail_and_hard_first():
    rows = 300
    for K, n_hard in ((5, 5), (25, 25), (25, 10), (25, 0), (12, 12), (13, 13)):
        neg = ref.negatives(range(rows), [TAILS] * rows, [ROW] * rows, NUM_ENT, K, n_hard, (5, 6), 9)
        assert neg.shape == (rows, K) and neg.min() >= 0 and neg.max() < NUM_ENT
        s = np.sort(neg, axis=1)
        assert (s[:, 1:] != s[:, :-1]).all()                                 # distinct
        assert not np.isin(neg, TAILS).any()                                 # no true tail
        want1 = min(n_hard, len(ELIGIBLE))
        assert np.isin(neg[:, :want1], ELIGIBLE).all()                       # the first want1: eligible neighbours
        if n_hard < len(ELIGIBLE):
            continue                                                         # (the uniform fill may hit a neighbour by chance)
        assert not np.isin(neg[:, want1:], ELIGIBLE).any()                   # all 12 are placed: the rest cannot be one
    # when every eligible neighbour is wanted, each row's first 12 are the whole set, in an order of its own
    neg = ref.negatives(range(50), [TAILS] * 50, [ROW] * 50, NUM_ENT, 13, 13, (5, 6), 9)
    assert (np.sort(neg[:, :12], axis=1) == np.sort(ELIGIBLE)).all()
    assert len({tuple(r) for r in neg[:, :12].tolist()}) > 1


def test_the_rest_of_a_row_is_not_an_eligible_neighbour_unless_by_the_uniform_draw():
    """want1 < A: slots want1..K come from the uniform stream, which skips what stage 1 placed and nothing else."""
    rows, K, n_hard = 200, 25, 10
    neg = ref.negatives(range(rows), [TAILS] * rows, [ROW] * rows, NUM_ENT, K, n_hard, (1, 2), 0)
    plain = sampler_ref.negatives(range(rows), [TAILS] * rows, NUM_ENT, K, (1, 2), 0)
    for i in range(rows):
        hard = neg[i, :n_hard].tolist()
        expect = [c for c in sampler_ref.negatives([i], [TAILS + hard], NUM_ENT, K - n_hard, (1, 2), 0)[0].tolist()]
        assert neg[i, n_hard:].tolist() == expect                            # the plain stream with stage 1's values forbidden
    assert not np.array_equal(neg, plain)


def test_without_hard_negatives_the_output_is_the_plain_samplers():
    rows = 100
    tails = [list(range(i % 7)) for i in range(rows)]
    nbr = np.random.default_rng(0).integers(0, NUM_ENT, (rows, 16))
    for seed, step in (((12345, 0), 0), ((7, 9), 1 << 33)):
        want = sampler_ref.negatives(range(rows), tails, NUM_ENT, 25, seed, step)
        assert np.array_equal(ref.negatives(range(rows), tails, nbr, NUM_ENT, 25, 0, seed, step), want)
        # a table in which no lane is eligible: the row's own true tails
        own = [[t[j % len(t)] if t else -1 for j in range(4)] for t in tails]
        assert np.array_equal(ref.negatives(range(rows), tails, own, NUM_ENT, 25, 25, seed, step), want)


def test_every_eligible_neighbour_is_included_equally_often():
    """20 000 rows that share one (h, r, t): A = 12, want1 = 5.  Under a uniform draw without replacement every eligible
    neighbour is among the five with probability p = 5 / 12, so its count is binomial(20000, p) with standard deviation
    sqrt(20000 p (1 - p)) = 69.7: each of the twelve counts must lie within 5 of them (two-sided tail 6e-7 each)."""
    rows, want1 = 20000, 5
    neg = ref.negatives(range(rows), [TAILS] * rows, [ROW] * rows, NUM_ENT, want1, want1, (12345, 0), 0)
    assert np.isin(neg, ELIGIBLE).all()
    p = want1 / len(ELIGIBLE)
    sd = np.sqrt(rows * p * (1 - p))
    counts = np.array([(neg == e).sum() for e in ELIGIBLE])
    print("inclusion counts (expected %.0f, sd %.1f):" % (rows * p, sd), counts.tolist())
    assert counts.sum() == rows * want1
    assert (np.abs(counts - rows * p) <= 5 * sd).all()
    first = np.array([(neg[:, 0] == e).sum() for e in ELIGIBLE])            # and the first slot alone: p = 1 / 12
    assert (np.abs(first - rows / 12) <= 5 * np.sqrt(rows * (1 / 12) * (11 / 12))).all()


def test_entry_point_validates_its_arguments_without_a_device():
    from jmac_amd import _lib
    f = _lib.lib().jmac_sample_completion_batch_truncated
    p = ctypes.c_void_p(16)
    ok = dict(T=100, num_ent=50, B=10, K=5, ldn=8, M=8, n_hard=5)

    def call(ptr=p, nbr=p, **kw):
        a = dict(ok, **kw)
        return f(ptr, a["T"], p, p, p, p, a["num_ent"], a["B"], a["K"], nbr, a["ldn"], a["M"], a["n_hard"], p, p, p, p, p, None)
    assert call(M=0, ldn=8) == -1 and call(M=65, ldn=65) == -1               # 1 <= M <= 64
    assert call(n_hard=6) == -1 and call(n_hard=-1) == -1                    # 0 <= n_hard <= K
    assert call(ldn=7) == -1                                                 # ldn >= M
    assert call(K=0, n_hard=0) == -1 and call(K=65) == -1 and call(B=0) == -1 and call(T=9) == -1 and call(num_ent=0) == -1
    assert call(num_ent=1 << 31) == -4 and call(B=1 << 31, T=1 << 32) == -4
    assert call(ptr=None) == -1 and call(nbr=None) == -1
