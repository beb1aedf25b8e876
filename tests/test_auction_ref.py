"""CPU: the numpy reference of the auction assignment (tests/auction_ref.py) -- the algorithm the rounds kernel is held to bit for
bit -- against its optimality certificate, a brute force over all permutations and, where SciPy is installed, the Hungarian
optimum."""
import itertools

import numpy as np
import pytest

import auction_ref as ar

EPS = 1e-3

# (n1, n2, d, noise, k, csls_k)
SHAPES = [(64, 64, 8, 2.0, 4, 10), (64, 64, 8, 2.0, 64, 10), (40, 70, 8, 2.0, 4, 10), (150, 150, 8, 3.0, 8, 10),
          (600, 600, 8, 2.0, 16, 10), (300, 300, 16, 0.3, 8, 10), (64, 64, 8, 2.0, 4, 0)]


def _case(n1, n2, d, noise, csls_k, seed=0):
    a, b, perm = ar.planted(n1, n2, d, noise, seed)
    return ar.csls_matrix(a, b, csls_k), perm


@pytest.mark.parametrize("n1,n2,d,noise,k,csls_k", SHAPES)
def test_reference_meets_the_certificate(n1, n2, d, noise, k, csls_k):
    c, perm = _case(n1, n2, d, noise, csls_k)
    m1, v1, price, stats = ar.auction_dense(c, k, EPS)
    slack, gap, tol = ar.certificate(c, m1, price, EPS)
    print("%dx%d k=%d: %s, slack %.3e (limit %.3e), gap %.3e (limit %.3e)"
          % (n1, n2, k, stats, slack, EPS + 2 * tol, gap, n1 * (EPS + 2 * tol)))
    assert stats["complete"] and stats["unmatched"] == 0
    assert np.abs(v1.astype(np.float64) - c[np.arange(n1), m1]).max() <= 2 * tol
    if k == n2:
        assert stats["refill_rows"] == 0
    if noise < 1:
        assert stats["rounds"] == 1 and np.array_equal(m1, perm)


SEVEN_SEED = 3


def seven():
    """7 x 7 raw similarities whose best permutation beats the runner-up by more than 7 (eps + 2 tol): (c, best permutation)."""
    a, b, _ = ar.planted(7, 7, 8, 2.0, SEVEN_SEED)
    c = ar.csls_matrix(a, b, 0)
    c64 = c.astype(np.float64)
    perms = np.array(list(itertools.permutations(range(7))))
    totals = c64[np.arange(7)[None, :], perms].sum(1)
    order = np.argsort(-totals)
    return c, perms[order[0]], float(totals[order[0]] - totals[order[1]])


def test_seven_by_seven_is_the_brute_force_optimum():
    c, best, margin = seven()
    tol = ar.tolerance(c, [1.0])                     # the prices of this instance stay below 1 (asserted)
    assert margin > 7 * (EPS + 2 * tol), margin
    m1, _, price, stats = ar.auction_dense(c, 2, EPS)
    assert price.max() < 1.0 and stats["complete"]
    assert np.array_equal(m1, best)


@pytest.mark.parametrize("n1,n2,d,noise,k,csls_k", SHAPES)
def test_total_against_scipy_hungarian(n1, n2, d, noise, k, csls_k):
    opt = pytest.importorskip("scipy.optimize")
    c, _ = _case(n1, n2, d, noise, csls_k)
    m1, _, price, _ = ar.auction_dense(c, k, EPS)
    c64 = c.astype(np.float64)
    ri, ci = opt.linear_sum_assignment(c64, maximize=True)
    tol = ar.tolerance(c, price)
    assert c64[np.arange(n1), m1].sum() >= c64[ri, ci].sum() - n1 * (EPS + 2 * tol)


def test_rounds_entry_point_validates_its_arguments_without_a_device():
    import ctypes
    import re
    from jmac_amd import _lib, scoring
    L = _lib.lib()
    p = ctypes.c_void_p(256)                                            # never dereferenced: every call below is refused first

    def call(n1=300, n2=300, k=4, ld=4, eps=1e-3, rounds=1, form=0, n_open=0, ws_bytes=1 << 20):
        return L.jmac_auction_rounds_f32(p, p, p, ld, n1, n2, k, p, p, p, eps, rounds, form, n_open, p, p, ws_bytes, None)
    for k in (0, 1, 65):
        assert call(k=k, ld=64) == -1
    assert call(n2=3) == -1                                             # k > n2
    assert call(ld=3) == -1
    assert call(form=3) == -1 and call(rounds=-1) == -1 and call(rounds=4097) == -1 and call(n_open=-1) == -1
    assert call(form=2, n_open=scoring.AUCTION_QUEUE_ROWS + 1) == -1    # more open rows than the one-workgroup queue holds
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        assert call(eps=eps) == -1
    assert call(n1=2 ** 31, n2=2 ** 31) == -4
    need = int(L.jmac_auction_rounds_workspace_bytes(300, 300))
    assert need >= 300 * 8 + 300 * 4 and call(ws_bytes=need - 1) == -3
    queue = re.search(r"#define\s+JMAC_AUCTION_QUEUE_ROWS\s+(\d+)", open(_lib.HEADER_PATH).read())
    assert int(queue.group(1)) == scoring.AUCTION_QUEUE_ROWS


def test_max_rounds_stops_with_a_partial_matching():
    c, _ = _case(64, 64, 8, 2.0, 10)
    m1, v1, price, stats = ar.auction_dense(c, 4, EPS, max_rounds=1)
    assert stats["complete"] is False and stats["rounds"] == 1 and 0 < stats["unmatched"] < 64
    held = m1[m1 >= 0]
    assert len(np.unique(held)) == len(held) and bool(np.isneginf(v1[m1 < 0]).all())


def test_batching_does_not_change_a_run_on_complete_lists():
    """(with refills it does: a waiting row comes back when its batch ends)"""
    c, _ = _case(64, 64, 8, 2.0, 10)
    one = ar.auction_dense(c, 64, EPS, batch=1)
    big = ar.auction_dense(c, 64, EPS, batch=64)
    assert one[3]["rounds"] == big[3]["rounds"] and one[3]["bids"] == big[3]["bids"]
    assert np.array_equal(one[0], big[0]) and np.array_equal(one[2].view(np.uint32), big[2].view(np.uint32))
