"""CPU: the reference the GPU tests of the stable alignment compare against (tests/stable_ref.py) is itself right -- a hand-worked
instance, stability (no blocking pair) on random and heavily tied instances, the all-equal matrix, and independence of the order
in which suitors are taken up."""
import numpy as np
import pytest

import stable_ref


def test_hand_worked_instance():
    """Suitors' lists: s0: r0 r1 r3 r2; s1: r0 r1 r2 r3; s2: r1 r2 r0 r3; s3: r0 r1 r2 r3.  Reviewers: r0: s0 s1 s3 s2 (the 9s tie,
    lower id first); r1: s0 s2 s3 s1; r2: s2 s3 s1 s0.  s0 takes r0; s1 loses the tie at r0, takes r1; s2 (8) displaces s1 (7) at
    r1; s1 takes r2; s3 loses both ties at r0 and r1, displaces s1 (6 > 3) at r2; s1 ends at r3."""
    c = np.array([[9, 8, 1, 2],
                  [9, 7, 3, 1],
                  [5, 8, 6, 2],
                  [9, 8, 6, 4]], dtype=np.float32)
    m1, m2 = stable_ref.stable_dense(c)
    assert m1.tolist() == [0, 3, 1, 2] and m2.tolist() == [0, 2, 3, 1]
    assert stable_ref.blocking_pairs(c, m1) == 0
    assert stable_ref.blocking_pairs(c, [1, 0, 2, 3]) > 0
    # the same instance as lists cut after two entries: s1 and s3 run out
    idx = np.array([[0, 1], [0, 1], [1, 2], [0, 1]])
    val = np.take_along_axis(c, idx, 1)
    l1, l2 = stable_ref.stable_lists(idx, val, 4)
    assert l1.tolist() == [0, -1, 1, -1] and l2.tolist() == [0, 2, -1, -1]


@pytest.mark.parametrize("n1,n2", [(40, 40), (30, 50), (50, 30)])
@pytest.mark.parametrize("quantum", [0.0, 0.25])
def test_no_blocking_pairs_and_order_independence(n1, n2, quantum):
    rng = np.random.default_rng(n1 * 100 + n2)
    for _ in range(5):
        c = rng.standard_normal((n1, n2)).astype(np.float32)
        if quantum:
            c = np.round(c / quantum) * np.float32(quantum)          # many exact ties
        m1, m2 = stable_ref.stable_dense(c)
        assert stable_ref.blocking_pairs(c, m1) == 0
        assert int((m1 >= 0).sum()) == min(n1, n2) == int((m2 >= 0).sum())
        assert all(m2[m1[i]] == i for i in range(n1) if m1[i] >= 0)
        for _ in range(3):
            o1, o2 = stable_ref.stable_dense(c, order=rng.permutation(n1))
            assert np.array_equal(o1, m1) and np.array_equal(o2, m2)
        # full lists in value order are the dense instance
        idx = np.argsort(-c, axis=1, kind="stable")
        l1, l2 = stable_ref.stable_lists(idx, np.take_along_axis(c, idx, 1), n2, order=rng.permutation(n1))
        assert np.array_equal(l1, m1) and np.array_equal(l2, m2)


def test_all_equal_matrix_matches_i_with_i():
    m1, m2 = stable_ref.stable_dense(np.full((25, 25), 0.5, dtype=np.float32))
    assert m1.tolist() == list(range(25)) and m2.tolist() == list(range(25))
    m1, _ = stable_ref.stable_dense(np.zeros((30, 20), dtype=np.float32), order=list(reversed(range(30))))
    assert m1.tolist() == list(range(20)) + [-1] * 10


def test_pack_word_orders_like_the_relation():
    v = np.array([-np.inf, -2.5, -0.0, 0.0, 1e-30, 0.25, 0.25, 3.0], dtype=np.float32)
    i = np.array([3, 1, 9, 2, 0, 7, 4, 5])
    w = stable_ref.pack_word(v, i)
    for a in range(len(v)):
        for b in range(len(v)):
            want = v[a] > v[b] or (v[a] == v[b] and i[a] < i[b])
            assert bool(w[a] > w[b]) == bool(want), (a, b)
    assert int(w.min()) > 0                                          # 0 stays "nothing held"
