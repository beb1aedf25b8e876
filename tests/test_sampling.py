"""CPU: the true-tail CSR of jmac_amd.sampling equals data.true_tail_dict, and the numpy restatement of the sampler's stream
definition (tests/sampler_ref.py, what the GPU tests compare the kernel with bit for bit) has the reference's distribution:
a uniform draw without replacement from the entities that are not a true tail (modules/load/data_loader.py:36-47)."""
import os

import numpy as np
import pytest
import torch

import sampler_ref
from conftest import GOLDEN
from jmac_amd import data
from jmac_amd.sampling import CompletionSampler, TrueTailIndex


def _triple_lists():
    kgs, _, _, _ = data.load_dbp5l(os.path.join(GOLDEN, "dbp5l_mini"), "ja")
    z = data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz"))
    return [("mini-" + l, kgs[l].train_data) for l in sorted(kgs)] + [("ja", z["ja.train"]), ("el", z["el.train"])]


@pytest.mark.parametrize("name,triples", _triple_lists(), ids=[n for n, _ in _triple_lists()])
def test_true_tail_index_equals_true_tail_dict(name, triples):
    triples = np.asarray(triples, dtype=np.int64)
    want = data.true_tail_dict(triples)
    ix = TrueTailIndex.from_triples(triples, "cpu")
    assert ix.tail_ptr.dtype == torch.int32 and ix.tail_idx.dtype == torch.int32 and ix.key_of_triple.dtype == torch.int32
    keys, ptr, idx, kot = ix.keys.numpy(), ix.tail_ptr.numpy(), ix.tail_idx.numpy(), ix.key_of_triple.numpy()
    assert [tuple(k) for k in keys.tolist()] == list(want)                   # same keys, same (lexicographic) order
    assert ptr[0] == 0 and ptr[-1] == len(idx) == sum(len(v) for v in want.values())
    for i, v in enumerate(want.values()):
        assert np.array_equal(idx[ptr[i]:ptr[i + 1]], v)                     # sorted distinct tails
    assert np.array_equal(keys[kot], triples[:, :2])
    assert ix.longest() == max(len(v) for v in want.values())


def test_restatement_draws_uniformly_without_replacement_from_the_allowed_entities():
    """num_ent = 40, tails {0, 2, .., 18}, K = 5, rows 0..19999, seed words (12345, 0), step 0.  Under the claim the first
    slot's counts over the 30 allowed entities are multinomial(20000, 1/30): Pearson's chi-square has df = 29 and the bound
    df + 6 sqrt(2 df) = 74.7 is exceeded with probability far below 1e-6.  Found: 24.26 (seed words (1, 0): 29.90; (2, 0): 31.16)."""
    num_ent, K, rows = 40, 5, 20000
    tails = list(range(0, 20, 2))
    neg = sampler_ref.negatives(range(rows), [tails] * rows, num_ent, K, (12345, 0), 0)
    assert neg.shape == (rows, K) and neg.min() >= 0 and neg.max() < num_ent
    assert not np.isin(neg, tails).any()                                     # no forbidden entity
    s = np.sort(neg, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all()                                     # no repeat in a row
    allowed = np.setdiff1d(np.arange(num_ent), tails)
    counts = np.bincount(neg[:, 0], minlength=num_ent)[allowed]
    expect = rows / len(allowed)
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    df = len(allowed) - 1
    print("chi-square of the first slot: %.2f (df = %d)" % (chi2, df))
    assert chi2 <= df + 6 * np.sqrt(2 * df)


def test_restatement_returns_the_whole_allowed_set_when_it_has_exactly_k_members():
    neg = sampler_ref.negatives(range(50), [range(40)] * 50, 70, 30, (7, 9), 3)
    assert (np.sort(neg, axis=1) == np.arange(40, 70)).all()
    assert len({tuple(r) for r in neg.tolist()}) > 1                         # ... in an order that differs from row to row


def test_restatement_depends_on_row_step_and_both_seed_words():
    base = sampler_ref.negatives([0, 1], [[], []], 1000, 8, (5, 6), 0)
    assert not np.array_equal(base[0], base[1])
    for seed, step in (((5, 7), 0), ((4, 6), 0), ((5, 6), 1), ((5, 6), 1 << 32)):
        assert not np.array_equal(sampler_ref.negatives([0, 1], [[], []], 1000, 8, seed, step), base)


def test_a_key_that_leaves_fewer_than_k_entities_is_refused():
    tr = np.array([[0, 0, t] for t in range(1, 8)] + [[1, 0, 2]], dtype=np.int64)      # (0, 0) has 7 true tails of 10 entities
    with pytest.raises(ValueError, match="fewer than num_negative"):
        CompletionSampler(tr, 10, 2, 4, "cpu")
    with pytest.raises(ValueError):
        CompletionSampler(tr, 10, 2, 65, "cpu")                              # K > 64
    with pytest.raises(ValueError):
        CompletionSampler(tr, 10, 9, 2, "cpu")                               # batch larger than the list
    with pytest.raises(IndexError):
        CompletionSampler(tr, 7, 2, 2, "cpu")                                # tail 7 with 7 entities


def test_entry_point_validates_its_arguments_without_a_device():
    import ctypes
    from jmac_amd import _lib
    f = _lib.lib().jmac_sample_completion_batch
    p = ctypes.c_void_p(16)
    ok = dict(T=100, num_ent=50, B=10, K=5)

    def call(ptr=p, **kw):
        a = dict(ok, **kw)
        return f(ptr, a["T"], p, p, p, p, a["num_ent"], a["B"], a["K"], p, p, p, p, p, None)
    assert call(K=0) == -1 and call(K=65) == -1                             # 1 <= K <= 64
    assert call(B=0) == -1 and call(T=9) == -1 and call(num_ent=0) == -1    # B >= 1, T >= B
    assert call(num_ent=1 << 31) == -4 and call(B=1 << 31, T=1 << 32) == -4
    assert call(ptr=None) == -1                                             # null pointer
