"""CPU: the known-tail index that link prediction reads on the device (sampling.TrueTailIndex.from_dict / key_code), the
argument validation and workspace sizes of jmac_linkpred_rank_indexed_* / jmac_linkpred_topk_*, and the float64 top-k helper
the GPU tests compare the kernels with."""
import ctypes
import os

import numpy as np
import pytest
import torch

import linkpred_ref
from conftest import GOLDEN
from jmac_amd import _lib, data
from jmac_amd.sampling import TrueTailIndex


def _triple_lists():
    kgs, _, _, _ = data.load_dbp5l(os.path.join(GOLDEN, "dbp5l_mini"), "ja")
    z = data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz"))
    assert {"ja.train", "ja.val", "ja.test"} <= set(z)
    ja = np.concatenate((z["ja.train"], z["ja.val"], z["ja.test"]))           # what KnowledgeGraph.true_tail is built from
    return [("mini-" + l, kgs[l].train_data) for l in sorted(kgs)] + [("ja", ja)]


@pytest.mark.parametrize("name,triples", _triple_lists(), ids=[n for n, _ in _triple_lists()])
def test_from_dict_equals_from_triples(name, triples):
    triples = np.asarray(triples, dtype=np.int64)
    a = TrueTailIndex.from_triples(triples, "cpu")
    b = TrueTailIndex.from_dict(data.true_tail_dict(triples), "cpu")
    for f in ("keys", "key_code", "tail_ptr", "tail_idx"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), f
    assert b.key_of_triple is None
    code = a.key_code.numpy()
    assert code.dtype == np.int64 and (np.diff(code) > 0).all()             # strictly ascending
    assert np.array_equal(code, a.keys.numpy()[:, 0] * (1 << 32) + a.keys.numpy()[:, 1])
    for i in range(len(code)):                                              # tails sorted and distinct within a key
        seg = a.tail_idx.numpy()[a.tail_ptr[i]:a.tail_ptr[i + 1]]
        assert (np.diff(seg) > 0).all()


def test_from_dict_sorts_and_dedupes_unsorted_lists():
    ix = TrueTailIndex.from_dict({(3, 1): [9, 2, 9, 4], (0, 7): np.array([5]), (3, 0): [1, 0]}, "cpu")
    assert ix.keys.tolist() == [[0, 7], [3, 0], [3, 1]]
    assert ix.tail_ptr.tolist() == [0, 1, 3, 6] and ix.tail_idx.tolist() == [5, 0, 1, 2, 4, 9]
    assert ix.key_code.tolist() == [7, (3 << 32), (3 << 32) | 1]
    with pytest.raises(ValueError):
        TrueTailIndex.from_dict({}, "cpu")
    with pytest.raises(ValueError):
        TrueTailIndex.from_dict({(1 << 31, 0): [1]}, "cpu")


def test_new_entry_points_validate_without_a_device():
    L = _lib.lib()
    assert L.jmac_version() >= 128
    p = ctypes.c_void_p(16)
    layers = (_lib.LinkLayer * 1)(_lib.LinkLayer(16, 8, 16, 8, 16, 8))
    for fn in (L.jmac_linkpred_topk_f32, L.jmac_linkpred_topk_bf16):
        def call(B=4, N=100, d=8, k=5, idx=p, index=None):
            return fn(layers, 1, p, p, 0, index, B, N, d, k, p, idx, p, 1 << 30, None)
        assert call(k=0) == -1 and call(k=-3) == -1                         # k <= 0
        assert call(k=65) == -1                                             # k > 64
        assert call(N=3, k=4) == -1                                         # k > N
        assert call(idx=None) == -1                                         # NULL idx
        assert call(d=513) == -2                                            # d > 512: JMAC_EDIM
        bad = _lib.TailIndex(None, 3, 16, 16)
        assert call(index=ctypes.byref(bad)) == -1                          # an index without keys
        assert call(B=0) == 0
    for fn in (L.jmac_linkpred_rank_indexed_f32, L.jmac_linkpred_rank_indexed_bf16):
        assert fn(layers, 1, p, p, 0, p, None, 4, 100, 8, None, p, 1 << 30, None) == -1      # NULL rank
        assert fn(layers, 1, p, p, 0, None, None, 4, 100, 8, p, p, 1 << 30, None) == -1      # NULL gold
        bad = _lib.TailIndex(16, 3, None, 16)
        assert fn(layers, 1, p, p, 0, p, ctypes.byref(bad), 4, 100, 8, p, p, 1 << 30, None) == -1
        assert fn(layers, 1, p, p, 0, p, None, 4, 100, 8, p, p, 8, None) == -3                # workspace too small
        assert fn(layers, 1, p, p, 0, p, None, 0, 100, 8, p, p, 1 << 30, None) == 0
        assert fn(layers, 1, p, p, 0, p, None, 4, 100, 513, p, p, 1 << 30, None) == -4           # d > 512: JMAC_ERANGE, as the CSR form
        assert L.jmac_linkpred_rank_f32(layers, 1, p, p, 0, p, None, None, 4, 100, 513, p, p, 1 << 30, None) == -4


def test_topk_workspace_holds_no_b_by_n_buffer():
    """N >= 8192: a column sample and the candidate lists, never B x N floats (jmac_sim_topk_f32's layout plus the query rows)."""
    f = _lib.lib().jmac_linkpred_topk_workspace_bytes
    assert 0 < f(1000, 11805, 300, 2, 10) < 1000 * 11805 * 4 // 2
    assert 0 < f(1000, 2000000, 300, 2, 10) < 1000 * 2000000 * 4 // 8
    assert f(10, 100, 8, 1, 0) == 0 and f(-1, 100, 8, 1, 5) == 0


def test_reference_topk_against_brute_force_with_ties():
    rng = np.random.default_rng(5)
    N, B, k = 50, 12, 10
    ent = [rng.integers(-2, 3, (N, 6)).astype(np.float64) for _ in range(2)]       # integer tables: many exact ties
    rel = [rng.integers(-2, 3, (4, 6)).astype(np.float64) for _ in range(2)]
    h, r = rng.integers(0, N, B), rng.integers(0, 4, B)
    tt = {(int(h[b]), int(r[b])): rng.choice(N, int(rng.integers(0, 45)), replace=False) for b in range(B)}
    for pred_head in (False, True):
        d = linkpred_ref.dist64(ent, rel, h, r, pred_head)
        listed = linkpred_ref.listed_mask(h, r, tt, N)
        idx, val = linkpred_ref.topk(d, k, listed)
        ties = 0
        for b in range(B):
            sign = -1.0 if pred_head else 1.0
            brute = []
            for n in range(N):
                if n in set(tt[(int(h[b]), int(r[b]))].tolist()):
                    continue
                dist = sum(np.abs(e[h[b]] + sign * rl[r[b]] - e[n]).sum() for e, rl in zip(ent, rel))
                brute.append((dist, n))
            brute.sort()                                                    # by distance, then by index
            want = brute[:k] + [(np.inf, -1)] * (k - len(brute[:k]))
            assert idx[b].tolist() == [n for _, n in want]
            assert val[b].tolist() == [x for x, _ in want]
            ties += sum(1 for j in range(len(brute[:k]) - 1) if brute[j][0] == brute[j + 1][0])
        assert ties > 0
