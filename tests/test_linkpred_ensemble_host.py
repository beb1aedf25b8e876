"""CPU: the host side of cross-KG ensemble link prediction -- scoring.link_map, the float64 reference's own reductions
(tests/ensemble_ref.py), and the argument validation of jmac_linkpred_ens_*, which needs no device."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_ref
import linkpred_ref


def test_link_map_fills_minus_one_and_keeps_the_smallest_duplicate():
    from jmac_amd import scoring
    pairs = np.array([[3, 7], [0, 2], [3, 5], [5, 0], [3, 9]])
    link = scoring.link_map(pairs, 6, 10, "cpu")
    assert link.dtype == torch.int32 and link.tolist() == [2, -1, -1, 5, -1, 0]
    assert scoring.link_map(torch.from_numpy(pairs[::-1].copy()), 6, 10, "cpu").tolist() == link.tolist()    # order-independent
    assert scoring.link_map(np.zeros((0, 2), dtype=np.int64), 4, 3, "cpu").tolist() == [-1] * 4


@pytest.mark.parametrize("bad", [[[6, 0]], [[-1, 0]], [[0, 10]], [[0, -1]]])
def test_link_map_refuses_ids_outside_their_kg(bad):
    from jmac_amd import scoring
    with pytest.raises(ValueError):
        scoring.link_map(np.array(bad), 6, 10, "cpu")


def _members(rng, N, rows, d, nl, nrel, weights, links=None):
    mk = lambda n: [rng.standard_normal((n, d)) for _ in range(nl)]
    out = [(mk(N), mk(nrel), None, weights[0])]
    for s, n in enumerate(rows):
        link = links[s] if links is not None else np.where(rng.random(N) < 0.5, rng.integers(0, n, N), -1)
        out.append((mk(n), mk(nrel), link, weights[s + 1]))
    return out


def test_reference_reduces_to_the_target_and_to_the_weight_sum():
    rng = np.random.default_rng(0)
    N, B = 40, 9
    h, r = rng.integers(0, N, B), rng.integers(0, 5, B)
    m = _members(rng, N, [30, 50], 6, 2, 5, (1.0, 0.0, 0.0))
    d0 = linkpred_ref.dist64(m[0][0], m[0][1], h, r)
    assert (ensemble_ref.D64(m, h, r) == d0).all()                       # weights (1, 0, ...): the target's dist64
    none = [np.full(N, -1), np.full(N, -1)]
    m = _members(rng, N, [30, 50], 6, 2, 5, (0.5, 0.25, 0.25), links=none)
    d0 = linkpred_ref.dist64(m[0][0], m[0][1], h, r, True)
    assert np.allclose(ensemble_ref.D64(m, h, r, True), d0, rtol=4e-16, atol=0)      # no links: sum(w) d_0 (two roundings)
    m = [(e, x, l, w) for (e, x, l, _), w in zip(m, (1.0, 1.0, 2.0))]
    assert (ensemble_ref.D64(m, h, r, True) == 4.0 * d0).all()           # ... exactly where the products and sums are exact
    # a linked pair takes the support's distance at the linked rows
    link = np.full(N, -1)
    link[[3, 4]] = [7, 2]
    m = _members(rng, N, [30], 6, 2, 5, (0.0, 1.0), links=[link])
    D = ensemble_ref.D64(m, [3, 5], [1, 1])
    ds = linkpred_ref.dist64(m[1][0], m[1][1], [7], [1])
    d0 = linkpred_ref.dist64(m[0][0], m[0][1], [3, 5], [1, 1])
    assert D[0, 4] == ds[0, 2] and D[0, 3] == ds[0, 7] and D[0, 5] == d0[0, 5] and (D[1] == d0[1]).all()
    assert ensemble_ref.ranks(np.array([[1.0, 0.5, 1.0, 0.5]]), [2]).tolist() == [4]
    assert ensemble_ref.ranks(np.array([[1.0, 0.5, 1.0, 0.5]]), [1], np.array([[False, False, False, True]])).tolist() == [1]


def _abi_members(n, links, weights, N=50):
    from jmac_amd import _lib
    p = ctypes.c_void_p(16).value
    lay = (_lib.LinkLayer * 2)(*[_lib.LinkLayer(p, 8, p, 8, p, 8) for _ in range(2)])
    arr = (_lib.LinkMember * max(n, 1))()
    for g in range(min(n, len(arr))):
        arr[g] = _lib.LinkMember(lay, p if links[g] else None, N if g == 0 else 40, weights[g])
    return arr, lay


def test_ensemble_entry_points_validate_without_a_device():
    from jmac_amd import _lib
    L = _lib.lib()
    assert L.jmac_version() >= 138
    p = ctypes.c_void_p(16)
    B, N, d, nl, k = 4, 50, 8, 2, 3
    EINVAL, EWORKSPACE = -1, -3
    assert b"workspace" in L.jmac_strerror(EWORKSPACE)

    def rank(arr, n, ws_bytes=None):
        need = L.jmac_linkpred_ens_rank_workspace_bytes(B, d, nl, max(n, 1))
        return L.jmac_linkpred_ens_rank_f32(arr, n, nl, p, p, 0, p, None, B, N, d, p, p, need if ws_bytes is None else ws_bytes, None)

    def topk(arr, n, ws_bytes=None, kk=k):
        need = L.jmac_linkpred_ens_topk_workspace_bytes(B, N, d, nl, max(n, 1), k)
        return L.jmac_linkpred_ens_topk_f32(arr, n, nl, p, p, 0, None, B, N, d, kk, p, p, p, need if ws_bytes is None else ws_bytes, None)

    w = (0.5, 0.25, 0.25, 0.0, 0.0)
    for call in (rank, topk):
        for n in (0, 5):                                                 # 1 <= n_members <= 4
            arr, keep = _abi_members(n, (False, True, True, True, True), w)
            assert call(arr, n) == EINVAL
        arr, keep = _abi_members(2, (True, True), w)                     # member 0 with a link
        assert call(arr, 2) == EINVAL
        arr, keep = _abi_members(3, (False, True, False), w)             # a supporting member without one
        assert call(arr, 3) == EINVAL
        for bad in (-0.5, float("nan"), float("inf")):
            arr, keep = _abi_members(2, (False, True), (0.5, bad))
            assert call(arr, 2) == EINVAL
        arr, keep = _abi_members(2, (False, True), w, N=49)              # member 0's tables are the N candidates
        assert call(arr, 2) == EINVAL
        arr, keep = _abi_members(3, (False, True, True), w)
        assert call(arr, 3, ws_bytes=64) == EWORKSPACE                   # a short workspace
        assert call(None, 1) == EINVAL
    arr, keep = _abi_members(2, (False, True), w)
    for kk in (0, 65, N + 1):
        assert topk(arr, 2, kk=kk) == EINVAL
    # more members need more workspace: every member has its own query rows
    assert L.jmac_linkpred_ens_rank_workspace_bytes(B, d, nl, 3) > L.jmac_linkpred_ens_rank_workspace_bytes(B, d, nl, 1)
    assert L.jmac_linkpred_ens_topk_workspace_bytes(B, N, d, nl, 3, k) > L.jmac_linkpred_ens_topk_workspace_bytes(B, N, d, nl, 1, k)
    assert L.jmac_linkpred_ens_rank_workspace_bytes(B, d, nl, 0) == 0
