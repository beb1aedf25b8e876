"""GPU: jmac_sim_topk_screened_f32 (scoring.sim_topk(..., screen="bf16")) returns jmac_sim_topk_f32's indices AND values bit for
bit on every input family of screen_ref.py, and the screen really ran: outside the rows that must overflow (the overflow family;
the zero rows of A in the un-normalised one, whose N scores all tie -- test_sim_screen_ref.py asserts both sides of that on the
host) every row rescored at least k columns and none fell back (n_rescored >= k, never -1).  N just past 8192 is the smallest width
that reaches the screened path; N = 4000 and k = 65 take the unscreened exit (n_rescored == -2).  The return-code test needs no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import screen_ref as R

FAMILIES = R.families()
CASES = [(name, k) for name, f in FAMILIES.items() for k in f["ks"]]


def _same(got, want):
    """(idx, val) pairs, bit for bit"""
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def _both(a, b, k):
    from jmac_amd import scoring
    want = scoring.sim_topk(a, b, k, return_values=True)
    idx, val, st = scoring.sim_topk(a, b, k, return_values=True, screen="bf16", return_stats=True)
    return want, (idx, val), st


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", CASES)
def test_screened_equals_fp32_entry(name, k):
    f = FAMILIES[name]
    a, b = torch.from_numpy(f["a"]).cuda(), torch.from_numpy(f["b"]).cuda()
    want, got, st = _both(a, b, k)
    assert _same(got, want)
    n = st["n_rescored"].numpy()
    must = np.zeros(len(n), dtype=bool)
    must[f["overflow_rows"] if f["overflow_rows"] is not None else slice(None)] = True
    print("%s k=%d: rescored per row mean %.1f max %d, overflow rows %d" % (name, k, st["rescored_mean"], st["rescored_max"], st["overflow_rows"]))
    assert (n[must] == -1).all()
    assert (n[~must] >= k).all()
    assert st["screened"] and st["overflow_rows"] == int(must.sum())
    # the numpy restatement's pruned set is the kernel's up to the roundings of sh: the same order of magnitude, never the whole list
    if (~must).any():
        ref = R.screen(f["a"], f["b"], k)
        assert n[~must].max() <= 2 * ref["kept"][~must].sum(1).max() + 8


@pytest.mark.gpu
def test_near_duplicates_are_ordered_by_the_exact_scores():
    """The first query is base row 0.  Its 40 perturbed copies (1e-5: invisible in bf16) score 1 +- 1e-5, its 12 exact copies all
    the same value in between, every other column far less: the top 64 carry the fp32 product's own values in descending order,
    ties in index order, and the 12 exact copies sit next to each other in index order."""
    from jmac_amd import scoring
    f = FAMILIES["near_duplicates"]
    a, b = torch.from_numpy(f["a"]).cuda(), torch.from_numpy(f["b"]).cuda()
    idx, val = scoring.sim_topk(a, b, 64, return_values=True, screen="bf16")
    s = scoring.sim_matrix(a[:1].contiguous(), b)[0]
    i, v = idx[0], val[0]
    exact = (b == a[0]).all(1).nonzero().flatten()
    assert len(exact) == 12
    assert torch.equal(v, s[i])
    assert (v[:-1] >= v[1:]).all()
    tie = v[:-1] == v[1:]
    assert (i[:-1][tie] < i[1:][tie]).all()
    pos = torch.isin(i, exact).nonzero().flatten()
    assert len(pos) == 12 and torch.equal(pos, torch.arange(int(pos[0]), int(pos[0]) + 12, device=pos.device))
    assert torch.equal(i[pos], exact) and (v[pos] == v[pos[0]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N,k", [(4000, 10), (8300, 65)])
def test_narrow_exits_take_the_fp32_code(N, k):
    gen = torch.Generator().manual_seed(3)
    a = torch.nn.functional.normalize(torch.randn(9, 16, generator=gen), dim=1).cuda()
    b = torch.nn.functional.normalize(torch.randn(N, 16, generator=gen), dim=1).cuda()
    want, got, st = _both(a, b, k)
    assert _same(got, want)
    assert (st["n_rescored"] == -2).all() and not st["screened"] and st["overflow_rows"] == 0


@pytest.mark.gpu
def test_empty_problem_and_optional_outputs():
    from jmac_amd import scoring
    b = torch.from_numpy(FAMILIES["random_unit"]["b"]).cuda()
    a = torch.from_numpy(FAMILIES["random_unit"]["a"]).cuda()
    idx, val, st = scoring.sim_topk(a[:0], b, 5, return_values=True, screen="bf16", return_stats=True)
    assert idx.shape == (0, 5) and val.shape == (0, 5) and st["rows"] == 0 and st["overflow_rows"] == 0
    # val and n_rescored are optional: indices alone
    assert torch.equal(scoring.sim_topk(a, b, 25, screen="bf16"), scoring.sim_topk(a, b, 25))


@pytest.mark.gpu
def test_get_neg_forms_pass_the_screen_on():
    from jmac_amd import scoring
    f = FAMILIES["two_row_tiles"]
    src, dst = torch.from_numpy(f["a"]).cuda(), torch.from_numpy(f["b"]).cuda()
    ill = [3, 0, 129, 77, 3]
    assert torch.equal(scoring.get_neg(ill, src, dst, 25, screen="bf16"), scoring.get_neg(ill, src, dst, 25))
    ill = [8999, 0, 4242, 17]
    assert torch.equal(scoring.get_neg_dbpv1(ill, dst, 25, screen="bf16"), scoring.get_neg_dbpv1(ill, dst, 25))


@pytest.mark.gpu
def test_two_calls_return_identical_bits():
    from jmac_amd import scoring
    f = FAMILIES["two_row_tiles"]
    a, b = torch.from_numpy(f["a"]).cuda(), torch.from_numpy(f["b"]).cuda()
    first = scoring.sim_topk(a, b, 25, return_values=True, screen="bf16", return_stats=True)
    again = scoring.sim_topk(a, b, 25, return_values=True, screen="bf16", return_stats=True)
    assert _same(first[:2], again[:2]) and torch.equal(first[2]["n_rescored"], again[2]["n_rescored"])


def test_bad_screen_value():
    from jmac_amd import scoring
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        scoring.sim_topk(x, x, 2, screen="fp16")
    with pytest.raises(ValueError):
        scoring.get_neg([0], x, x, 2, screen=True)
    with pytest.raises(ValueError):
        scoring.sim_topk(x, x, 2, return_stats=True)


def test_return_codes_and_workspace():
    """jmac_sim_topk_f32's checks in its order (sizes > empty problem > pointers > strides > workspace; val optional), plus
    JMAC_EDIM for d % 4 and d > 512 and JMAC_ERANGE for 2^31 rows, both ahead of the workspace check.  No device is touched."""
    from jmac_amd import _lib
    OK, EINVAL, EDIM, EWORKSPACE, ERANGE = 0, -1, -2, -3, -4
    P, BIG, I31 = ctypes.c_void_p(16), 1 << 40, 2 ** 31 - 1
    base = dict(A=P, lda=8, B=P, ldb=8, L=4, N=100, d=8, k=10, val=P, idx=P, nres=P, ws=P, ws_bytes=BIG, stream=None)
    order = "A lda B ldb L N d k val idx nres ws ws_bytes stream".split()
    L = _lib.lib()
    rows = [
        (dict(L=-1), EINVAL), (dict(N=0), EINVAL), (dict(d=0), EINVAL), (dict(k=0), EINVAL), (dict(N=5, k=6), EINVAL),
        (dict(L=0, A=None, B=None, idx=None, ws=None, ws_bytes=0), OK), (dict(L=0, k=0), EINVAL), (dict(L=0, lda=6), OK), (dict(L=0, d=516), OK),
        (dict(A=None), EINVAL), (dict(B=None), EINVAL), (dict(idx=None), EINVAL), (dict(A=None, ldb=6), EINVAL), (dict(A=None, d=516), EINVAL),
        (dict(lda=6), EDIM), (dict(ldb=6), EDIM), (dict(lda=6, ws=None), EDIM), (dict(d=516), EDIM), (dict(d=516, ws_bytes=0), EDIM),
        (dict(d=6, ws_bytes=0), EDIM), (dict(d=512, ws_bytes=0), EWORKSPACE), (dict(L=I31, ws_bytes=0), ERANGE), (dict(L=I31, d=516), EDIM),
        (dict(ws=None), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE), (dict(k=65, ws_bytes=0), EWORKSPACE),
        (dict(val=None, ws_bytes=0), EWORKSPACE), (dict(nres=None, ws_bytes=0), EWORKSPACE),
    ]
    for over, want in rows:
        args = dict(base, **over)
        assert L.jmac_sim_topk_screened_f32(*[args[f] for f in order]) == want, over
    wsb = L.jmac_sim_topk_screened_workspace_bytes
    # unscreened shapes: the fp32 entry's workspace; screened: bf16 copies + norms + an eighth of the matrix + the lists, no L x N
    assert wsb(100, 4000, 16, 10) == L.jmac_sim_topk_workspace_bytes(100, 4000, 10)
    assert wsb(50, 10000, 16, 65) == L.jmac_sim_topk_workspace_bytes(50, 10000, 65)
    assert wsb(-1, 100, 8, 1) == 0 and wsb(4, 100, 0, 1) == 0 and wsb(4, 100, 8, 0) == 0
    need = wsb(3000, 30000, 300, 25)
    assert 0 < need < 0.3 * 3000 * 30000 * 4
    short = dict(base, L=3000, N=30000, d=300, k=25, ws_bytes=need - 1)
    assert L.jmac_sim_topk_screened_f32(*[short[f] for f in order]) == EWORKSPACE
