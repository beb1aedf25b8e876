"""GPU: the three L1 tile kernels against EACH OTHER, bit for bit -- l1_score_kernel (scoring.l1_scores), link_rank_tile_kernel
(linkpred_topk / linkpred_ranks, and the Manhattan alignment's alignment_topk / alignment_ranks) and link_ens_tile_kernel (the
ensemble forms with the target as the only member) -- on non-integer data at ragged sizes.  The kernels share one tile body and one
sequential sum; every path here is held to another path's bits, so there is no reference and no tolerance anywhere in this file.

One layer only: for more layers linkpred_dist adds per-layer sums where the fused kernels run one sum across the layers, and those
agree to rounding, by design.  Every table has one duplicated row, so every query has an exact tie that the index resolves.
bf16 tables: l1_scores' bf16 form against the link-prediction kernels' (the ensemble and the alignment have no bf16 form)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NREL = 5
# (B, N, d, table is a column slice of a wider tensor, table dtype)
CASES = [
    (37, 61, 7, False, torch.float32),        # scalar loads, one partial tile each way
    (70, 64, 48, False, torch.float32),       # vector loads, two row tiles, one exact column tile
    (5, 33, 30, False, torch.float32),        # d % 4 != 0 with more than one slab
    # a leading dimension that is no multiple of 4.  The wrappers copy such a table, so through them this case runs the vector
    # form again, on other data; the scalar form at d % 4 == 0 is reached by test_scalar_form_at_d_multiple_of_4 alone
    (70, 64, 48, True, torch.float32),
    (37, 61, 7, False, torch.bfloat16),
    (70, 64, 48, False, torch.bfloat16),
]
IDS = ["%dx%dx%d%s-%s" % (B, N, d, "-slice" if sl else "", "bf16" if dt == torch.bfloat16 else "f32") for B, N, d, sl, dt in CASES]
F32 = [i for i, c in enumerate(CASES) if c[4] == torch.float32]


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(i):
    """The inputs of case i, S = l1_scores(q, E) and the single-KG top-k of all N candidates: computed once, never modified."""
    from jmac_amd import scoring
    B, N, d, sliced, dtype = CASES[i]
    gen = torch.Generator().manual_seed(100 + i)
    wide = torch.randn(N, d + 5, generator=gen)
    wide[N - 1, 1:1 + d] = wide[2, 1:1 + d]                    # rows 2 and N - 1 of the table are equal: a tie in every row
    wide = wide.cuda()
    E = wide[:, 1:1 + d] if sliced else wide[:, 1:1 + d].contiguous()
    R = torch.randn(NREL, d, generator=gen).cuda()
    h = torch.randint(0, N, (B,), generator=gen).cuda()
    r = torch.randint(0, NREL, (B,), generator=gen).cuda()
    q = E[h] + R[r]                                             # fp32, as the prep kernel forms it
    if dtype == torch.bfloat16:
        S = scoring.l1_scores(q.to(torch.bfloat16), E.to(torch.bfloat16))
    else:
        S = scoring.l1_scores(q, E.contiguous())
    assert S.shape == (B, N) and torch.equal(S[:, 2], S[:, N - 1])
    idx, val = scoring.linkpred_topk([E], [R], h, r, N, table_dtype=dtype)
    return dict(B=B, N=N, d=d, dtype=dtype, wide=wide, E=E, R=R, h=h, r=r, q=q, S=S, idx=idx, val=val)


def _sorted_rows(S):
    """Every row of S in ascending order, equal values by ascending index."""
    val, idx = torch.sort(S, dim=1, stable=True)
    return idx, val


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_topk_is_the_sorted_score_row(i):
    c = _case(i)
    idx, val = _sorted_rows(c["S"])
    assert torch.equal(c["idx"], idx)
    assert torch.equal(_bits(c["val"]), _bits(val))


@pytest.mark.parametrize("i", F32, ids=[IDS[i] for i in F32])
def test_single_member_ensemble_is_the_single_kg_call(i):
    from jmac_amd import scoring
    c = _case(i)
    idx, val = scoring.linkpred_topk_ensemble([([c["E"]], [c["R"]], None, 1.0)], c["h"], c["r"], c["N"])
    assert torch.equal(idx, c["idx"])
    assert torch.equal(_bits(val), _bits(c["val"]))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_jth_prediction_ranks_j_plus_1(i):
    from jmac_amd import scoring
    c = _case(i)
    B, N = c["B"], c["N"]
    hh, rr, gold = c["h"].repeat_interleave(N), c["r"].repeat_interleave(N), c["idx"].reshape(-1)
    want = torch.arange(1, N + 1, dtype=torch.int32, device="cuda").repeat(B)
    rank = scoring.linkpred_ranks([c["E"]], [c["R"]], hh, rr, gold, table_dtype=c["dtype"])
    assert torch.equal(rank, want)
    if c["dtype"] == torch.float32:
        rank = scoring.linkpred_ranks_ensemble([([c["E"]], [c["R"]], None, 1.0)], hh, rr, gold)
        assert torch.equal(rank, want)


@pytest.mark.parametrize("i", F32, ids=[IDS[i] for i in F32])
def test_manhattan_alignment_is_one_minus_the_scores(i):
    from jmac_amd import scoring
    c = _case(i)
    B, N = c["B"], c["N"]
    sim = 1.0 - c["S"]
    assert torch.equal(_bits(scoring.alignment_sim(c["q"], c["E"], "manhattan")), _bits(sim))
    # the columns of 1 - S in descending order, equal values by ascending index (negation is exact)
    order, neg = _sorted_rows(-sim)
    idx, val = scoring.alignment_topk(c["q"], c["E"], min(N, 64), csls_k=0, metric="manhattan")
    assert torch.equal(idx, order)
    assert torch.equal(_bits(val), _bits(-neg))
    # ... and the larger-first count: the j-th column of that order ranks j + 1
    rank = scoring.alignment_ranks(c["q"].repeat_interleave(N, dim=0), c["E"], idx.reshape(-1), csls_k=0, metric="manhattan")
    assert torch.equal(rank, torch.arange(1, N + 1, dtype=torch.int32, device="cuda").repeat(B))


def test_scalar_form_at_d_multiple_of_4():
    """The wrappers copy a strided table into a contiguous one, so the sliced case above reaches the kernels with a leading dimension
    of d.  Here the C entry point gets the slice itself -- leading dimension d + 5 = 53, base 4 bytes off a 16-byte boundary -- and
    must take the scalar form at d % 4 == 0: same top-k, bit for bit, and the j-th prediction ranks j + 1."""
    from jmac_amd import _lib
    i = [n for n, c in enumerate(CASES) if c[3]][0]
    c = _case(i)
    B, N, d, L = c["B"], c["N"], c["d"], _lib.lib()
    E, Ec, R = c["E"], c["E"].contiguous(), c["R"]
    assert E.stride(0) % 4 != 0 and E.data_ptr() % 16 != 0 and d % 4 == 0
    lay = (_lib.LinkLayer * 1)(_lib.LinkLayer(Ec.data_ptr(), Ec.stride(0), R.data_ptr(), R.stride(0), E.data_ptr(), E.stride(0)))
    h, r = c["h"].to(torch.int32), c["r"].to(torch.int32)
    idx = torch.empty((B, N), dtype=torch.int32, device="cuda")
    val = torch.empty((B, N), dtype=torch.float32, device="cuda")
    nbytes = int(L.jmac_linkpred_topk_workspace_bytes(B, N, d, 1, N))
    ws = _lib.workspace(nbytes, "cuda")
    _lib.check(L.jmac_linkpred_topk_f32(lay, 1, _lib.ptr(h), _lib.ptr(r), 0, None, B, N, d, N, _lib.ptr(val), _lib.ptr(idx), _lib.ptr(ws),
                                        nbytes, _lib.stream()), "jmac_linkpred_topk_f32")
    assert torch.equal(idx.to(torch.int64), c["idx"])
    assert torch.equal(_bits(val), _bits(c["val"]))
    hh, rr, gold = h.repeat_interleave(N), r.repeat_interleave(N), idx.reshape(-1).contiguous()
    rank = torch.empty(B * N, dtype=torch.int32, device="cuda")
    nbytes = int(L.jmac_linkpred_rank_workspace_bytes(B * N, d, 1))
    ws = _lib.workspace(nbytes, "cuda")
    _lib.check(L.jmac_linkpred_rank_f32(lay, 1, _lib.ptr(hh), _lib.ptr(rr), 0, _lib.ptr(gold), None, None, B * N, N, d, _lib.ptr(rank),
                                        _lib.ptr(ws), nbytes, _lib.stream()), "jmac_linkpred_rank_f32")
    torch.cuda.synchronize()
    assert torch.equal(rank, torch.arange(1, N + 1, dtype=torch.int32, device="cuda").repeat(B))
    # l1_score_kernel's own scalar form at d % 4 == 0: jmac_l1_score_f32 refuses a leading dimension that is no multiple of 4
    # (JMAC_EDIM), so its table is the same slice of a tensor 56 wide -- the base alone rules the 4-element loads out
    wide4 = torch.zeros((N, 56), device="cuda")
    E4 = wide4[:, 1:1 + d]
    E4.copy_(E)
    assert E4.stride(0) % 4 == 0 and E4.data_ptr() % 16 != 0
    S = torch.empty((B, N), device="cuda")
    q = c["q"].contiguous()
    _lib.check(L.jmac_l1_score_f32(_lib.ptr(q), q.stride(0), _lib.ptr(E4), E4.stride(0), B, N, d, _lib.ptr(S), S.stride(0), 0,
                                   _lib.stream()), "jmac_l1_score_f32")
    assert torch.equal(_bits(S), _bits(c["S"]))
