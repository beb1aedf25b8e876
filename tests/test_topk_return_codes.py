"""CPU: the return code of every argument check of the top-k and rank entry points of score.hip, and their precedence.

Validation touches no device.  The pointers are fakes that are never dereferenced: every row ends in a JMAC_E* code or in the
empty-problem JMAC_OK, none passes validation and reaches a launch.  The expected codes are those the library returned before
its three top-k drivers, its two LinkRankArgs fills and its six alignment argument checks were merged."""
import ctypes

import pytest

from jmac_amd import _lib

OK, EINVAL, EDIM, EWORKSPACE, ERANGE = 0, -1, -2, -3, -4
P = ctypes.c_void_p(16)
BIG, I31 = 1 << 40, 2 ** 31 - 1

ALIGN = dict(A=P, lda=8, B=P, ldb=8, L=4, N=100, d=8, r1=None, r2=None, row_id=P, best=P, k=10, gold=P, rank=P, val=P, idx=P, ws=P,
             ws_bytes=BIG, stream=None)
ORDER = {
    "sim_topk": "A lda B ldb L N d k val idx ws ws_bytes stream",
    "topk": "A lda B ldb L N d r1 r2 k val idx ws ws_bytes stream",
    "viable": "A lda B ldb L N d r1 r2 row_id best k val idx ws ws_bytes stream",
    "rank": "A lda B ldb L N d r1 r2 gold rank ws ws_bytes stream",
    "link_topk": "layers nl h r pred_head index B N d k val idx ws ws_bytes stream",
    "link_rank": "layers nl h r pred_head gold filt_ptr filt_idx B N d rank ws ws_bytes stream",
    "link_rank_indexed": "layers nl h r pred_head gold index B N d rank ws ws_bytes stream",
}


def _layers(n=1, **null):
    arr = (_lib.LinkLayer * n)()
    for l in range(n):
        arr[l] = _lib.LinkLayer(16, 8, 16, 8, 16, 8)
    for field in null:
        setattr(arr[n - 1], field, None)
    return arr


def _index(n_keys=3, key=16, tail_ptr=16, tail_idx=16):
    return ctypes.byref(_lib.TailIndex(key, n_keys, tail_ptr, tail_idx))


LINK = dict(layers=_layers(), nl=1, h=P, r=P, pred_head=0, gold=P, filt_ptr=None, filt_idx=None, index=None, B=4, N=100, d=8, k=10,
            rank=P, val=P, idx=P, ws=P, ws_bytes=BIG, stream=None)


def _call(name, form, base, **over):
    args = dict(base, **over)
    return getattr(_lib.lib(), name)(*[args[f] for f in ORDER[form].split()])


# (override, code): checks the four jmac_{sim,l1}_csls_topk{,_viable}_f32 and (without the k rows) the two *_csls_rank_f32 share
SHARED = [
    (dict(L=-1), EINVAL), (dict(N=0), EINVAL), (dict(d=0), EINVAL),
    (dict(r1=P), EINVAL), (dict(r2=P), EINVAL),                                   # one of r1 / r2
    (dict(L=0, A=None, B=None, idx=None, val=None, rank=None, ws=None, ws_bytes=0), OK),
    (dict(A=None), EINVAL), (dict(B=None), EINVAL),
    (dict(lda=6), EDIM), (dict(ldb=6), EDIM),
    (dict(L=I31), ERANGE), (dict(N=I31), ERANGE),
    (dict(ws=None), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE),
    # precedence: EINVAL (sizes) > empty OK > EINVAL (pointers) > EDIM > ERANGE > EWORKSPACE
    (dict(L=0, d=0), EINVAL), (dict(L=0, lda=6), OK), (dict(d=-4, lda=6), EINVAL), (dict(A=None, lda=6), EINVAL),
    (dict(lda=6, L=I31), EDIM), (dict(L=I31, ws_bytes=0), ERANGE), (dict(ldb=2, ws=None), EDIM),
]
TOPK_ONLY = [
    (dict(k=0), EINVAL), (dict(k=65), EINVAL), (dict(N=5, k=6), EINVAL), (dict(idx=None), EINVAL),
    (dict(k=0, lda=6), EINVAL), (dict(k=65, L=0), EINVAL), (dict(L=3, N=8191, k=64, ws_bytes=98560 - 1), EWORKSPACE),
]
RANK_ONLY = [(dict(gold=None), EINVAL), (dict(rank=None), EINVAL), (dict(L=I31, N=I31, ws=None), ERANGE)]
# the asymmetries: (override, code of the sim form, code of the L1 form); a short workspace stops the form that accepts the rest
BY_METRIC = [
    (dict(d=6), EDIM, None), (dict(d=6, ws_bytes=0), EDIM, EWORKSPACE),           # d % 4: the sim forms only
    (dict(lda=2 ** 31), None, ERANGE), (dict(lda=2 ** 31, ws_bytes=0), EWORKSPACE, ERANGE),     # lda an int32: the L1 forms only
]


@pytest.mark.parametrize("metric", ["sim", "l1"])
def test_csls_topk_return_codes(metric):
    plain, viable = "jmac_%s_csls_topk_f32" % metric, "jmac_%s_csls_topk_viable_f32" % metric
    for over, want in SHARED + TOPK_ONLY:
        assert _call(plain, "topk", ALIGN, **over) == want, (plain, over)
        assert _call(viable, "viable", ALIGN, **over) == want, (viable, over)
    for over, sim, l1 in BY_METRIC:
        want = sim if metric == "sim" else l1
        if want is not None:
            assert _call(plain, "topk", ALIGN, **over) == want, (plain, over)
            assert _call(viable, "viable", ALIGN, **over) == want, (viable, over)
    # val: optional in jmac_sim_csls_topk_f32 alone (the short workspace stops that call)
    assert _call(plain, "topk", ALIGN, val=None, ws_bytes=0) == (EWORKSPACE if metric == "sim" else EINVAL)
    assert _call(viable, "viable", ALIGN, val=None, ws_bytes=0) == EINVAL
    assert _call(viable, "viable", ALIGN, row_id=None) == EINVAL
    assert _call(viable, "viable", ALIGN, best=None) == EINVAL
    assert _call(viable, "viable", ALIGN, best=None, lda=6) == EINVAL


@pytest.mark.parametrize("metric", ["sim", "l1"])
def test_csls_rank_return_codes(metric):
    name = "jmac_%s_csls_rank_f32" % metric
    for over, want in SHARED + RANK_ONLY:
        assert _call(name, "rank", ALIGN, **over) == want, (name, over)
    for over, sim, l1 in BY_METRIC:
        want = sim if metric == "sim" else l1
        if want is not None:
            assert _call(name, "rank", ALIGN, **over) == want, (name, over)
    assert _call(name, "rank", ALIGN, L=3, ws_bytes=255) == EWORKSPACE


def test_sim_topk_return_codes():
    """jmac_sim_topk_f32: any k <= N (k > 64 takes the stored path), val optional, no d % 4 and no int32 check of its own."""
    rows = [
        (dict(L=-1), EINVAL), (dict(N=0), EINVAL), (dict(d=0), EINVAL), (dict(k=0), EINVAL), (dict(N=5, k=6), EINVAL),
        (dict(L=0, A=None, B=None, idx=None, ws=None, ws_bytes=0), OK), (dict(L=0, k=0), EINVAL), (dict(L=0, lda=6), OK),
        (dict(A=None), EINVAL), (dict(B=None), EINVAL), (dict(idx=None), EINVAL), (dict(A=None, ldb=6), EINVAL),
        (dict(lda=6), EDIM), (dict(ldb=6), EDIM), (dict(lda=6, ws=None), EDIM),
        (dict(ws=None), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE),
        (dict(k=65, ws_bytes=0), EWORKSPACE), (dict(val=None, ws_bytes=0), EWORKSPACE), (dict(d=6, ws_bytes=0), EWORKSPACE),
        (dict(L=I31, ws_bytes=0), EWORKSPACE), (dict(L=50, N=10000, k=65, ws_bytes=2000384 - 1), EWORKSPACE),
    ]
    for over, want in rows:
        assert _call("jmac_sim_topk_f32", "sim_topk", ALIGN, **over) == want, over


# checks jmac_linkpred_topk_* and jmac_linkpred_rank_* share
LINK_SHARED = [
    (dict(B=-1), EINVAL), (dict(N=0), EINVAL), (dict(d=0), EINVAL), (dict(nl=0), EINVAL), (dict(nl=5), EINVAL),
    (dict(B=0, layers=None, h=None, r=None, ws=None, ws_bytes=0), OK), (dict(B=0, nl=5), EINVAL),
    (dict(layers=None), EINVAL), (dict(h=None), EINVAL), (dict(r=None), EINVAL),
    (dict(B=I31), ERANGE), (dict(N=I31), ERANGE),
    (dict(ws=None), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE),
    (dict(layers=_layers(ent=None)), EINVAL), (dict(layers=_layers(rel=None)), EINVAL), (dict(layers=_layers(table=None)), EINVAL),
    (dict(layers=_layers(2, table=None), nl=2), EINVAL),
    # precedence: a null layer field is found after the workspace check, a null argument before the range check
    (dict(layers=_layers(ent=None), ws_bytes=0), EWORKSPACE), (dict(layers=_layers(ent=None), B=I31), ERANGE),
    (dict(h=None, B=I31), EINVAL), (dict(B=I31, ws=None), ERANGE),
]
BAD_INDEX = [dict(n_keys=-1), dict(n_keys=I31), dict(key=None), dict(tail_ptr=None), dict(tail_idx=None)]


@pytest.mark.parametrize("name", ["jmac_linkpred_topk_f32", "jmac_linkpred_topk_bf16"])
def test_linkpred_topk_return_codes(name):
    rows = LINK_SHARED + [
        (dict(k=0), EINVAL), (dict(k=65), EINVAL), (dict(N=5, k=6), EINVAL), (dict(val=None), EINVAL), (dict(idx=None), EINVAL),
        (dict(d=516), EDIM), (dict(d=516, k=0), EINVAL), (dict(d=516, B=0), EDIM), (dict(d=516, h=None), EDIM),     # d > 512: before B == 0
        (dict(B=2, N=8192, k=10, ws_bytes=34304 - 1), EWORKSPACE),
        (dict(index=_index(), ws_bytes=0), EWORKSPACE),
    ] + [(dict(index=_index(**bad)), EINVAL) for bad in BAD_INDEX] + [(dict(index=_index(key=None), B=I31), EINVAL)]
    for over, want in rows:
        assert _call(name, "link_topk", LINK, **over) == want, over


@pytest.mark.parametrize("ty", ["f32", "bf16"])
def test_linkpred_rank_return_codes(ty):
    rows = LINK_SHARED + [
        (dict(gold=None), EINVAL), (dict(rank=None), EINVAL),
        (dict(d=516), ERANGE), (dict(d=516, h=None), EINVAL), (dict(d=516, ws=None), ERANGE),        # d > 512: a range error here
        (dict(B=3, ws_bytes=_lib.lib().jmac_linkpred_rank_workspace_bytes(3, 8, 1) - 1), EWORKSPACE),
    ]
    for over, want in rows:
        assert _call("jmac_linkpred_rank_" + ty, "link_rank", LINK, **over) == want, over
        assert _call("jmac_linkpred_rank_indexed_" + ty, "link_rank_indexed", LINK, index=_index(), **over) == want, over
    assert _call("jmac_linkpred_rank_" + ty, "link_rank", LINK, filt_ptr=P) == EINVAL              # a CSR pointer without its indices
    assert _call("jmac_linkpred_rank_" + ty, "link_rank", LINK, filt_ptr=P, filt_idx=P, ws_bytes=0) == EWORKSPACE
    for bad in BAD_INDEX:
        assert _call("jmac_linkpred_rank_indexed_" + ty, "link_rank_indexed", LINK, index=_index(**bad)) == EINVAL, bad
    assert _call("jmac_linkpred_rank_indexed_" + ty, "link_rank_indexed", LINK, index=_index(key=None), N=I31) == EINVAL
    assert _call("jmac_linkpred_rank_indexed_" + ty, "link_rank_indexed", LINK, index=None, ws_bytes=0) == EWORKSPACE
