"""No GPU: the return codes and workspace sizes of jmac_sim_csls_topk_screened_f32 / jmac_sim_csls_topk_viable_screened_f32, and
the ValueErrors of their Python callers.  The checks are the fp32 entries' in their order (sizes and the r1 / r2 pairing > empty
problem > pointers > strides and row length > 2^31 > workspace), with JMAC_EDIM for d % 4 and d > 512 and JMAC_ERANGE for 2^31 rows
or columns both ahead of the workspace check.  No device is touched: every call returns before its first launch."""
import ctypes

import pytest
import torch

OK, EINVAL, EDIM, EWORKSPACE, ERANGE = 0, -1, -2, -3, -4
P, BIG, I31 = ctypes.c_void_p(16), 1 << 40, 2 ** 31 - 1
BASE = dict(A=P, lda=8, B=P, ldb=8, n1=4, n2=100, d=8, r1=P, r2=P, row_id=P, best=P, k=10, val=P, idx=P, nres=P, ws=P, ws_bytes=BIG,
            stream=None)
PLAIN = "A lda B ldb n1 n2 d r1 r2 k val idx nres ws ws_bytes stream".split()
VIABLE = "A lda B ldb n1 n2 d r1 r2 row_id best k val idx nres ws ws_bytes stream".split()
# (overrides, plain form's code, viable form's code)
ROWS = [
    (dict(n1=-1), EINVAL, EINVAL), (dict(n2=0), EINVAL, EINVAL), (dict(d=0), EINVAL, EINVAL), (dict(k=0), EINVAL, EINVAL),
    (dict(n2=5, k=6), EINVAL, EINVAL), (dict(k=65, n2=9000), EINVAL, EINVAL), (dict(r1=None), EINVAL, EINVAL), (dict(r2=None), EINVAL, EINVAL),
    (dict(n1=0, A=None, B=None, idx=None, ws=None, ws_bytes=0), OK, OK), (dict(n1=0, k=0), EINVAL, EINVAL), (dict(n1=0, lda=6), OK, OK),
    (dict(n1=0, d=516), OK, OK),
    (dict(A=None), EINVAL, EINVAL), (dict(B=None), EINVAL, EINVAL), (dict(idx=None), EINVAL, EINVAL), (dict(A=None, ldb=6), EINVAL, EINVAL),
    (dict(A=None, d=516), EINVAL, EINVAL), (dict(val=None, ws_bytes=0), EWORKSPACE, EINVAL), (dict(row_id=None, ws_bytes=0), EWORKSPACE, EINVAL),
    (dict(best=None, ws_bytes=0), EWORKSPACE, EINVAL),
    (dict(lda=6), EDIM, EDIM), (dict(ldb=6), EDIM, EDIM), (dict(lda=6, ws=None), EDIM, EDIM), (dict(d=516), EDIM, EDIM),
    (dict(d=516, ws_bytes=0), EDIM, EDIM), (dict(d=6, ws_bytes=0), EDIM, EDIM), (dict(d=512, ws_bytes=0), EWORKSPACE, EWORKSPACE),
    (dict(n1=I31, ws_bytes=0), ERANGE, ERANGE), (dict(n2=I31, ws_bytes=0), ERANGE, ERANGE), (dict(n1=I31, d=516), EDIM, EDIM),
    (dict(ws=None), EWORKSPACE, EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE, EWORKSPACE), (dict(r1=None, r2=None, ws_bytes=0), EWORKSPACE, EWORKSPACE),
    (dict(nres=None, ws_bytes=0), EWORKSPACE, EWORKSPACE),
]


def test_return_codes_in_the_documented_order():
    from jmac_amd import _lib
    L = _lib.lib()
    for over, plain, viable in ROWS:
        args = dict(BASE, **over)
        assert L.jmac_sim_csls_topk_screened_f32(*[args[f] for f in PLAIN]) == plain, over
        assert L.jmac_sim_csls_topk_viable_screened_f32(*[args[f] for f in VIABLE]) == viable, over


def test_the_fp32_entries_agree_where_they_share_a_check():
    """every row whose code does not come from the screen's own two checks (d > 512; the position of 2^31) is the fp32 entry's"""
    from jmac_amd import _lib
    L = _lib.lib()
    f_plain = [f for f in PLAIN if f != "nres"]
    f_viable = [f for f in VIABLE if f != "nres"]
    for over, plain, viable in ROWS:
        if over.get("d") == 516 or "nres" in over:
            continue
        args = dict(BASE, **over)
        assert L.jmac_sim_csls_topk_f32(*[args[f] for f in f_plain]) == plain, over
        assert L.jmac_sim_csls_topk_viable_f32(*[args[f] for f in f_viable]) == viable, over


def test_workspace_sizes():
    from jmac_amd import _lib
    L = _lib.lib()
    wsb = L.jmac_sim_csls_topk_screened_workspace_bytes
    # unscreened shapes: exactly the fp32 entry's workspace
    assert wsb(100, 4000, 16, 10) == L.jmac_sim_csls_topk_workspace_bytes(100, 4000, 10)
    assert wsb(8300, 300, 32, 4) == L.jmac_sim_csls_topk_workspace_bytes(8300, 300, 4)
    assert wsb(-1, 100, 8, 1) == 0 and wsb(4, 100, 0, 1) == 0 and wsb(4, 100, 8, 0) == 0
    # screened: bf16 copies + norms + the sample (max(n2 / 8, 2048) columns) + the lists (2048 words per row), never n1 x n2: as a
    # share of the matrix max(1/8, 2048 / n2) + 2048 / n2 + (n1 + n2) d / (2 n1 n2), under 0.3 for tables of 16384 columns and more
    for n1, n2, d, k in ((3000, 30000, 300, 16), (13996, 20000, 256, 64)):
        need = wsb(n1, n2, d, k)
        assert 0 < need < 0.3 * n1 * n2 * 4
        assert need == L.jmac_sim_topk_screened_workspace_bytes(n1, n2, d, k)
        short = dict(BASE, n1=n1, n2=n2, d=d, lda=d, ldb=d, k=k, ws_bytes=need - 1)
        assert L.jmac_sim_csls_topk_screened_f32(*[short[f] for f in PLAIN]) == EWORKSPACE
        assert L.jmac_sim_csls_topk_viable_screened_f32(*[short[f] for f in VIABLE]) == EWORKSPACE
    # a narrow shape one byte short of the fp32 entry's workspace
    short = dict(BASE, n2=4000, ws_bytes=wsb(4, 4000, 8, 10) - 1)
    assert L.jmac_sim_csls_topk_screened_f32(*[short[f] for f in PLAIN]) == EWORKSPACE
    assert L.jmac_sim_csls_topk_viable_screened_f32(*[short[f] for f in VIABLE]) == EWORKSPACE


def test_python_value_errors():
    from jmac_amd import scoring
    x = torch.zeros(4, 8)
    best = torch.zeros(4, dtype=torch.int64)
    for bad in ("fp16", True, 1):
        with pytest.raises(ValueError, match="screen must be None or 'bf16'"):
            scoring.alignment_topk(x, x, 2, screen=bad)
        with pytest.raises(ValueError, match="screen must be None or 'bf16'"):
            scoring.alignment_topk_viable(x, x, 2, best, screen=bad)
        with pytest.raises(ValueError, match="screen must be None or 'bf16'"):
            scoring.stable_alignment(x, x, 2, screen=bad)
        with pytest.raises(ValueError, match="screen must be None or 'bf16'"):
            scoring.auction_alignment(x, x, 2, screen=bad)
        with pytest.raises(ValueError, match="screen must be None or 'bf16'"):
            scoring.csls_terms(x, x, 2, screen=bad)
    for fn, extra in ((scoring.alignment_topk, ()), (scoring.alignment_topk_viable, (best,)), (scoring.stable_alignment, ()),
                      (scoring.auction_alignment, ())):
        with pytest.raises(ValueError, match="manhattan"):
            fn(x, x, 2, *extra, metric="manhattan", screen="bf16")
    with pytest.raises(ValueError, match="manhattan"):
        scoring.csls_terms(x, x, 2, metric="manhattan", screen="bf16")
    with pytest.raises(ValueError, match="return_stats needs screen"):
        scoring.alignment_topk(x, x, 2, return_stats=True)
