"""Host side of the matrix-free EnTr refresh (no GPU): argument validation and workspace size of
jmac_sim_softmax_stats_f32, and the closed form the GPU tests take their expected values from (tests/align_stats_ref.py)
against the reference's golden matrices and the float64 oracle."""
import ctypes

import numpy as np
import torch

import align_stats_ref as ref
from util import assert_close, load_golden


def _call(L, n1=8, n2=8, d=8, lda=8, ldb=8, outs=1, ws_bytes=None, scale=20.0):
    fake = ctypes.c_void_p(4096)                      # never dereferenced: every case returns before a launch
    need = int(L.jmac_sim_softmax_stats_workspace_bytes(max(n1, 0), max(n2, 0)))
    o = [fake if outs else None] + [None] * 7
    return L.jmac_sim_softmax_stats_f32(fake, lda, fake, ldb, n1, n2, d, scale, *o, fake, need if ws_bytes is None else ws_bytes, None)


def test_stats_entry_validates_before_touching_a_device():
    from jmac_amd._lib import lib
    L = lib()
    assert _call(L, n1=-1) == -1 and _call(L, n2=-1) == -1 and _call(L, d=0) == -1
    assert _call(L, outs=0) == -1                     # every output NULL
    assert _call(L, scale=0.0) == -1
    assert _call(L, lda=3) == -2 and _call(L, ldb=6) == -2
    assert _call(L, ws_bytes=16) == -3
    assert _call(L, n1=0) == 0 and _call(L, n2=0) == 0


def test_stats_workspace_is_linear_not_quadratic():
    from jmac_amd._lib import lib
    ws = lib().jmac_sim_softmax_stats_workspace_bytes
    assert 0 < ws(30000, 30000) <= 30000 * 30000 * 4 // 4          # a quarter of ONE matrix (the stored path holds three)
    for n2 in (1112, 30000):
        for n1 in (100, 5000, 30000):
            assert ws(4 * n1, n2) <= 4 * ws(n1, n2) and ws(n2, 4 * n1) <= 4 * ws(n2, n1)
    assert ws(10 ** 6, 3000) < 10 ** 6 * 3000 * 4 // 4            # config 4's entity count with 3 000 listed columns: linear in n1


def test_closed_form_reproduces_the_reference_golden():
    g = load_golden("model_small")
    l1, l2 = g["aq_list1"], g["aq_list2"]
    H, rp, ri, cp, ci = ref.alignment_stats(g["emb1_align"], g["emb2_align"], l1, l2)
    assert abs(float(H) - float(g["aq_entropy"])) <= 1e-4 * float(g["aq_entropy"])
    P, Q = torch.from_numpy(g["aq_softmax_rows"]), torch.from_numpy(g["aq_softmax_cols"])
    assert_close(rp, P.max(1)[0], 1e-4, what="row maxima")
    assert_close(cp, Q.max(1)[0], 1e-4, what="column maxima")
    assert np.array_equal(ri[l1].numpy(), ref.first_argmax(P, 1)[l1]) and np.array_equal(ci[l2].numpy(), ref.first_argmax(Q, 1)[l2])
    out1 = np.setdiff1d(np.arange(P.shape[0]), l1)
    assert (ri[out1] == 0).all() and torch.allclose(rp[out1], torch.tensor(1.0 / P.shape[1], dtype=torch.float64))
    assert_close(rp[out1], P[out1].max(1)[0], 1e-4, what="masked rows")


def test_closed_form_against_oracle_with_repeats_and_antipodal_row():
    import oracle.jmac_oracle as orc
    e1, e2, l1, l2, (ia, ib, jc) = ref.seeded_case()
    H, P, Q = orc.alignment_quality(e1.double(), e2.double(), l1, l2)
    h, rp, ri, cp, ci = ref.alignment_stats(e1, e2, l1, l2)
    assert abs(float(h) - float(H)) <= 1e-9 * abs(float(H))
    assert_close(rp, P.max(1)[0], 1e-4, what="row maxima")
    assert_close(cp, Q.max(1)[0], 1e-4, what="column maxima")
    assert np.array_equal(ri.numpy(), ref.first_argmax(P, 1)) and np.array_equal(ci.numpy(), ref.first_argmax(Q, 1))
    # the constructed lines: x == fill -> the lower of (first listed maximum, first masked column); x < fill -> first masked
    assert int(ri[ia]) == 0 and int(ri[ib]) == 2 and int(ci[jc]) == 0
