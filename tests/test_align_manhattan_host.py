"""CPU: the Manhattan alignment metric's definition (tests/align_metric_ref.py, float64) against the reference's own evaluator,
recorded in tests/golden/align_manhattan.npz by tests/golden/gen_align_manhattan.py, and the evaluator's arguments in the harness."""
import os

import numpy as np
import pytest

import align_metric_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = [(False, 0), (False, 10), (True, 0), (True, 10)]


@pytest.mark.parametrize("normalize,csls_k", SETTINGS)
def test_restatement_reproduces_the_reference(normalize, csls_k):
    z = np.load(os.path.join(GOLD, "align_eval.npz"))
    g = np.load(os.path.join(GOLD, "align_manhattan.npz"))
    tag = "n%d_csls%d" % (int(normalize), csls_k)
    c = ref.csls(ref.manhattan_sim(z["e1"], z["e2"], normalize), csls_k)
    hits, mr, mrr = ref.summary(ref.ranks(c, np.arange(c.shape[0])))
    assert np.allclose(hits, g["hits_" + tag], atol=1e-9)
    assert abs(mr - float(g["mr_" + tag])) < 1e-9 and abs(mrr - float(g["mrr_" + tag])) < 1e-9
    # csls_k = 10: the reference's np.partition-based neighbourhood mean may swap the k-th for the (k+1)-th neighbour
    # (the allowance tests/test_oracle_golden.py gives the cosine fixture)
    err = float(np.abs(c - g["sim_" + tag]).max())
    print(tag, "max |float64 - reference fp32| = %.3g" % err)
    assert err < (1e-5 if csls_k == 0 else 2e-2)


def test_restatement_ties_go_to_the_lower_index():
    c = np.array([[1.0, 1.0, 0.5, 1.0], [0.0, 2.0, 2.0, -1.0]])
    assert ref.ranks(c, [3, 2]).tolist() == [3, 2] and ref.ranks(c, [0, 1]).tolist() == [1, 1]


def test_make_args_carries_the_evaluator_defaults():
    from jmac_amd import harness
    args = harness.make_args()
    assert args.eval_metric == "cosine" and args.eval_norm is False          # train.py:95-96
    assert harness.make_args(eval_metric="manhattan", eval_norm=True).eval_metric == "manhattan"


def test_l1_csls_entry_points_validate_before_any_device_work():
    import ctypes
    from jmac_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    EINVAL, EDIM, EWORKSPACE = -1, -2, -3
    topk = lambda lda, k, r1, r2, ws, wsb: L.jmac_l1_csls_topk_f32(p, lda, p, 8, 4, 100, 8, r1, r2, k, p, p, ws, wsb, None)       # noqa: E731
    assert topk(8, 0, None, None, p, 1 << 20) == EINVAL and topk(8, 65, None, None, p, 1 << 20) == EINVAL
    assert topk(8, 101, None, None, p, 1 << 20) == EINVAL                   # k > N (and > 64)
    assert topk(8, 5, p, None, p, 1 << 20) == EINVAL                        # r1 without r2
    assert topk(6, 5, None, None, p, 1 << 20) == EDIM
    assert topk(8, 5, None, None, None, 0) == EWORKSPACE and topk(8, 5, None, None, p, 16) == EWORKSPACE
    assert L.jmac_l1_csls_topk_viable_f32(p, 8, p, 8, 4, 100, 8, None, None, None, p, 5, p, p, p, 1 << 20, None) == EINVAL   # no row_id
    assert L.jmac_l1_csls_topk_viable_f32(p, 8, p, 6, 4, 100, 8, None, None, p, p, 5, p, p, p, 1 << 20, None) == EDIM
    assert L.jmac_l1_csls_rank_f32(p, 8, p, 8, 4, 100, 8, None, None, None, p, p, 1 << 20, None) == EINVAL                   # no gold
    assert L.jmac_l1_csls_rank_f32(p, 6, p, 8, 4, 100, 8, None, None, p, p, p, 1 << 20, None) == EDIM
    assert L.jmac_l1_csls_rank_f32(p, 8, p, 8, 4, 100, 8, None, None, p, p, None, 0, None) == EWORKSPACE
    assert L.jmac_l1_csls_topk_workspace_bytes(4, 100, 8, 5) == L.jmac_sim_csls_topk_workspace_bytes(4, 100, 5) >= 4 * 100 * 4
    assert L.jmac_l1_csls_rank_workspace_bytes(4, 100) >= 16
    assert L.jmac_l1_csls_topk_f32(p, 8, p, 8, 0, 100, 8, None, None, 5, p, p, None, 0, None) == 0                           # no rows: nothing to do
