"""CPU: the attention export's definition against the reference, and its entry points' argument checks.

1. tests/attention_ref.py -- the float64 restatement the GPU tests hold the kernels to -- applied to the reference layer's
   parameters in factorised form reproduces what the reference's own scatter_softmax returned (tests/golden/attention.npz,
   written by tests/golden/gen_attention.py).
2. jmac_rel_attn_edge_weights_* validate their arguments before any device call."""
import ctypes

import numpy as np
import pytest

from attention_ref import attention_ref, reference_tables
from util import load_golden

CASES = ["tiny", "rand200", "d300", "ja_train", "noedge", "dbpv1"]


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_golden("layer_" + case)
    gold = load_golden("attention")
    params = {k[len("param."):]: v for k, v in g.items() if k.startswith("param.")}
    P, Q, Rq, a = reference_tables(params, g["X"], g["R"], float(g["slope"]), "relu" if case == "dbpv1" else "leaky_relu")
    ei, et = g["edge_index"], g["edge_type"]
    ref = attention_ref(P, Q, Rq, a, ei[0], ei[1], et, float(g["slope"]), int(g["n"]))
    for got, key in ((ref.alpha, "alpha_" + case), (ref.alpha_scaled, "alpha_scaled_" + case)):
        want = gold[key].astype(np.float64)
        assert got.shape == want.shape == (ei.shape[1],)
        if want.size == 0:
            continue
        assert want.min() > 0
        err = float(np.max(np.abs(got - want) / want))               # per edge, relative to that edge's weight
        print("%s: max relative error %.2e" % (key, err))
        assert err <= 1e-5, (key, err)
    if case == "noedge":
        assert ref.entropy.tolist() == [0.0] * int(g["n"]) and ref.argmax.tolist() == [-1] * int(g["n"])


def test_restatement_ties_entropy_and_argmax():
    """Hand-checkable: two identical edges and a third on destination 0, one edge on destination 2, destination 1 empty."""
    P = np.zeros((3, 4))
    Q = np.array([[1.0, 0, 0, 0], [0, 0, 0, 0], [0, -2.0, 0, 0]])
    Rq = np.zeros((1, 4))
    a = np.array([1.0, 1.0, 0, 0])
    dst, src, typ = [0, 2, 0, 0], [0, 1, 0, 2], [0, 0, 0, 0]        # logits: 1, 0, 1, -2 * 0.5
    r = attention_ref(P, Q, Rq, a, dst, src, typ, 0.5, 3)
    e = np.exp([0.0, 0.0, -2.0])
    np.testing.assert_allclose(r.logit, [1.0, 0.0, 1.0, -1.0])
    np.testing.assert_allclose(r.alpha, [e[0] / e.sum(), 1.0, e[1] / e.sum(), e[2] / e.sum()])
    assert r.alpha[0] == r.alpha[2] and r.alpha[1] == 1.0
    np.testing.assert_allclose(r.alpha_scaled, r.alpha * np.sqrt([3, 1, 3, 3]))
    assert r.argmax.tolist() == [0, -1, 1]                            # the tie on destination 0 goes to the lower edge id
    p = e / e.sum()
    np.testing.assert_allclose(r.entropy, [-(p * np.log(p)).sum(), 0.0, 0.0], atol=1e-15)
    np.testing.assert_allclose(r.A, [1.0, 0.0, 1.0, 1.0])


def test_edge_weight_entry_points_validate_without_a_device():
    from jmac_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                                          # never dereferenced: every call returns before a launch
    view = _lib.View(256, None, 256, 256, 256, 4, 0, 0, None, 0, 0, None)
    v = ctypes.pointer(view)
    need = L.jmac_rel_attn_edge_weights_workspace_bytes(5, 7)
    assert need >= 7 * 4
    assert L.jmac_rel_attn_edge_weights_workspace_bytes(5, 0) <= 512

    def f32(P=p, ldp=8, QZ=p, ldqz=16, RR=p, ldrr=16, a=p, col=p, et=p, by_dst=v, N=5, E=7, d=8, alpha=p, ws=p, ws_bytes=need):
        return L.jmac_rel_attn_edge_weights_f32(P, ldp, QZ, ldqz, RR, ldrr, a, col, et, None, by_dst, N, E, d, 0.05, 0, alpha, None,
                                                None, None, ws, ws_bytes, None)

    def bf16(dh=8, d=8, ldp=8, N=5, P=p, ws_bytes=need):
        return L.jmac_rel_attn_edge_weights_bf16(P, ldp, p, 16, p, 16, dh, p, p, p, None, v, N, 7, d, 0.05, 0, p, None, None, None, p,
                                                 ws_bytes, None)

    for bad in (dict(P=None), dict(QZ=None), dict(RR=None), dict(a=None), dict(col=None), dict(et=None), dict(by_dst=None),
                dict(alpha=None), dict(N=-1), dict(E=-1)):
        assert f32(**bad) == -1, bad                                  # JMAC_EINVAL
    assert bf16(P=None) == -1 and bf16(N=-2) == -1
    for bad in (dict(d=6), dict(d=516), dict(d=0), dict(ldp=6), dict(ldqz=18), dict(ldrr=4)):
        assert f32(**bad) == -2, bad                                  # JMAC_EDIM
    assert bf16(d=10) == -2 and bf16(d=520, dh=520, ldp=520) == -2 and bf16(dh=4) == -2 and bf16(dh=16, ldp=8) == -2
    assert f32(P=None, d=6) == -1                                     # the null pointer is reported ahead of the dimension
    assert f32(ws_bytes=need - 1) == -3 and f32(ws=None) == -3        # JMAC_EWORKSPACE
    assert bf16(ws_bytes=7) == -3
    assert f32(d=6, ws_bytes=0) == -2                                 # ... and the dimension ahead of the workspace
    assert f32(N=2 ** 31, ws_bytes=0) == -4                           # JMAC_ERANGE ahead of the workspace
