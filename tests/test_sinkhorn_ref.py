"""Host side of the Sinkhorn alignment (no GPU): the float64 recursion the GPU tests take their expected values from
(tests/sinkhorn_ref.py) has the properties it is used for, the C ABI carries the new entry point, and jmac_sim_lse_f32 validates
its arguments before it touches a device."""
import ctypes
import functools

import torch

import sinkhorn_ref as ref

SCALE = 50.0


@functools.lru_cache(maxsize=None)
def hub(n1, n2, d, iters):
    e1, e2, gold = ref.hub_pair(n1, n2, d)
    return (e1, e2, gold) + ref.potentials(e1, e2, SCALE, iters)


def test_column_marginals_hold_and_the_row_residual_falls():
    for shape in ((300, 515, 48), (2000, 2000, 64)):
        e1, e2, _, f, g, res = hub(*shape, 10)
        P = torch.exp(ref.log_plan(e1, e2, SCALE, f, g))
        assert float((P.sum(0) - 1.0 / shape[1]).abs().max()) <= 1e-12
        assert abs(float(P.sum()) - 1.0) <= 1e-12
        print("row residuals:", ["%.3g" % r for r in res])
        assert all(x > y for x, y in zip(res, res[1:]))


def test_log_plan_is_the_rescored_similarity():
    e1, e2, _, f, g, _ = hub(300, 515, 48, 10)
    c = ref.rescored(e1, e2, *ref.terms(f, g, SCALE))
    assert float((c - (2.0 / SCALE) * ref.log_plan(e1, e2, SCALE, f, g)).abs().max()) <= 1e-12


def test_sinkhorn_beats_csls_on_the_hub_pair():
    import oracle.jmac_oracle as orc
    e1, e2, gold, f, g, _ = hub(2000, 2000, 64, 10)
    S = e1.double() @ e2.double().t()
    hits = [float((m.argmax(1) == gold).double().mean())
            for m in (S, orc.csls_sim(S, 10), ref.rescored(e1, e2, *ref.terms(f, g, SCALE)))]
    print("Hits@1: cosine %.4f, CSLS-10 %.4f, Sinkhorn %.4f" % tuple(hits))
    assert hits[2] > hits[1] > hits[0]


def test_fp32_recursion_stays_close():
    """The yardstick of the GPU test: the fp32 evaluation's error does not grow with the iterations (the map is non-expansive)."""
    e1, e2, _, f, g, _ = hub(300, 515, 48, 30)
    f32, g32 = ref.potentials_fp32(e1, e2, SCALE, 30)
    err = max(float((f32 - f).abs().max()), float((g32 - g).abs().max()))
    print("fp32 error after 30 iterations: %.3g" % err)
    assert err <= 1e-4


def test_abi_carries_the_entry_point():
    from jmac_amd import _lib
    assert "jmac_sim_lse_f32" in _lib._SIGS and "jmac_sim_lse_workspace_bytes" in _lib._SIGS
    assert set(("jmac_sim_lse_f32", "jmac_sim_lse_workspace_bytes")) <= set(_lib.header_symbols())
    assert _lib.lib().jmac_version() >= 132


def _call(L, n1=8, n2=8, d=8, lda=8, ldb=8, rows=1, cols=1, ws_bytes=None, scale=50.0):
    fake = ctypes.c_void_p(4096)                      # never dereferenced: every case returns before a launch
    need = int(L.jmac_sim_lse_workspace_bytes(max(n1, 0), max(n2, 0)))
    return L.jmac_sim_lse_f32(fake, lda, fake, ldb, n1, n2, d, scale, None, None, 0.0, 0.0, fake if rows else None,
                              fake if cols else None, fake, need if ws_bytes is None else ws_bytes, None)


def test_lse_entry_validates_before_touching_a_device():
    from jmac_amd._lib import lib
    L = lib()
    assert _call(L, n1=-1) == -1 and _call(L, n2=-1) == -1 and _call(L, d=0) == -1
    assert _call(L, rows=0, cols=0) == -1             # both outputs NULL
    assert _call(L, scale=0.0) == -1 and _call(L, scale=float("nan")) == -1
    assert _call(L, d=6) == -2 and _call(L, lda=6) == -2 and _call(L, ldb=10) == -2
    assert _call(L, ws_bytes=16) == -3 and _call(L, rows=0, ws_bytes=16) == -3
    assert _call(L, n1=0) == 0 and _call(L, n2=0) == 0


def test_lse_workspace_is_linear_not_quadratic():
    from jmac_amd._lib import lib
    ws = lib().jmac_sim_lse_workspace_bytes
    for n1, n2 in ((11805, 13996), (30000, 30000), (100, 10 ** 6)):
        parts = ((n2 + 63) // 64) * n1 + ((n1 + 63) // 64) * n2
        assert parts * 8 <= ws(n1, n2) <= parts * 8 + 1024
    assert ws(30000, 30000) <= 30000 * 30000 * 4 // 15
