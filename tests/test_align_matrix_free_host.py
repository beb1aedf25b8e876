"""No device: the matrix-free alignment entry points are declared, exported and typed (test_abi.py checks that for every symbol of
the header), validate their arguments before the device is touched, and keep the workspace promises of the header."""
import ctypes

import pytest

from jmac_amd import _lib

OK, EINVAL, EDIM, EWORKSPACE = 0, -1, -2, -3
P = ctypes.c_void_p(256)                       # a non-NULL pointer no entry point may dereference on these paths


def test_symbols_are_declared_and_bound():
    names = ["jmac_sim_csls_rank_workspace_bytes", "jmac_sim_csls_rank_f32", "jmac_sim_csls_topk_workspace_bytes", "jmac_sim_csls_topk_f32"]
    assert set(names) <= set(_lib.header_symbols())
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib._SIGS[n][1]


def test_rank_validation_needs_no_device():
    f = _lib.lib().jmac_sim_csls_rank_f32
    ws = _lib.lib().jmac_sim_csls_rank_workspace_bytes(5, 7)
    assert f(None, 4, None, 4, 0, 7, 4, None, None, None, None, None, 0, None) == OK              # n1 == 0
    assert f(P, 4, P, 4, -1, 7, 4, None, None, P, P, P, ws, None) == EINVAL
    assert f(P, 4, P, 4, 5, 0, 4, None, None, P, P, P, ws, None) == EINVAL
    assert f(None, 4, P, 4, 5, 7, 4, None, None, P, P, P, ws, None) == EINVAL                      # NULL operands
    assert f(P, 4, None, 4, 5, 7, 4, None, None, P, P, P, ws, None) == EINVAL
    assert f(P, 4, P, 4, 5, 7, 4, None, None, None, P, P, ws, None) == EINVAL                      # NULL gold
    assert f(P, 4, P, 4, 5, 7, 4, None, None, P, None, P, ws, None) == EINVAL                      # NULL rank
    assert f(P, 4, P, 4, 5, 7, 4, P, None, P, P, P, ws, None) == EINVAL                            # r1 without r2
    assert f(P, 4, P, 4, 5, 7, 4, None, P, P, P, P, ws, None) == EINVAL                            # r2 without r1
    assert f(P, 6, P, 4, 5, 7, 4, P, P, P, P, P, ws, None) == EDIM                                 # lda % 4
    assert f(P, 4, P, 6, 5, 7, 4, P, P, P, P, P, ws, None) == EDIM                                 # ldb % 4
    assert f(P, 4, P, 4, 5, 7, 4, P, P, P, P, P, ws - 1, None) == EWORKSPACE
    assert f(P, 4, P, 4, 5, 7, 4, P, P, P, P, None, ws, None) == EWORKSPACE


def test_topk_validation_needs_no_device():
    L = _lib.lib()
    f = L.jmac_sim_csls_topk_f32
    ws = L.jmac_sim_csls_topk_workspace_bytes(5, 70, 3)
    assert f(None, 4, None, 4, 0, 70, 4, None, None, 3, None, None, None, 0, None) == OK           # n1 == 0
    assert f(P, 4, P, 4, 5, 70, 4, P, P, 0, None, P, P, ws, None) == EINVAL                        # k out of range
    assert f(P, 4, P, 4, 5, 70, 4, P, P, 65, None, P, P, 1 << 30, None) == EINVAL
    assert f(P, 4, P, 4, 5, 7, 4, P, P, 8, None, P, P, 1 << 30, None) == EINVAL                    # k > n2
    assert f(None, 4, P, 4, 5, 70, 4, P, P, 3, None, P, P, ws, None) == EINVAL
    assert f(P, 4, None, 4, 5, 70, 4, P, P, 3, None, P, P, ws, None) == EINVAL
    assert f(P, 4, P, 4, 5, 70, 4, P, P, 3, None, None, P, ws, None) == EINVAL                     # NULL idx (val may be NULL)
    assert f(P, 4, P, 4, 5, 70, 4, P, None, 3, None, P, P, ws, None) == EINVAL
    assert f(P, 4, P, 4, 5, 70, 4, None, P, 3, None, P, P, ws, None) == EINVAL
    assert f(P, 6, P, 4, 5, 70, 4, P, P, 3, None, P, P, ws, None) == EDIM
    assert f(P, 4, P, 6, 5, 70, 4, P, P, 3, None, P, P, ws, None) == EDIM
    assert f(P, 4, P, 4, 5, 70, 4, P, P, 3, None, P, P, ws - 1, None) == EWORKSPACE
    assert f(P, 4, P, 4, 5, 70, 4, P, P, 3, None, P, None, ws, None) == EWORKSPACE
    assert f(P, 4, P, 4, 5, 70, 4, None, None, 3, None, P, P, ws - 1, None) == EWORKSPACE          # the plain form validates the same way


@pytest.mark.parametrize("n1", [1, 300, 30000])
def test_rank_workspace_does_not_grow_with_the_columns(n1):
    f = _lib.lib().jmac_sim_csls_rank_workspace_bytes
    assert f(n1, 8192) == f(n1, 10 ** 6) == f(n1, 1)
    assert 4 * n1 <= f(n1, 8192) <= 4 * n1 + 1024                                                  # O(n1): one float per row


def test_topk_workspace_bounds():
    L = _lib.lib()
    mine = L.jmac_sim_csls_topk_workspace_bytes(30000, 30000, 10)
    assert 0 < mine <= 1.25 * L.jmac_sim_topk_workspace_bytes(30000, 30000, 10)
    assert mine <= 0.25 * 30000 ** 2 * 4
