"""CPU: the return code of every argument check of jmac_sim_csls_rank_screened_f32, and their precedence: jmac_sim_csls_rank_f32's
checks in its order, with the screen's row-length limit (d <= 512) next to d % 4 and both ahead of the range and workspace checks.

Validation touches no device.  The pointers are fakes that are never dereferenced: every row ends in a JMAC_E* code or in the
empty-problem JMAC_OK, none passes validation and reaches a launch (the manner of test_topk_return_codes.py)."""
import ctypes

import pytest

from jmac_amd import _lib

OK, EINVAL, EDIM, EWORKSPACE, ERANGE = 0, -1, -2, -3, -4
P = ctypes.c_void_p(16)
BIG, I31 = 1 << 40, 2 ** 31 - 1

BASE = dict(A=P, lda=8, B=P, ldb=8, L=4, N=100, d=8, r1=None, r2=None, gold=P, rank=P, n_rescored=P, finish=1, ws=P, ws_bytes=BIG, stream=None)
SCREENED = "A lda B ldb L N d r1 r2 gold rank n_rescored finish ws ws_bytes stream"
FP32 = "A lda B ldb L N d r1 r2 gold rank ws ws_bytes stream"


def _call(name, order, **over):
    args = dict(BASE, **over)
    return getattr(_lib.lib(), name)(*[args[f] for f in order.split()])


# the checks the two rank entries share, in the fp32 entry's order
SHARED = [
    (dict(L=-1), EINVAL), (dict(N=0), EINVAL), (dict(d=0), EINVAL),
    (dict(r1=P), EINVAL), (dict(r2=P), EINVAL),                                   # one of r1 / r2
    (dict(L=0, A=None, B=None, gold=None, rank=None, ws=None, ws_bytes=0), OK),
    (dict(A=None), EINVAL), (dict(B=None), EINVAL), (dict(gold=None), EINVAL), (dict(rank=None), EINVAL),
    (dict(lda=6), EDIM), (dict(ldb=6), EDIM), (dict(d=6), EDIM),
    (dict(L=I31), ERANGE), (dict(N=I31), ERANGE),
    (dict(ws=None), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE),
    # precedence: EINVAL (sizes) > empty OK > EINVAL (pointers) > EDIM > ERANGE > EWORKSPACE
    (dict(L=0, d=0), EINVAL), (dict(L=0, lda=6), OK), (dict(d=-4, lda=6), EINVAL), (dict(A=None, lda=6), EINVAL),
    (dict(lda=6, L=I31), EDIM), (dict(L=I31, ws_bytes=0), ERANGE), (dict(ldb=2, ws=None), EDIM), (dict(d=6, ws_bytes=0), EDIM),
    (dict(L=I31, N=I31, ws=None), ERANGE),
]


@pytest.mark.parametrize("finish", [0, 1])
def test_shared_checks_agree_with_the_fp32_entry(finish):
    for over, want in SHARED:
        assert _call("jmac_sim_csls_rank_screened_f32", SCREENED, finish=finish, **over) == want, over
        assert _call("jmac_sim_csls_rank_f32", FP32, **over) == want, over


def test_the_screens_own_checks():
    f = lambda **over: _call("jmac_sim_csls_rank_screened_f32", SCREENED, **over)      # noqa: E731
    # d > 512: JMAC_EDIM, after the pointers, ahead of the range and workspace checks; the empty problem stays OK
    assert f(d=516) == EDIM and f(d=512, ws_bytes=0) == EWORKSPACE
    assert f(d=516, N=9000) == EDIM and f(d=516, ws_bytes=0) == EDIM and f(d=516, L=I31) == EDIM
    assert f(d=516, A=None) == EINVAL and f(d=516, L=0) == OK and f(d=516, r1=P) == EINVAL
    # n_rescored is optional: a call without it gets as far as the workspace check
    assert f(n_rescored=None, ws_bytes=0) == EWORKSPACE and f(n_rescored=None, N=9000, ws_bytes=0) == EWORKSPACE


def test_workspace_bytes():
    L = _lib.lib()
    scr, fp32 = L.jmac_sim_csls_rank_screened_workspace_bytes, L.jmac_sim_csls_rank_workspace_bytes
    assert scr(-1, 100, 8) == 0 and scr(4, -1, 8) == 0 and scr(4, 100, 0) == 0
    # a narrow table runs the fp32 entry's code in that entry's workspace
    assert scr(4, 8191, 8) == fp32(4, 8191) and scr(0, 8191, 300) == fp32(0, 8191)
    # a screened one: the bf16 copies (rows padded to 32 k), norms, gold values, counts and 512 list entries per row
    need = scr(130, 9000, 300)
    assert need >= max(fp32(130, 9000), (130 + 9000) * 320 * 2 + (3 * 130 + 9000) * 4 + 130 * 512 * 4)
    assert need < 1.02 * ((130 + 9000) * 320 * 2 + (3 * 130 + 9000) * 4 + 130 * 512 * 4) + 4096
    f = lambda **over: _call("jmac_sim_csls_rank_screened_f32", SCREENED, **over)      # noqa: E731
    assert f(L=130, N=9000, d=300, lda=300, ldb=300, ws_bytes=need - 1) == EWORKSPACE
    assert f(L=3, N=8191, ws_bytes=fp32(3, 8191) - 1) == EWORKSPACE
