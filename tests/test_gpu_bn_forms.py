"""GPU: the plain, segmented and phased forms of BatchNorm + tanh (jmac_amd/csrc/norm.hip) against each other and against float64
torch, through the C ABI itself -- the Python wrappers never take the segmented path with one block, so blk_ptr = [0, N] is
passed here.

Shapes: the smallest that reach every path of the column-sum body (kBlock = 256 threads, D4 = d / 4 column quads, rpb =
kBlock / D4 row slots per workgroup, at most kStatBlocks = 512 workgroups):

    d = 4      D4 = 1, rpb = 256      LDS fold
    d = 300    D4 = 75, rpb = 3       LDS fold, threads 225-255 idle
    d = 1024   D4 = 256 = kBlock      direct store
    d = 1028   D4 = 257               second column pass

each with N = 1, 2 and rpb * 512 + 5 (the statistics grid is capped and the slots wrap).  Every case uses y2 and gy2, both
strided into a [N, 2d] buffer, and non-trivial weight, bias and running estimates.

(a) one-block segmented call against the plain call, same inputs, training mode.  Bit-equal: y, y2, save_mean, save_invstd, and
    gbias / gweight up to 128 partial rows (beyond that the plain reduction's four accumulators per lane and the segmented one's
    two associate differently: 1e-4 relative, 1e-6 absolute, the tolerances of test_segmented_bn_kernels_against_torch).
    NOT bit-equal, though one would expect it from the source (profiles/bn_one_body.txt):
      * running_mean / running_var: r <- (1-m) r + m b rounds both products in the plain form and fuses the first in the
        segmented form.  Bound used here: two roundings of at most half an ulp of a term, the terms at most twice the largest
        result -> 2^-22 relative to the largest result.
      * gx: the segmented apply fuses gz = g (1 - y^2) into gz - invn (...), the plain apply rounds gz first (so that a one-row
        batch gets an exact zero; the segmented form gets the rounding residue of gz there).  One rounding of gz, half an ulp,
        scaled by weight * invstd -> 2^-24 max|weight invstd| max|gz| up to 128 partial rows, where it stands in for the
        equality; beyond that the tolerance above alone.
(b) phased backward (sums, then apply with n_total = N) against the whole backward without gy2: gx and [gbias | gweight]
    bit-equal (the same kernels, the same reduction).
(c) plain forward and backward against float64 torch BatchNorm1d + tanh, d = 300 and 1028, N > 1, training and eval mode."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from util import assert_close

DEV = "cuda"
K_BLOCK, K_STAT_BLOCKS = 256, 512
MOMENTUM, EPS = 0.1, 1e-5


def _rpb(d):
    return max(K_BLOCK // (d // 4), 1)


def _partial_rows(N, d):
    return min((N + _rpb(d) - 1) // _rpb(d), K_STAT_BLOCKS)


WIDTHS = (4, 300, 1024, 1028)
CASES = [(d, N) for d in WIDTHS for N in (1, 2, _rpb(d) * K_STAT_BLOCKS + 5)]
CASE_IDS = ["d%d-N%d" % c for c in CASES]
REF_CASES = [(d, N) for d, N in CASES if d in (300, 1028) and N > 1]
REF_IDS = ["d%d-N%d" % c for c in REF_CASES]


def _L():
    from jmac_amd import _lib
    return _lib


def _ws(nbytes):
    return _L().workspace(nbytes, DEV)


def _fwd_plain(x, w, b, rm, rv, training):
    """jmac_bn_tanh_fwd2_f32 -> y, y2 (strided into [N, 2d]), save_mean, save_invstd, running_mean, running_var."""
    L, ptr = _L().lib(), _L().ptr
    N, d = x.shape
    y, buf = torch.empty(N, d, device=DEV), torch.zeros(N, 2 * d, device=DEV)
    y2 = buf[:, d:]
    mean, invstd = torch.empty(d, device=DEV), torch.empty(d, device=DEV)
    rm, rv = rm.clone(), rv.clone()
    nb = int(L.jmac_bn_tanh_workspace_bytes(N, d))
    ws = _ws(nb)
    _L().check(L.jmac_bn_tanh_fwd2_f32(ptr(x), x.stride(0), N, d, ptr(w), ptr(b), ptr(rm), ptr(rv), 1 if training else 0, MOMENTUM,
                                       EPS, ptr(y), y.stride(0), ptr(y2), y2.stride(0), ptr(mean), ptr(invstd), ptr(ws), nb,
                                       _L().stream()), "jmac_bn_tanh_fwd2_f32")
    return dict(y=y, y2=y2, mean=mean, invstd=invstd, rm=rm, rv=rv)


def _fwd_seg(x, w, b, rm, rv):
    """jmac_bn_tanh_seg_fwd2_f32 with the one block [0, N]."""
    L, ptr = _L().lib(), _L().ptr
    N, d = x.shape
    y, buf = torch.empty(N, d, device=DEV), torch.zeros(N, 2 * d, device=DEV)
    y2 = buf[:, d:]
    mean, invstd = torch.empty(1, d, device=DEV), torch.empty(1, d, device=DEV)
    rm, rv = rm.clone(), rv.clone()
    nb = int(L.jmac_bn_tanh_seg_workspace_bytes(1, d))
    ws = _ws(nb)
    blk, order = (C.c_int64 * 2)(0, N), (C.c_int32 * 1)(0)
    _L().check(L.jmac_bn_tanh_seg_fwd2_f32(ptr(x), x.stride(0), d, 1, blk, order, ptr(w), ptr(b), ptr(rm), ptr(rv), MOMENTUM, EPS,
                                           ptr(y), y.stride(0), ptr(y2), y2.stride(0), ptr(mean), ptr(invstd), ptr(ws), nb,
                                           _L().stream()), "jmac_bn_tanh_seg_fwd2_f32")
    return dict(y=y, y2=y2, mean=mean[0], invstd=invstd[0], rm=rm, rv=rv)


def _bwd_plain(x, y, gy, gy2, w, mean, invstd, training):
    """jmac_bn_tanh_bwd2_f32 -> gx, [gbias | gweight]."""
    L, ptr = _L().lib(), _L().ptr
    N, d = x.shape
    gx, gbw = torch.empty(N, d, device=DEV), torch.empty(2 * d, device=DEV)
    nb = int(L.jmac_bn_tanh_workspace_bytes(N, d))
    ws = _ws(nb)
    _L().check(L.jmac_bn_tanh_bwd2_f32(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(gy), gy.stride(0), ptr(gy2),
                                       gy2.stride(0) if gy2 is not None else 0, N, d, ptr(w), ptr(mean), ptr(invstd),
                                       1 if training else 0, ptr(gx), d, gbw.data_ptr() + 4 * d, ptr(gbw), ptr(ws), nb,
                                       _L().stream()), "jmac_bn_tanh_bwd2_f32")
    return gx, gbw


def _bwd_seg(x, y, gy, gy2, w, mean, invstd):
    L, ptr = _L().lib(), _L().ptr
    N, d = x.shape
    gx, gbw = torch.empty(N, d, device=DEV), torch.empty(2 * d, device=DEV)
    nb = int(L.jmac_bn_tanh_seg_workspace_bytes(1, d))
    ws = _ws(nb)
    blk = (C.c_int64 * 2)(0, N)
    _L().check(L.jmac_bn_tanh_seg_bwd2_f32(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(gy), gy.stride(0), ptr(gy2), gy2.stride(0),
                                           d, 1, blk, ptr(w), ptr(mean), ptr(invstd), ptr(gx), d, gbw.data_ptr() + 4 * d, ptr(gbw),
                                           ptr(ws), nb, _L().stream()), "jmac_bn_tanh_seg_bwd2_f32")
    return gx, gbw


def _bwd_phased(x, y, gy, w, mean, invstd):
    """jmac_bn_tanh_bwd_sums_f32, then jmac_bn_tanh_bwd_apply_f32 with n_total = N -> gx, sums = [sum gz | sum gz xhat]."""
    L, ptr = _L().lib(), _L().ptr
    N, d = x.shape
    gx, sums = torch.empty(N, d, device=DEV), torch.empty(2 * d, device=DEV)
    nb = int(L.jmac_bn_tanh_workspace_bytes(N, d))
    ws = _ws(nb)
    _L().check(L.jmac_bn_tanh_bwd_sums_f32(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(gy), gy.stride(0), N, d, ptr(mean),
                                           ptr(invstd), ptr(sums), ptr(ws), nb, _L().stream()), "jmac_bn_tanh_bwd_sums_f32")
    _L().check(L.jmac_bn_tanh_bwd_apply_f32(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(gy), gy.stride(0), N, d, ptr(w), ptr(mean),
                                            ptr(invstd), ptr(sums), N, ptr(gx), d, _L().stream()), "jmac_bn_tanh_bwd_apply_f32")
    return gx, sums


@functools.lru_cache(maxsize=None)
def _run(d, N):
    """Inputs and every form's outputs of one case, computed once and shared by the tests (which only read them)."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000 * d + N)

    def rnd(*shape):
        return torch.randn(*shape, device=DEV, generator=gen)

    def uni(lo, hi):
        return torch.rand(d, device=DEV, generator=gen) * (hi - lo) + lo

    x = rnd(N, d) * 0.3 + 0.1
    w, b, rm, rv = uni(0.5, 1.5), uni(-0.3, 0.3), uni(-0.1, 0.1), uni(0.5, 1.5)
    gy, gbuf = rnd(N, d), rnd(N, 2 * d)
    gy2 = gbuf[:, d:]
    r = dict(x=x, w=w, b=b, rm=rm, rv=rv, gy=gy, gy2=gy2)
    r["plain"] = p = _fwd_plain(x, w, b, rm, rv, True)
    r["seg"] = _fwd_seg(x, w, b, rm, rv)
    # both backward forms read the plain forward's y and statistics: the comparison of the backwards does not lean on (a) forward
    r["plain_bwd"] = _bwd_plain(x, p["y"], gy, gy2, w, p["mean"], p["invstd"], True)
    r["seg_bwd"] = _bwd_seg(x, p["y"], gy, gy2, w, p["mean"].view(1, d), p["invstd"].view(1, d))
    r["whole_bwd"] = _bwd_plain(x, p["y"], gy, None, w, p["mean"], p["invstd"], True)
    r["phased_bwd"] = _bwd_phased(x, p["y"], gy, w, p["mean"], p["invstd"])
    torch.cuda.synchronize()
    return r


def _maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item() if a.numel() else 0.0


@pytest.mark.parametrize("d,N", CASES, ids=CASE_IDS)
def test_one_block_segmented_forward_equals_plain(d, N):
    r = _run(d, N)
    p, s = r["plain"], r["seg"]
    for k in ("y", "y2", "mean", "invstd", "rm", "rv"):
        print("fwd d=%d N=%d %-6s max|seg - plain| = %.3e" % (d, N, k, _maxdiff(s[k], p[k])))
    for k in ("y", "y2", "mean", "invstd"):
        assert torch.equal(s[k], p[k]), k
    assert torch.equal(p["y"], p["y2"]) and torch.equal(s["y"], s["y2"])
    for k in ("rm", "rv"):                                      # one product fused in the segmented form only: see (a)
        assert_close(s[k], p[k], 2.0 ** -22, 0.0, "seg vs plain " + k)


@pytest.mark.parametrize("d,N", CASES, ids=CASE_IDS)
def test_one_block_segmented_backward_against_plain(d, N):
    r = _run(d, N)
    (gx_p, gbw_p), (gx_s, gbw_s) = r["plain_bwd"], r["seg_bwd"]
    y = r["plain"]["y"]
    gz = (r["gy"] + r["gy2"]) * (1.0 - y * y)
    fused_gz = 2.0 ** -24 * (r["w"] * r["plain"]["invstd"]).abs().max().item() * gz.abs().max().item()
    rows = _partial_rows(N, d)
    print("bwd d=%d N=%d partial rows %d: max|seg - plain| gx %.3e (max|gx| %.3e, fused-gz bound %.3e)  gbias %.3e  gweight %.3e"
          % (d, N, rows, _maxdiff(gx_s, gx_p), gx_p.abs().max().item(), fused_gz, _maxdiff(gbw_s[:d], gbw_p[:d]),
             _maxdiff(gbw_s[d:], gbw_p[d:])))
    if rows <= 128:                                             # the two reductions add the same terms in the same order
        assert torch.equal(gbw_s, gbw_p)
        assert_close(gx_s, gx_p, 2.0 ** -22, fused_gz, "seg vs plain gx")
    else:
        assert_close(gbw_s[:d], gbw_p[:d], 1e-4, 1e-6, "seg vs plain gbias")
        assert_close(gbw_s[d:], gbw_p[d:], 1e-4, 1e-6, "seg vs plain gweight")
        assert_close(gx_s, gx_p, 1e-4, 1e-6, "seg vs plain gx")


@pytest.mark.parametrize("d,N", CASES, ids=CASE_IDS)
def test_phased_backward_equals_whole_backward(d, N):
    r = _run(d, N)
    (gx_w, gbw_w), (gx_ph, sums) = r["whole_bwd"], r["phased_bwd"]
    print("phased d=%d N=%d: max|phased - whole| gx %.3e  sums %.3e" % (d, N, _maxdiff(gx_ph, gx_w), _maxdiff(sums, gbw_w)))
    assert torch.equal(gx_ph, gx_w)
    assert torch.equal(sums, gbw_w)


def _reference(r, training):
    """float64 torch BatchNorm1d + tanh on the CPU: y, running estimates, gx, grad bias, grad weight."""
    d = r["x"].shape[1]
    bn = torch.nn.BatchNorm1d(d, eps=EPS, momentum=MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(r["w"].cpu().double())
        bn.bias.copy_(r["b"].cpu().double())
        bn.running_mean.copy_(r["rm"].cpu().double())
        bn.running_var.copy_(r["rv"].cpu().double())
    bn.train(training)
    x = r["x"].cpu().double().requires_grad_(True)
    y = torch.tanh(bn(x))
    (y * (r["gy"] + r["gy2"]).cpu().double()).sum().backward()
    return y.detach(), bn.running_mean, bn.running_var, x.grad, bn.bias.grad, bn.weight.grad


@pytest.mark.parametrize("d,N", REF_CASES, ids=REF_IDS)
def test_plain_training_against_float64_torch(d, N):
    r = _run(d, N)
    p, (gx, gbw) = r["plain"], r["plain_bwd"]
    y, rm, rv, gxr, gb, gw = _reference(r, True)
    assert_close(p["y"], y, 2e-5, 1e-6, "y")
    assert_close(p["rm"], rm, 2e-5, 1e-7, "running_mean")
    assert_close(p["rv"], rv, 2e-5, 1e-7, "running_var")
    assert_close(gx, gxr, 1e-4, 1e-6, "gx")
    assert_close(gbw[:d], gb, 1e-4, 1e-6, "grad bias")
    assert_close(gbw[d:], gw, 1e-4, 1e-6, "grad weight")


@pytest.mark.parametrize("d,N", REF_CASES, ids=REF_IDS)
def test_plain_eval_against_float64_torch(d, N):
    r = _run(d, N)
    e = _fwd_plain(r["x"], r["w"], r["b"], r["rm"], r["rv"], False)
    gx, gbw = _bwd_plain(r["x"], e["y"], r["gy"], r["gy2"], r["w"], e["mean"], e["invstd"], False)
    torch.cuda.synchronize()
    y, rm, rv, gxr, gb, gw = _reference(r, False)
    assert torch.equal(e["rm"], r["rm"]) and torch.equal(e["rv"], r["rv"])      # eval mode leaves the running estimates alone
    assert torch.equal(e["y"], e["y2"])
    assert_close(e["y"], y, 2e-5, 1e-6, "y")
    assert_close(gx, gxr, 1e-4, 1e-6, "gx")
    assert_close(gbw[:d], gb, 1e-4, 1e-6, "grad bias")
    assert_close(gbw[d:], gw, 1e-4, 1e-6, "grad weight")
