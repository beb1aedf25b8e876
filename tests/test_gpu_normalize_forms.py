"""GPU: the row normalise + dropout kernels of jmac_amd/csrc/norm.hip against oracles that do not come from the library.  The plain
launches, the fused row passes and (from 2048 rows on) their R-rows forms share one forward and one backward body, so the
fused-against-separate equalities of test_gpu_row_fusions.py partly compare a body with itself; here

  draws    the zero pattern of every seeded forward equals a host Philox4x32-10 mask (tests/sampler_ref.py, which reproduces the
           Random123 known answer): element 4c + j of row r is kept iff word j of philox4x32_10(counter = (lo32(i), hi32(i), 0, 0),
           key = (lo32(seed), hi32(seed))) < keep_thr, i = r * (d / 4) + c, keep_thr = floor((1 - float32(p)) * 2^32) clamped to
           0xFFFFFFFF; and the seeded forward equals the mask-form forward run with that host mask, bit for bit;
  values   forward, seeded backward (accumulate 0 and 1) and the adjoint + scatter launch (add, permutation map, accumulate) against
           float64 torch with the host mask, at the tolerances of test_gpu_encoder.py::test_normalize_dropout_kernels: assert_close
           (1e-6, 1e-7) forward, (1e-5, 1e-6) backward; the clamped rows (one all-zero, one with norm below eps) compared as there.

Shapes, the smallest that reach every path: d = 12 a partly filled first chunk, 300 the second chunk on lanes 0-10, 512 both chunks
full, 516 beyond the R-rows forms at every N and a third loop trip of the row-per-wave kernel; N = 5 ragged for R = 2 and R = 4,
N = 2049 the R-rows threshold plus a ragged last wave."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sampler_ref
from util import assert_close

DEV = "cuda"
FUSED_SHAPES = [(1, 12), (5, 12), (5, 300), (5, 512), (2049, 300), (2049, 512)]
SHAPES = FUSED_SHAPES + [(3, 516), (2049, 516)]
IDS = ["N%d-d%d" % s for s in SHAPES]
SEEDS = (0x9E3779B9, (0x1234ABCD << 32) | 0x0BADF00D)             # high word zero / nonzero
EPS = 1e-12


def _p32(p):
    return float(np.float32(p))                                   # the library takes p_drop as a float


def _scale(p):
    return float(np.float32(1.0 / (1.0 - _p32(p))))


@functools.lru_cache(maxsize=None)
def _host_keep_np(N, d, seed, p):
    D4 = d // 4
    i = np.arange(N * D4, dtype=np.uint64)
    thr = min(int(np.floor((1.0 - _p32(p)) * 4294967296.0)), 0xFFFFFFFF)
    w = sampler_ref.philox4x32_10(i & sampler_ref.M32, i >> np.uint64(32), np.zeros_like(i), np.zeros_like(i),
                                  seed & 0xFFFFFFFF, seed >> 32)
    return (np.stack(w, axis=1) < np.uint64(thr)).reshape(N, d)


def _host_keep(N, d, seed, p):
    """{0,1} float mask [N, d] on the device."""
    return torch.from_numpy(_host_keep_np(N, d, seed, p).astype(np.float32)).to(DEV)


def _seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device=DEV)


def test_host_keep_rates():
    """The host reference itself: keep rates near 1 - p and no all-dropped row at the shapes below (so that a zero pattern that
    equals it says something)."""
    for N, d in SHAPES:
        for p in (0.4, 0.05):
            for seed in SEEDS:
                k = _host_keep_np(N, d, seed, p)
                assert k.any(1).all(), (N, d, p)
                if N * d > 1000:
                    assert abs(k.mean() - (1 - p)) < 0.04, (N, d, p, k.mean())


@pytest.mark.parametrize("p", [0.4, 0.05])
@pytest.mark.parametrize("N,d", SHAPES, ids=IDS)
def test_seeded_draws_equal_host_philox(N, d, p):
    from jmac_amd import encoder, ops
    from jmac_amd._lib import check, lib, ptr, stream
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d)
    x = torch.randn(N, d, device=DEV, generator=gen) + 3.0        # no exact zeros among the normalised values
    perm = torch.randperm(N, device=DEV, generator=gen)
    for seed in SEEDS:
        what = "seed %#x" % seed
        keep = _host_keep(N, d, seed, p)
        sd = _seed_tensor(seed)
        y = torch.empty(N, d, device=DEV)
        inv, _ = encoder._norm_drop_fwd(x, p, True, y, seed=sd)
        assert torch.equal((y != 0).float(), keep), what
        y2, inv2 = torch.empty(N, d, device=DEV), torch.empty(N, device=DEV)
        check(lib().jmac_row_normalize_drop_fwd_f32(ptr(x), d, N, d, EPS, ptr(keep), d, _scale(p), ptr(y2), d, ptr(inv2), stream()))
        assert torch.equal(y, y2) and torch.equal(inv[:N], inv2), what
        if d > 512:
            continue
        y3 = torch.empty(N, d, device=DEV)
        xr, inv3, _ = encoder._gather_norm_drop_fwd(x, perm, p, True, y3, seed=sd)
        assert torch.equal(xr, x[perm]), what
        assert torch.equal((y3 != 0).float(), keep), what         # the index is the class-order row
        yb, yn = torch.empty(N, d, device=DEV), torch.empty(N, d, device=DEV)
        ops.bn_tanh_norm_fwd_raw(x, torch.ones(d, device=DEV), torch.full((d,), 0.5, device=DEV), torch.zeros(d, device=DEV),
                                 torch.ones(d, device=DEV), True, 0.1, 1e-5, yb, yn, ("seed", sd, p))
        assert bool((yb != 0).all()) and torch.equal((yn != 0).float(), keep), what


def _rows(N, d, gen):
    """normal rows, one all-zero (N >= 3) and one with norm below eps -> (x, indices of the clamped rows)"""
    x = torch.randn(N, d, device=DEV, generator=gen)
    tiny = 3 if N > 3 else 0
    x[tiny] = 1e-20
    clamped = [tiny]
    if N >= 3:
        x[1] = 0.0
        clamped.append(1)
    return x, clamped


@functools.lru_cache(maxsize=None)
def _case(N, d, p):
    """Inputs and the float64 reference of a shape, made once and left unchanged: forward y, inv and the adjoint gx of g."""
    seed = SEEDS[1]
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d + 7)
    x, clamped = _rows(N, d, gen)
    g = torch.randn(N, 2 * d, device=DEV, generator=gen)[:, d:]
    base = torch.randn(N, d, device=DEV, generator=gen)
    add = torch.randn(N, d, device=DEV, generator=gen)
    perm = torch.randperm(N, device=DEV, generator=gen)
    m = _host_keep(N, d, seed, p).double().cpu() * _scale(p)
    xr = x.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.normalize(xr, 2, -1, EPS) * m
    ref.backward(g.double().cpu())
    want = xr.grad.clone()
    for r in clamped:                                             # ||x|| <= eps: y = x / eps
        want[r] = g[r].double().cpu() * m[r] * 1e12
    normal = torch.ones(N, dtype=torch.bool)
    normal[clamped] = False
    ref_inv = 1.0 / xr.detach().norm(dim=-1).clamp_min(EPS)
    return dict(seed=_seed_tensor(seed), x=x, g=g, base=base, add=add, perm=perm, ref=ref.detach(), ref_inv=ref_inv, want=want,
                normal=normal, clamped=clamped)


def _check_adjoint(got, want, c, what):
    """non-clamped rows at (1e-5, 1e-6); each clamped row (values of the order of 1e12) at 1e-5 of its own magnitude"""
    got = got.double().cpu()
    if c["normal"].any():
        assert_close(got[c["normal"]], want[c["normal"]], 1e-5, 1e-6, what)
    for r in c["clamped"]:
        assert_close(got[r], want[r], 1e-5, what=what + " clamped row %d" % r)


@pytest.mark.parametrize("p", [0.4, 0.05])
@pytest.mark.parametrize("N,d", SHAPES, ids=IDS)
def test_seeded_forward_and_backward_against_float64(N, d, p):
    from jmac_amd import encoder
    c = _case(N, d, p)
    buf = torch.zeros(N, 3 * d, device=DEV)
    y = buf[:, d:2 * d]
    inv, drop = encoder._norm_drop_fwd(c["x"], p, True, y, seed=c["seed"])
    assert_close(y, c["ref"], 1e-6, 1e-7, "y")
    assert float(buf[:, :d].abs().max()) == 0.0 and float(buf[:, 2 * d:].abs().max()) == 0.0
    if c["normal"].any():
        assert_close(inv[:N].cpu()[c["normal"]], c["ref_inv"][c["normal"]], 1e-6, 1e-7, "inv")
    assert all(abs(float(inv[r]) - 1e12) <= 1e6 for r in c["clamped"])              # 1 / eps
    for acc in (0, 1):
        gx = c["base"].clone() if acc else torch.full((N, d), 7.0, device=DEV)
        encoder._norm_drop_bwd(c["x"], inv, drop, c["g"], gx, bool(acc))
        _check_adjoint(gx, c["want"] + (c["base"].double().cpu() if acc else 0.0), c, "gx accumulate %d" % acc)


@pytest.mark.parametrize("p", [0.4, 0.05])
@pytest.mark.parametrize("N,d", FUSED_SHAPES, ids=IDS[:len(FUSED_SHAPES)])
def test_adjoint_scatter_against_float64(N, d, p):
    """dst[map[r]] = base[map[r]] + add[r] + adjoint[r]"""
    from jmac_amd import encoder
    c = _case(N, d, p)
    inv, drop = encoder._norm_drop_fwd(c["x"], p, True, torch.empty(N, d, device=DEV), seed=c["seed"])
    got = encoder._norm_drop_bwd_scatter(c["x"], inv, drop, c["g"], c["add"], c["perm"], dst=c["base"].clone())
    perm = c["perm"].cpu()
    want = c["want"] + c["add"].double().cpu() + c["base"].double().cpu()[perm]
    _check_adjoint(got[c["perm"]], want, c, "dst")
