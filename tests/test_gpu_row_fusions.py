"""GPU: the fused row passes of the encoder node's completion chain (jmac_amd/encoder.py: FUSE_ROW_PASSES; kernels in
jmac_amd/csrc/norm.hip) against the separate launches they replace, composed here from the raw wrappers:

  A  _gather_rows + _norm_drop_fwd                               ->  _gather_norm_drop_fwd                    bit-equal
  B  ops.bn_tanh_fwd_raw + _norm_drop_fwd (+ _gather_rows of y)   ->  ops.bn_tanh_norm_fwd_raw                 bit-equal
  C+D  _norm_drop_bwd + ops.bn_tanh_bwd_raw (+ _gather_rows of gy2) -> ops.bn_tanh_bwd_normadj_raw
       per row bit-equal (checked through D with unit statistics); error against a float64 reference at most twice that of the
       separate launches -- and, the column sums being kept in the separate launches' order, bit-equal as well
  E  _norm_drop_bwd(accumulate) + _scatter_rows                  ->  _norm_drop_bwd_scatter                   bit-equal

Shapes: d = 300 (the second column chunk is valid on lanes 0-10 only), 64 (one chunk, lanes 16-63 idle), 512 (both chunks full);
N = 1, 5, 1031 (no multiple of the rows per wave; 1031 no multiple of the waves per block either); row map none / identity / a
random permutation; destination pitch 2d and 3d; p_drop 0 and 0.4 (seed form); one all-zero row and one row with norm below eps;
with and without the second gradient; and N = 2053, d = 300: from 2048 rows on the separate normalise launches take the
four-rows-per-wave form, whose adjoint is rounded differently from the row-per-wave kernels' (norm.hip spells both forms out; a
fused launch takes the form of the launch it replaces).  From that row count on the separate launches and the fused ones run the
same forward and backward body, so A and E compare a body with itself there: tests/test_gpu_normalize_forms.py holds oracles from
outside the library.  Then the node itself, FUSE_ROW_PASSES on against off."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from util import assert_close, rel_err

DEV = "cuda"
SHAPES = [(N, d) for d in (300, 64, 512) for N in (1, 5, 1031)]
SHAPE_IDS = ["N%d-d%d" % s for s in SHAPES]
P_DROPS = (0.0, 0.4)


def _maps(N, gen):
    """row map: none, identity, a random permutation"""
    return {"none": None, "identity": torch.arange(N, device=DEV), "perm": torch.randperm(N, device=DEV, generator=gen)}


def _rows(N, d, gen, scale=1.0):
    """[N, d] normal rows with one all-zero row and one row whose norm is below F.normalize's eps (N = 1: the latter alone)."""
    x = torch.randn(N, d, device=DEV, generator=gen) * scale
    if N > 3:
        x[1] = 0.0
        x[3] = 1e-20
    else:
        x[0] = 1e-20
    return x


def _seed(gen):
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=DEV, generator=gen)


def _pitched(N, d, pitch):
    """A [N, d] block of a [N, pitch * d] cat buffer (not the first one) and the buffer."""
    buf = torch.zeros(N, pitch * d, device=DEV)
    return buf[:, d:2 * d], buf


@pytest.mark.parametrize("N,d", SHAPES + [(2053, 300)], ids=SHAPE_IDS + ["N2053-d300"])
def test_gather_normalize_dropout_forward_is_bit_equal(N, d):
    """A.  (N = 2053: the separate normalise launch takes its four-rows-per-wave form there.)"""
    from jmac_amd import encoder
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d)
    x, seed = _rows(N, d, gen), _seed(gen)
    for mname, rmap in _maps(N, gen).items():
        for pitch in (2, 3):
            for p in P_DROPS:
                what = "map %s pitch %dd p_drop %g" % (mname, pitch, p)
                (xg,) = encoder._gather_rows([x], rmap) if rmap is not None else (x,)
                y0, buf0 = _pitched(N, d, pitch)
                inv0, drop0 = encoder._norm_drop_fwd(xg, p, True, y0, seed=seed)
                y1, buf1 = _pitched(N, d, pitch)
                xr, inv1, drop1 = encoder._gather_norm_drop_fwd(x, rmap, p, True, y1, seed=seed)
                assert torch.equal(xr, xg), what
                assert torch.equal(buf1, buf0) and torch.equal(inv1[:N], inv0[:N]), what     # (the whole buffer: nothing beside the block)
                assert (drop1 is None) == (drop0 is None) and (drop1 is None or drop1[2] == drop0[2]), what
                if p > 0 and N >= 1000:                                                      # the draws were made (keep rate 0.6;
                    kept = (y1[(xg != 0).any(1)] != 0).float().mean()                        # 5 sigma at these sizes < 0.01)
                    assert 0.59 < float(kept) < 0.61, what


def _bn(d, gen, unit=False):
    bn = torch.nn.BatchNorm1d(d).to(DEV)
    if not unit:
        with torch.no_grad():
            bn.weight.copy_(torch.rand(d, device=DEV, generator=gen) + 0.5)
            bn.bias.copy_(torch.rand(d, device=DEV, generator=gen) * 0.4 - 0.2)
            bn.running_mean.copy_(torch.randn(d, device=DEV, generator=gen) * 0.1)
            bn.running_var.copy_(torch.rand(d, device=DEV, generator=gen) + 0.5)
    return bn


def _bn_state(bn):
    return {k: v.clone() for k, v in bn.state_dict().items()}


@pytest.mark.parametrize("N,d", SHAPES + [(2053, 300)], ids=SHAPE_IDS + ["N2053-d300"])
def test_bn_tanh_normalize_dropout_forward_is_bit_equal(N, d):
    """B: both copies of c1, the cat block, inv, the statistics and the running estimates.  Batch statistics on normal rows; running
    statistics (mean 0, bias 0) on rows of which one is zero and one tiny, so that c1 has an all-zero row and one below eps."""
    from jmac_amd import encoder, ops
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d + 1)
    seed = _seed(gen)
    for training in (True, False):
        bn = _bn(d, gen)
        x = torch.randn(N, d, device=DEV, generator=gen) * 0.5 + 0.1
        if not training:
            with torch.no_grad():
                bn.bias.zero_()
                bn.running_mean.zero_()
            x = _rows(N, d, gen, 0.5)
        state = _bn_state(bn)
        for mname, rmap in _maps(N, gen).items():
            for pitch in (2, 3):
                for p in P_DROPS:
                    what = "training %s map %s pitch %dd p_drop %g" % (training, mname, pitch, p)
                    bn.load_state_dict(state)
                    y0 = torch.empty(N, d, device=DEV)
                    mean0, invstd0 = ops.bn_tanh_fwd_raw(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum,
                                                         bn.eps, y0)
                    yn0, buf0 = _pitched(N, d, pitch)
                    inv0, _ = encoder._norm_drop_fwd(y0, p, True, yn0, seed=seed)
                    after0 = _bn_state(bn)
                    yr0 = None
                    if rmap is not None:                              # today's output gather: out[map[r]] = y[r]
                        back = torch.empty_like(rmap)
                        back[rmap] = torch.arange(N, device=DEV)
                        (yr0,) = encoder._gather_rows([y0], back)
                    bn.load_state_dict(state)
                    y1 = torch.empty(N, d, device=DEV)
                    yr1 = torch.full((N, d), float("nan"), device=DEV) if rmap is not None else None
                    yn1, buf1 = _pitched(N, d, pitch)
                    mean1, invstd1, inv1 = ops.bn_tanh_norm_fwd_raw(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training,
                                                                    bn.momentum, bn.eps, y1, yn1, encoder._seed_drop(p, True, seed),
                                                                    rmap, yr1)
                    assert torch.equal(y1, y0) and torch.equal(buf1, buf0) and torch.equal(inv1[:N], inv0[:N]), what
                    assert torch.equal(mean1, mean0) and torch.equal(invstd1, invstd0), what
                    if rmap is not None:
                        assert torch.equal(yr1, yr0), what
                    for k, v in _bn_state(bn).items():
                        assert torch.equal(v, after0[k]), (what, k)
        if not training and N > 3:
            assert float(y1[1].abs().max()) == 0.0 and float(inv1[3]) > 9e11         # the zero row, the clamped norm


@pytest.mark.parametrize("N,d", SHAPES + [(2053, 300)], ids=SHAPE_IDS + ["N2053-d300"])
def test_normalize_adjoint_scatter_is_bit_equal(N, d):
    """E: with and without the table that is added, onto a destination (accumulate) and into a fresh one."""
    from jmac_amd import encoder
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d + 2)
    x, seed = _rows(N, d, gen), _seed(gen)
    add = torch.randn(N, d, device=DEV, generator=gen)
    base = torch.randn(N, d, device=DEV, generator=gen)
    for mname, rmap in _maps(N, gen).items():
        pos32 = None
        if rmap is not None:
            pos32 = torch.empty(N, dtype=torch.int32, device=DEV)
            pos32[rmap] = torch.arange(N, dtype=torch.int32, device=DEV)
        for pitch in (2, 3):
            g = torch.randn(N, pitch * d, device=DEV, generator=gen)[:, d:2 * d]
            for p in P_DROPS:
                y, _ = _pitched(N, d, 2)
                inv, drop = encoder._norm_drop_fwd(x, p, True, y, seed=seed)
                for with_add in (True, False):
                    for onto in (True, False):
                        what = "map %s pitch %dd p_drop %g add %s accumulate %s" % (mname, pitch, p, with_add, onto)
                        gx = add.clone() if with_add else torch.empty(N, d, device=DEV)
                        encoder._norm_drop_bwd(x, inv, drop, g, gx, with_add)
                        if pos32 is not None:
                            want = encoder._scatter_rows(gx, pos32, dst=base.clone() if onto else None)
                        else:
                            want = base + gx if onto else gx
                        got = encoder._norm_drop_bwd_scatter(x, inv, drop, g, add if with_add else None, rmap,
                                                             dst=base.clone() if onto else None)
                        assert torch.equal(got, want), what


def _dyadic(N, d, gen):
    """Values k / 8, |k| <= 7: y * y and 1 - y * y are exact in fp32, so g (1 - y^2) is ONE rounding however it is contracted."""
    return torch.randint(-7, 8, (N, d), device=DEV, generator=gen).float() / 8.0


@pytest.mark.parametrize("N,d", SHAPES + [(2053, 300)], ids=SHAPE_IDS + ["N2053-d300"])
def test_bn_backward_forms_the_adjoint_per_row_bit_equal(N, d):
    """D with unit BatchNorm statistics (mean 0, invstd 1, weight 1, running statistics applied) and no second gradient writes
    gx = gy (1 - y^2) with gy the adjoint it formed in registers.  y (the adjoint's x) holds dyadic values, so 1 - y^2 is exact
    and the product one rounding: gx must equal _norm_drop_bwd's table times (1 - y^2), bit for bit."""
    from jmac_amd import encoder, ops
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d + 3)
    y, seed = _dyadic(N, d, gen), _seed(gen)
    if N > 3:
        y[1] = 0.0
        y[3] = 2.0 ** -50
    else:
        y[0] = 2.0 ** -50
    x = torch.randn(N, d, device=DEV, generator=gen)
    one, zero = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    for pitch in (2, 3):
        g = torch.randn(N, pitch * d, device=DEV, generator=gen)[:, d:2 * d]
        for p in P_DROPS:
            yn, _ = _pitched(N, d, 2)
            inv, drop = encoder._norm_drop_fwd(y, p, True, yn, seed=seed)
            gy = torch.empty(N, d, device=DEV)
            encoder._norm_drop_bwd(y, inv, drop, g, gy, False)
            gx, _ = ops.bn_tanh_bwd_normadj_raw(x, y, inv, drop, g, None, None, one, zero, one, False)
            assert torch.equal(gx, gy * (1.0 - y * y)), "pitch %dd p_drop %g" % (pitch, p)


def _reference64(x, bn_w, bn_b, mean, var, eps, keep_scale, g, g2):
    """float64, CPU: tanh(BN(x)) -> normalise -> the given keep mask (times its scale), differentiated by autograd ->
    (gx, [grad bias | grad weight]).  mean / var None: batch statistics."""
    x = x.detach().double().cpu().requires_grad_(True)
    w, b = bn_w.detach().double().cpu().requires_grad_(True), bn_b.detach().double().cpu().requires_grad_(True)
    mu = x.mean(0) if mean is None else mean.double().cpu()
    va = x.var(0, unbiased=False) if var is None else var.double().cpu()
    y = torch.tanh((x - mu) / torch.sqrt(va + eps) * w + b)
    ss = (y * y).sum(-1, keepdim=True)
    clamped = ss <= 1e-24                                            # ||y|| <= eps: y / eps (both branches finite: no NaN from autograd)
    yn = torch.where(clamped, y / 1e-12, y / torch.sqrt(torch.where(clamped, torch.ones_like(ss), ss)))
    loss = (yn * keep_scale.double().cpu() * g.double().cpu()).sum()
    if g2 is not None:
        loss = loss + (y * g2.double().cpu()).sum()
    loss.backward()
    return x.grad, torch.cat((b.grad, w.grad))


@pytest.mark.parametrize("N,d", SHAPES + [(2053, 300)], ids=SHAPE_IDS + ["N2053-d300"])
def test_bn_backward_with_adjoint_within_twice_the_separate_launches_error(N, d):
    """C + D against a float64 reference: max-norm error (util.rel_err) of gx and [grad bias | grad weight] at most twice that of
    _norm_drop_bwd + ops.bn_tanh_bwd_raw (the factor: another association of an N-term column sum).  The keep mask is read back
    from the separate forward run on a table of ones.  Measured on MI355X (worst case over the combinations of a shape,
    separate / fused): see profiles/row_fusion_timing.txt."""
    from jmac_amd import encoder, ops
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d + 4)
    seed = _seed(gen)
    worst = {}
    for training in (True, False):
        bn = _bn(d, gen)
        x = torch.randn(N, d, device=DEV, generator=gen) * 0.5 + 0.1
        if not training:                                          # running statistics: c1 with a zero row and one below eps
            with torch.no_grad():
                bn.bias.zero_()
                bn.running_mean.zero_()
            x = _rows(N, d, gen, 0.5)
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        y = torch.empty(N, d, device=DEV)
        mean, invstd = ops.bn_tanh_fwd_raw(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps, y)
        g2_rows = torch.randn(N, d, device=DEV, generator=gen)
        maps = _maps(N, gen)
        for pitch in (2, 3):
            g = torch.randn(N, pitch * d, device=DEV, generator=gen)[:, d:2 * d]
            for p in P_DROPS:
                ones_out, _ = _pitched(N, d, 2)
                encoder._norm_drop_fwd(torch.ones(N, d, device=DEV), p, True, ones_out, seed=seed)
                keep_scale = (ones_out != 0).float() * (1.0 / (1.0 - p))
                yn, _ = _pitched(N, d, 2)
                inv, drop = encoder._norm_drop_fwd(y, p, True, yn, seed=seed)
                gy = torch.empty(N, d, device=DEV)
                encoder._norm_drop_bwd(y, inv, drop, g, gy, False)
                for with_g2 in (True, False):
                    # (the reference knows no row order: one per combination, shared by the row maps)
                    ref_gx, ref_gbw = _reference64(x, bn.weight, bn.bias, None if training else rm, None if training else rv,
                                                   bn.eps, keep_scale, g, g2_rows if with_g2 else None)
                    for mname, rmap in maps.items():
                        what = "training %s map %s pitch %dd p_drop %g gy2 %s" % (training, mname, pitch, p, with_g2)
                        # the second gradient arrives in the caller's order: its row map[r] belongs to row r
                        g2_caller = g2_today = None
                        if with_g2:
                            g2_caller = g2_rows
                            if rmap is not None:
                                g2_caller = torch.empty_like(g2_rows)
                                g2_caller[rmap] = g2_rows
                            (g2_today,) = encoder._gather_rows([g2_caller], rmap) if rmap is not None else (g2_caller,)
                        gx0, gbw0 = ops.bn_tanh_bwd_raw(x, y, gy, g2_today, bn.weight, mean, invstd, training)
                        gx1, gbw1 = ops.bn_tanh_bwd_normadj_raw(x, y, inv, drop, g, g2_caller, rmap, bn.weight, mean, invstd, training)
                        for name, got0, got1, ref in (("gx", gx0, gx1, ref_gx), ("gbw", gbw0, gbw1, ref_gbw)):
                            e0, e1 = rel_err(got0, ref), rel_err(got1, ref)
                            key = (training, name)
                            if key not in worst or e1 > worst[key][1]:
                                worst[key] = (e0, e1)
                            assert e1 <= 2.0 * e0, "%s %s: fused %.3e, separate %.3e" % (what, name, e1, e0)
                            # (more than was asked: the fused partial pass keeps the separate one's summation order)
                            assert torch.equal(got1, got0), "%s %s: not the separate launches' bits" % (what, name)
    for (training, name), (e0, e1) in sorted(worst.items()):
        print("N %d d %d %s %s: rel_err separate %.3e fused %.3e" % (N, d, "batch-stats" if training else "running-stats", name, e0, e1))


# ---- the node --------------------------------------------------------------------------------------------------------------------------
def _args(d, dropout):
    return types.SimpleNamespace(dim=d, dropout=dropout, leaky_relu_w=0.05, comp_op="sub", num_gcn_layer=2, num_negative=5,
                                 margin_align=1.0, margin_completion=5.0, batch_size=64, no_name_info=False, device=DEV)


def _node_setup(d):
    """A forward_name model on 301 entities of all four classes: 0-99 destinations only, 100-149 both, 150-249 sources only,
    250-300 isolated."""
    from jmac_amd.model import JMAC
    n, nr, di, e = 301, 11, 20, 900
    torch.manual_seed(21)
    rng = np.random.default_rng(21)
    m = JMAC(_args(d, 0.4), rng.standard_normal((n, di)).astype(np.float32), nr, n).to(DEV)
    m.ent_info_att = m.ent_info_att.to(DEV)
    with torch.no_grad():
        for lay in (m.conv1_alignment, m.conv2_alignment, m.conv1_completion):
            lay.bn.weight.add_(0.1 * torch.randn_like(lay.bn.weight))
            lay.bn.bias.add_(0.1 * torch.randn_like(lay.bn.bias))
    dst, src = rng.integers(0, 150, e), rng.integers(100, 250, e)
    ei = torch.from_numpy(np.stack([dst, src]).astype(np.int64)).to(DEV)
    et = torch.from_numpy(rng.integers(0, nr, e).astype(np.int64)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(22)
    G = {k: torch.randn(s, device=DEV, generator=gen) for k, s in (("align", (n, d)), ("c1", (n, d)), ("r1", (nr, d)))}
    B, K = 32, 5
    h, t = (torch.randint(0, n, (B * (K + 1),), device=DEV, generator=gen) for _ in range(2))
    r = torch.randint(0, nr, (B * (K + 1),), device=DEV, generator=gen)
    return m, ei, et, n, nr, G, (h, r, t, B)


@pytest.mark.parametrize("mode", ["train", "eval", "c1-only"])
@pytest.mark.parametrize("d", [64, 300])
def test_node_with_fused_row_passes_equals_the_separate_launches(d, mode, monkeypatch):
    """FUSE_ROW_PASSES on against off, class order on (ACTIVE_ROWS_MIN_N lowered), same parameters, BatchNorm buffers and dropout
    seeds: outputs bit-equal, every gradient within assert_close(rtol = 1e-5) of the separate launches' (a tenth of the project's
    1e-4 bar; the BatchNorm backward's column sums are associated differently), the same number of gradient buffers taken over.
    "c1-only": the loss reads c1 alone, so the backward has no adjoint to form and keeps today's launches behind a fused forward."""
    from jmac_amd import encoder, losses
    from jmac_amd.graph import graph_cache
    monkeypatch.setattr(encoder, "ACTIVE_ROWS_MIN_N", 64)
    m, ei, et, n, nr, G, (h, r, t, B) = _node_setup(d)
    m.train(mode != "eval")
    state = {k: v.clone() for k, v in m.state_dict().items()}
    calls = []
    real = encoder._gather_norm_drop_fwd
    monkeypatch.setattr(encoder, "_gather_norm_drop_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(encoder, "FUSE_ROW_PASSES", flag)
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)                                      # the dropout seed words are redrawn from this
        before = encoder.INPLACE_COUNT
        align_out, comp, rel = m.forward_base(ei, et, [0, n], [0, nr])
        if mode == "c1-only":
            loss = (comp[1] * G["c1"]).sum()
        else:
            loss = ((align_out * G["align"]).sum() + (comp[1] * G["c1"]).sum() + (rel[1] * G["r1"]).sum()
                    + losses.triple_l1_margin_loss(comp[0], rel[0], h, r, t, B, m.margin_completion).sum())
        loss.backward()
        res[flag] = ((align_out.detach(), comp[1].detach(), rel[1].detach()),
                     {k: (p.grad.clone() if p.grad is not None else None) for k, p in m.named_parameters()},
                     encoder.INPLACE_COUNT - before,
                     {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k})
    ro = graph_cache.get(ei, et, n, nr + 1, m.conv1_completion.chunk)._row_orders[None]
    assert 0 < ro.s0 < ro.nD < ro.s1 < n and len(calls) == 1          # all four classes; the fused path ran (once: flag on)
    for a, b, what in zip(res[True][0], res[False][0], ("align_out", "c1", "rel_c1")):
        assert torch.equal(a, b), what
    for k, v in res[False][3].items():
        assert torch.equal(res[True][3][k], v), k
    assert res[True][2] == res[False][2] == (0 if mode == "c1-only" else 2), (res[True][2], res[False][2])
    # d loss / d loop_rel is mathematically ZERO under batch statistics (a constant row shift cancels in the batch mean, util.
    # assert_close): what the kernels leave there is the rounding residue of column sums over gradients of the size of the others,
    # so its bound is the same 1e-5 taken of the largest gradient instead of its own (near-zero) magnitude
    scale = max(float(g_.abs().max()) for g_ in res[False][1].values() if g_ is not None)
    checked = 0
    for k, ref in res[False][1].items():
        got = res[True][1][k]
        if ref is None:
            assert got is None, k
            continue
        zero = k.endswith("loop_rel") and mode != "eval"
        print("%-44s max|err| %.3e of max|ref| %.3e" % (k, float((got - ref).abs().max()), float(ref.abs().max())))
        assert_close(got, ref, 1e-5, atol=1e-5 * scale if zero else 1e-6, what="grad " + k)
        checked += 1
    assert checked >= 10, checked
