"""GPU: the half-wave forward kernel against the 64-lane kernels of jmac_amd/csrc/aggregate.hip, which the testing build's
entry points keep at the widths the product gives to the half-wave kernel (ops.rel_attn_split_fwd_raw(..., lanes64=True)):

  * on a graph large enough for the persistent grid the two agree to rounding (a different summation tree across lanes), on
    fp32 tables and on padded bf16 tables;
  * on a graph small enough to carry inline entries both entry points choose the 64-lane U = 2 kernel -- the testing entry
    point differs from the product's in the half-wave gate alone -- so out, seg_max and seg_den are bitwise equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_half_wave_forms_agree():
    from jmac_amd import ops, synth
    from jmac_amd.graph import RelGraph
    dev = torch.device("cuda")
    n, e, nr, d = 80000, 1000000, 120, 300
    ei, et, n, nrel = synth.power_law_graph(n, e, nr, seed=77)
    g = RelGraph(torch.from_numpy(ei).to(dev), torch.from_numpy(et).to(dev), n, nrel)
    assert g.by_dst.n_items_max > 65536 and g.by_dst.item_edges is None       # the persistent form (graph.INLINE_EDGES_MAX_ITEMS)
    gen = torch.Generator(device=dev).manual_seed(5)
    PQZ = torch.randn(n, 3 * d, device=dev, generator=gen) * 0.3
    RR = torch.randn(nrel, 2 * d, device=dev, generator=gen) * 0.3
    av = torch.randn(d, device=dev, generator=gen) * 0.1
    with torch.no_grad():
        P16, R16 = ops.pad_table(PQZ.to(torch.bfloat16), d, 3), ops.pad_table(RR.to(torch.bfloat16), d, 2)
        o32 = ops.rel_attn_aggregate(PQZ, RR, av, g, 0.05, nrel - 1, 0.5).cpu().numpy()
        o16 = ops.rel_attn_aggregate(P16, R16, av, g, 0.05, nrel - 1, 0.5).cpu().numpy()
        w32 = ops.rel_attn_split_fwd_raw(*ops.pqz_views(PQZ), RR, av, g, 0.05, 0.5, nrel - 1, 0, lanes64=True)[0].cpu().numpy()
        w16 = ops.rel_attn_split_fwd_raw(*ops.pqz_views(P16), R16, av, g, 0.05, 0.5, nrel - 1, 0, lanes64=True)[0].cpu().numpy()
    assert np.isfinite(o32).all() and np.isfinite(o16).all() and float(np.abs(o32).max()) > 0.1
    scale = float(np.abs(o32).max())
    assert float(np.abs(w32 - o32).max()) <= 2e-5 * scale
    assert float(np.abs(w16 - o16).max()) <= 2e-5 * scale


def _small_graph():
    """N = 300, E = 3000, 7 relations + the loop relation; destination 0 has 200 in-edges (four 64-entry batches), destinations
    290 .. 299 have none."""
    rng = np.random.default_rng(11)
    n, e, nr = 300, 3000, 7
    dst = rng.integers(1, 290, size=e)
    dst[:200] = 0
    ei = np.stack([dst, rng.integers(0, n, size=e)]).astype(np.int64)
    et = rng.integers(0, nr, size=e).astype(np.int64)
    return ei, et, n, nr + 1


@pytest.mark.parametrize("table", ["f32", "bf16-padded"])
@pytest.mark.parametrize("d", [300, 256])
def test_small_graph_testing_entry_equals_product_bitwise(d, table):
    from jmac_amd import ops
    from jmac_amd.graph import RelGraph
    dev = torch.device("cuda")
    ei, et, n, nrel = _small_graph()
    g = RelGraph(torch.from_numpy(ei).to(dev), torch.from_numpy(et).to(dev), n, nrel)
    assert g.by_dst.item_edges is not None                                    # inline entries: the small-graph form
    deg = np.bincount(ei[0], minlength=n)
    assert deg.min() == 0 and deg.max() > 64
    gen = torch.Generator().manual_seed(d)
    PQZ = (torch.randn(n, 3 * d, generator=gen) * 0.3).to(dev)
    RR = (torch.randn(nrel, 2 * d, generator=gen) * 0.3).to(dev)
    av = (torch.randn(d, generator=gen) * 0.1).to(dev)
    if table == "bf16-padded":
        PQZ, RR = ops.pad_table(PQZ.to(torch.bfloat16), d, 3), ops.pad_table(RR.to(torch.bfloat16), d, 2)
        assert PQZ.shape[1] == 3 * ops.bf16_pad(d)
    P, QZ = ops.pqz_views(PQZ)
    want = ops.rel_attn_split_fwd_raw(P, QZ, RR, av, g, 0.05, 0.5, nrel - 1, 0)
    got = ops.rel_attn_split_fwd_raw(P, QZ, RR, av, g, 0.05, 0.5, nrel - 1, 0, lanes64=True)
    torch.cuda.synchronize()
    out = want[0].cpu().numpy()
    assert np.isfinite(out).all() and float(np.abs(out).max()) > 0.1
    for name, w, v in zip(("out", "seg_max", "seg_den"), want, got):
        assert torch.equal(w[:n], v[:n]), name
    assert bool((want[1][:n].cpu()[torch.from_numpy(deg == 0)] == -float("inf")).all())
