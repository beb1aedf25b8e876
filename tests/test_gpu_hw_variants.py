"""GPU: the half-wave forward kernel against the 64-lane kernels of jmac_amd/csrc/aggregate.hip, which the testing build's
entry points keep at the widths the product gives to the half-wave kernel (ops.rel_attn_split_fwd_raw(..., lanes64=True)):

  * on a graph large enough for the persistent grid the two agree to rounding (a different summation tree across lanes), on
    fp32 tables and on padded bf16 tables;
  * on a graph small enough to carry inline entries both entry points choose the 64-lane U = 2 kernel -- the testing entry
    point differs from the product's in the half-wave gate alone -- so out, seg_max and seg_den are bitwise equal;
  * on a schedule with COOPERATIVE segments and no inline entries (a combination graph.py does not build: its cooperative
    schedules carry inline entries and take the U = 2 kernel) the half-wave kernel and the 64-lane U = 4 kernel both walk the
    cooperative section, the split items and the empty packs: against the float64 oracle, and against each other."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import persistent_case as pc  # noqa: E402

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


@pytest.mark.parametrize("table", ["f32", "bf16-padded"])
@pytest.mark.parametrize("d", [300, 256])
def test_small_graph_testing_entry_equals_product_bitwise(d, table):
    from jmac_amd import ops
    from jmac_amd.graph import RelGraph
    dev = torch.device("cuda")
    ei, et, n, nrel = pc.small_graph()
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


@functools.lru_cache(maxsize=None)
def _coop_tables(d, table):
    """([P|Q|Z], [Rq|Rz], a) on the CPU and the float64 oracle on them (bf16: on the rounded tables)."""
    ei, et, n, nrel, _ = pc.coop_case()
    PQZ, RR, a, _ = pc.tables(n, nrel, d, seed=d)
    if table == "bf16-padded":
        PQZ, RR = PQZ.to(torch.bfloat16), RR.to(torch.bfloat16)
    ref = pc.oracle_aggregate(PQZ.double(), RR.double(), a, ei, et, nrel - 1, torch.float64)
    return PQZ, RR, a, ref


@pytest.mark.parametrize("table", ["f32", "bf16-padded"])
@pytest.mark.parametrize("d", [300, 256])
def test_cooperative_schedule_without_inline_entries(d, table):
    """The half-wave kernel (product entry) and the 64-lane U = 4 kernel (lanes64 entry) on cooperative segments."""
    from jmac_amd import ops
    from jmac_amd.graph import RelGraph, _Schedule
    dev = torch.device("cuda")
    ei, et, n, nrel, deg = pc.coop_case()
    g = RelGraph(torch.from_numpy(ei).to(dev), torch.from_numpy(et).to(dev), n, nrel, chunk=256)
    g.by_dst = _Schedule(g.rowptr, n, ei.shape[1], 256, None, coop=True)
    s = g.by_dst
    n_empty = int((deg == 0).sum())
    assert s.item_edges is None and s.n_items_max > 16384 and s.n_coop >= 41 and s.n_splits_max > s.n_coop
    assert s.n_empty == n_empty and n_empty >= 1000 and n_empty % 4 != 0
    PQZ, RR, a, ref = _coop_tables(d, table)
    PQZ, RR, a = PQZ.to(dev), RR.to(dev), a.to(dev)
    if table == "bf16-padded":
        PQZ, RR = ops.pad_table(PQZ, d, 3), ops.pad_table(RR, d, 2)
        assert PQZ.shape[1] == 3 * ops.bf16_pad(d)
    P, QZ = ops.pqz_views(PQZ)
    hw = ops.rel_attn_split_fwd_raw(P, QZ, RR, a, g, pc.SLOPE, pc.OUT_SCALE, nrel - 1, 0)
    l64 = ops.rel_attn_split_fwd_raw(P, QZ, RR, a, g, pc.SLOPE, pc.OUT_SCALE, nrel - 1, 0, lanes64=True)
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    assert scale > 0.1
    e_hw = float((hw[0].double().cpu() - ref).abs().max())
    e_64 = float((l64[0].double().cpu() - ref).abs().max())
    e_x = float((hw[0] - l64[0]).abs().max())
    print("cooperative d=%d %s: half-wave vs oracle %.2e, lanes64 vs oracle %.2e, half-wave vs lanes64 %.2e (of scale)"
          % (d, table, e_hw / scale, e_64 / scale, e_x / scale))
    assert e_hw <= 1e-4 * scale                   # test_gpu_persistent_oracle.py's RTOL
    assert e_64 <= 1e-4 * scale
    assert e_x <= 2e-5 * scale                    # test_half_wave_forms_agree's bound
    empty = torch.from_numpy(deg == 0)
    for res in (hw, l64):
        assert bool((res[1][:n].cpu()[empty] == -float("inf")).all()) and bool((res[2][:n].cpu()[empty] == 0).all())
