"""The case of tests/test_gpu_persistent_oracle.py: ONE seeded graph large enough for the
PERSISTENT-GRID forms of the aggregation kernels (more than 65 536 by-destination items without inline entries:
jmac_amd/graph.py INLINE_EDGES_MAX_ITEMS, aggregate.hip launch_rel_attn_fwd), seeded tables on it, and the oracle
(oracle/jmac_oracle.py aggregate_from_tables_sliced -- the reference's per-destination softmax / weighted sum of
modules/helper/message_passing.py:24-28 on the node / relation tables of src/jmac_model.py:75-88)."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_ENT, N_EDGE, N_REL = 80000, 600000, 100
SLOPE, OUT_SCALE = 0.05, 0.5
HUB_SOURCES = ((5, 2000), (N_ENT // 2, 700), (N_ENT - 3, 1300))      # sources with enough out-edges to be split in pass B


def graph(n=N_ENT, e=N_EDGE, nr=N_REL, seed=501):
    """Power-law destinations (hubs of 10^4 in-edges), Zipf relation types, uniform sources + three hub sources.
    -> (edge_index [2,E] int64, edge_type [E] int64, N, nrel) with nrel = nr + 1 (the loop row)."""
    from jmac_amd import synth
    ei, et, n, nrel = synth.power_law_graph(n, e, nr, seed=seed)
    rng = np.random.default_rng(seed + 1)
    pos, off = rng.permutation(e), 0
    for hub, cnt in HUB_SOURCES:
        cnt = min(cnt, e // 8)
        ei[1, pos[off:off + cnt]] = min(hub, n - 1)
        off += cnt
    return ei, et, n, nrel


def tables(n, nrel, d, seed=7):
    """fp32 [P|Q|Z] [n,3d], [Rq|Rz] [nrel,2d], a [d], upstream gradient G [n,d] (CPU generator: the same bits in every process)."""
    gen = torch.Generator().manual_seed(seed)
    PQZ = torch.randn(n, 3 * d, generator=gen) * 0.3
    RR = torch.randn(nrel, 2 * d, generator=gen) * 0.3
    a = torch.randn(d, generator=gen) * 0.1
    G = torch.randn(n, d, generator=gen)
    return PQZ, RR, a, G


def oracle_aggregate(PQZ, RR, a, ei, et, loop_rel, dtype, G=None, kink_mask=None, nslices=8):
    """out_scale * (nb + Z - Rz[loop]) of the oracle in ``dtype`` (+ (dPQZ, dRR, da) of sum(out * G) with G), evaluated in
    destination slices (oracle.aggregate_from_tables_sliced)."""
    import oracle.jmac_oracle as orc
    return orc.aggregate_from_tables_sliced(PQZ, RR, a, torch.from_numpy(ei), torch.from_numpy(et), SLOPE, loop_rel, OUT_SCALE,
                                            dtype, G, kink_mask, nslices)


def rel_err(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


# ---- the two small cases of tests/test_gpu_hw_variants.py (tools/aggregate_bits_dump.py runs them too) ----
def small_graph():
    """N = 300, E = 3000, 7 relations + the loop relation; destination 0 has 200 in-edges (four 64-entry batches), destinations
    290 .. 299 have none."""
    rng = np.random.default_rng(11)
    n, e, nr = 300, 3000, 7
    dst = rng.integers(1, 290, size=e)
    dst[:200] = 0
    ei = np.stack([dst, rng.integers(0, n, size=e)]).astype(np.int64)
    et = rng.integers(0, nr, size=e).astype(np.int64)
    return ei, et, n, nr + 1


@functools.lru_cache(maxsize=None)
def coop_case():
    """N = 17 000 destinations (just past the 16 384 items where the launcher leaves the U = 2 form), 7 relations + the loop
    relation.  In-degrees: 17, 23, ..., 251 and 256 (cooperative segments: four quarters, of exactly 64 entries for 256);
    257, 300, 513, 700 (split at 256: multi-batch items, a 1-entry item, the combine pass); 1, 2, 3, 5; the rest from
    {0 .. 4} with the number of empty rows not a multiple of kEmptyPack = 4.  -> (edge_index, edge_type, N, nrel, degrees)"""
    rng = np.random.default_rng(23)
    n, nr = 17000, 7
    special = [17 + 6 * r for r in range(40)] + [256, 257, 300, 513, 700, 1, 2, 3, 5]
    deg = rng.integers(0, 5, size=n)
    rows = rng.permutation(n)
    deg[rows[:len(special)]] = special
    if int((deg == 0).sum()) % 4 == 0:
        deg[rows[len(special)]] = 0 if deg[rows[len(special)]] else 1
    dst = np.repeat(np.arange(n), deg)
    e = dst.size
    order = rng.permutation(e)
    ei = np.stack([dst, rng.integers(0, n, size=e)])[:, order].astype(np.int64)
    et = rng.integers(0, nr, size=e)[order].astype(np.int64)
    return ei, et, n, nr + 1, deg
