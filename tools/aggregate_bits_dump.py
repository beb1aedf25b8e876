"""out, seg_max and seg_den of the forward aggregation kernels of aggregate.hip, for comparing two builds of the library bit for
bit (profiles/fwd_schedule_one_walk.txt, section 3).  One process per build; JMAC_LIB_PATH selects the library, and the testing
build (the lanes64 entry points) is taken from the same directory:

  JMAC_LIB_PATH=<build A>/libjmac_hip.so python tools/aggregate_bits_dump.py --write DIR --digest
  JMAC_LIB_PATH=<build B>/libjmac_hip.so python tools/aggregate_bits_dump.py --check DIR --digest    # exit 1 on a difference

Graphs (tests/persistent_case.py): the small inline graph and the cooperative schedule without inline entries of
tests/test_gpu_hw_variants.py, and the persistent-grid graph -- every one with five more source rows than destinations, so that a non-zero
self_off is valid.  On each: d = 64, 128, 200, 256, 300, 400; fp32, plain bf16 and (d = 300) padded bf16 tables; the product and
the lanes64 testing entry; slope 0.05 with the loop relation set (self_off 0 and 5) and without it, slope 1.5 (the generic
D4T = 0 kernels) with it.  The jobs entry (two aggregations in one launch) on the small graph, two different table sets, slopes
(0.05, 0.2) and (1.5, 1.5).  Fixed seeds."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "tests")]
import normalize_bits_dump as nbd  # noqa: E402  (Sink, main; puts the repository root on sys.path)
import persistent_case as pc  # noqa: E402
from jmac_amd import _lib, encoder, ops  # noqa: E402
from jmac_amd.graph import RelGraph, _Schedule  # noqa: E402

DEV = "cuda"
DS = (64, 128, 200, 256, 300, 400)
EXTRA = 5                                                     # source rows past the destinations: the non-zero self_off
CALLS = ((0.05, True, 0), (0.05, True, EXTRA), (0.05, False, 0), (1.5, True, 0))      # (slope, loop relation set, self_off)


def build_graph(ei, et, n, nrel, extra, coop=False):
    g = RelGraph(torch.from_numpy(ei).to(DEV), torch.from_numpy(et).to(DEV), n, nrel, num_src=n + extra, **({"chunk": 256} if coop else {}))
    if coop:
        g.by_dst = _Schedule(g.rowptr, n, ei.shape[1], 256, None, coop=True)
        assert g.by_dst.item_edges is None and g.by_dst.n_coop >= 41 and g.by_dst.n_items_max > 16384
    return g


def table_forms(n_src, nrel, d, seed):
    """name -> ([P|Q|Z] of n_src rows, [Rq|Rz], a) on the device"""
    PQZ, RR, a, _ = pc.tables(n_src, nrel, d, seed=seed)
    PQZ, RR, a = PQZ.to(DEV), RR.to(DEV), a.to(DEV)
    forms = {"f32": (PQZ, RR, a), "bf16": (PQZ.to(torch.bfloat16), RR.to(torch.bfloat16), a)}
    if ops.bf16_pad(d) != d:
        forms["bf16-padded"] = (ops.pad_table(forms["bf16"][0], d, 3), ops.pad_table(forms["bf16"][1], d, 2), a)
    return forms


def graph_cases(tag, g, n, nrel, out):
    for d in DS:
        for form, (PQZ, RR, a) in table_forms(n + EXTRA, nrel, d, d).items():
            P, QZ = ops.pqz_views(PQZ)
            for slope, loop, self_off in CALLS:
                for lanes64 in (False, True):
                    res = ops.rel_attn_split_fwd_raw(P[:n], QZ, RR, a, g, slope, pc.OUT_SCALE, nrel - 1 if loop else -1, self_off,
                                                     lanes64=lanes64)
                    what = "%s/d%d-%s-slope%g-loop%d-self%d-%s" % (tag, d, form, slope, loop, self_off, "lanes64" if lanes64 else "product")
                    for name, t in zip(("out", "seg_max", "seg_den"), res):
                        out.put("%s/%s" % (what, name), t[:n])


def jobs_cases(ei, et, n, nrel, out):
    g = build_graph(ei, et, n, nrel, 0)
    assert g.by_dst.item_edges is not None
    for d in DS:
        t0, t1 = table_forms(n, nrel, d, d)["f32"], table_forms(n, nrel, d, d + 1000)["f32"]
        for s0, s1 in ((0.05, 0.2), (1.5, 1.5)):
            pair = encoder._agg_fwd_pair(((t0[0], t0[1], t0[2], s0), (t1[0], t1[1], t1[2], s1)), g)
            for j, res in enumerate(pair):
                for name, t in zip(("out", "seg_max", "seg_den"), res):
                    out.put("jobs/d%d-slopes%g-%g/job%d/%s" % (d, s0, s1, j, name), t[:n])


def cases(out):
    if os.environ.get("JMAC_LIB_PATH"):                       # the testing build beside the library under test
        _lib._HERE = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    tpath = os.path.realpath(_lib.testing_lib()._name)
    assert os.path.dirname(tpath) == os.path.dirname(os.path.realpath(_lib.LIB_PATH)), (tpath, _lib.LIB_PATH)
    print("testing library:", tpath)
    small = pc.small_graph()
    g = build_graph(*small, EXTRA)
    assert g.by_dst.item_edges is not None
    graph_cases("small-inline", g, small[2], small[3], out)
    jobs_cases(*small, out)
    coop = pc.coop_case()[:4]
    graph_cases("cooperative", build_graph(*coop, EXTRA, coop=True), coop[2], coop[3], out)
    big = pc.graph()
    g = build_graph(*big, EXTRA)
    assert g.by_dst.n_items_max > 65536 and g.by_dst.item_edges is None and g.by_dst.n_splits_max > 0
    graph_cases("persistent", g, big[2], big[3], out)


if __name__ == "__main__":
    sys.exit(nbd.main(cases))
