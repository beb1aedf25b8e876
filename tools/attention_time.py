"""Attention export (ops.rel_attn_edge_weights) beside the forward aggregation (ops.rel_attn_aggregate) on the same graph and
tables in the same run, d = 300:

    python tools/attention_time.py [--scale S] [--runs R] [--skip-synth]

Graphs: the real DBP-5L ja train graph (tests/golden/dbp5l_ja_el_data.npz) and config 4 (power-law, 1M entities / 20M triples /
1k relations) scaled by S (default 1.0).  fp32 tables and bf16 tables in the padded layout.  Every figure is the median of R
(default 30) device-event timings of one call after 5 warm-up calls; the two ops alternate, so a drift of the clock hits both.
Bytes: the export's bound E (d s + 12 + 4) + N (d s + 4) ('Attention export'), the forward's
synth.fwd_algorithmic_bytes.  Run it under `timeout`."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from jmac_amd import ops, synth
from jmac_amd.graph import RelGraph

D, SLOPE = 300, 0.05


def export_bytes(n, e, d, elem, logits=False):
    return e * (d * elem + 12 + 4 + (4 if logits else 0)) + n * (d * elem + 4)


def one_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(name, ei, et, n, nrel, runs):
    dev = torch.device("cuda")
    g = RelGraph(torch.from_numpy(ei).to(dev), torch.from_numpy(et).to(dev), n, nrel)
    e = g.E
    gen = torch.Generator(device=dev).manual_seed(0)
    PQZ = torch.randn(n, 3 * D, device=dev, generator=gen) * 0.3
    RR = torch.randn(nrel, 2 * D, device=dev, generator=gen) * 0.3
    a = torch.randn(D, device=dev, generator=gen) * 0.1
    print("%s: N=%d E=%d relations=%d chunk=%d items=%d" % (name, n, e, nrel, g._chunk_dst, g.by_dst.n_items_max), flush=True)
    for kind, elem in (("fp32", 4), ("bf16", 2)):
        if kind == "bf16":
            T, R = ops.pad_table(PQZ.to(torch.bfloat16), D, 3), ops.pad_table(RR.to(torch.bfloat16), D, 2)
        else:
            T, R = PQZ, RR
        P, QZ = ops.pqz_views(T)
        calls = {
            "forward": lambda: ops.rel_attn_aggregate(T, R, a, g, SLOPE, loop_rel=-1, out_scale=1.0),
            "export": lambda: ops.rel_attn_edge_weights(P, QZ, R, a, g, SLOPE),
            "export+logits+stats": lambda: ops.rel_attn_edge_weights(P, QZ, R, a, g, SLOPE, logits=True, stats=True),
        }
        times = {k: [] for k in calls}
        with torch.no_grad():
            for _ in range(5):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(runs):
                for k, fn in calls.items():
                    times[k].append(one_ms(fn))
        nbytes = {"forward": synth.fwd_algorithmic_bytes(n, e, D, elem), "export": export_bytes(n, e, D, elem),
                  "export+logits+stats": export_bytes(n, e, D, elem, True) + 8 * n}
        fwd = statistics.median(times["forward"])
        for k in calls:
            ms = statistics.median(times[k])
            print("  %-4s %-20s median %9.4f ms (min %9.4f)  %7.1f GB/s of its byte bound  %.2f x forward"
                  % (kind, k, ms, min(times[k]), nbytes[k] / ms / 1e6, ms / fwd), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--skip-synth", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_time.py measures on an MI355X: no HIP device here")
    from jmac_amd.data import edges_from_triples, load_dbp5l_arrays
    z = load_dbp5l_arrays(os.path.join(ROOT, "tests", "golden", "dbp5l_ja_el_data.npz"))
    ei, et = edges_from_triples(z["ja.train"], False)
    measure("DBP-5L ja train", ei, et, int(z["ja.num_entity"]), int(z["n_relation_lines"]) + 2, max(args.runs, 20))
    if not args.skip_synth:
        n, e = int(1_000_000 * args.scale), int(20_000_000 * args.scale)
        ei, et, n, nrel = synth.power_law_graph(n, e, 1000, seed=1234)
        measure("config 4 x %.2f" % args.scale, ei, et, n, nrel, max(args.runs, 20))


if __name__ == "__main__":
    main()
