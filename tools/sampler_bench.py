"""What a completion batch costs on the device, and what an epoch costs on the wall clock, per batch source of jmac_amd.harness
(real DBP-5L ja / el triples of tests/golden/dbp5l_ja_el_data.npz, B = 1000, K = 25):

  batches   HIP events around N back-to-back batches after warm-up, per batch: (i) the body of harness.completion_batches plus
            the repeat / cat of train_completion_component (the "uniform" mode), (ii) CompletionSampler.next_batch() (the
            "filtered" mode); both in one process, alternating, the pair repeated --repeats times.
  epochs    host clock around a final synchronise of one train_completion_component epoch on the el + ja pair at dim = 300:
            "uniform" eager, "filtered" eager, "filtered" with capture_completion; three epochs in a row each (the first pays warm-up and the captures).
  --sampler-only   nothing but N next_batch() launches: the process to put under a kernel trace, in a run of its own.
  --merge-trace DB adds the two kernels' durations from that trace's database to the record (needs no GPU).

    python tools/sampler_bench.py --out profiles/sampler_ja.json
    rocprofv3 --kernel-trace --stats -d trace -o sampler -- python tools/sampler_bench.py --sampler-only
    python tools/sampler_bench.py --out profiles/sampler_ja.json --merge-trace trace/sampler_results.db
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jmac_amd import data, harness, optim  # noqa: E402
from jmac_amd.model import JMAC  # noqa: E402
from jmac_amd.sampling import CompletionSampler  # noqa: E402

REAL = os.path.join(ROOT, "tests", "golden", "dbp5l_ja_el_data.npz")
STEP_MS = 1.833          # the ja training step of BENCH_r06.json (hipGraph replay)


def uniform_batches(triples, num_ent, B, K, dev, gen, n):
    """n batches of the "uniform" mode, built exactly as train_completion_component builds them; the last one is returned."""
    done, d = 0, None
    while done < n:
        for tr, neg in harness.completion_batches(triples, num_ent, B, K, dev, gen):
            d = {"batch_h": tr[:, 0].repeat(K + 1), "batch_r": tr[:, 1].repeat(K + 1), "batch_t": torch.cat((tr[:, 2], neg.view(-1)))}
            done += 1
            if done == n:
                break
    return d


def filtered_batches(sampler, gen, n):
    done, d = 0, None
    while done < n:
        sampler.new_epoch(gen)
        for _ in range(min(len(sampler), n - done)):
            d = sampler.next_batch()
            done += 1
    return d


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn(n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n


def bench_batches(a, dev):
    z = data.load_dbp5l_arrays(REAL)
    triples, num_ent = np.asarray(z["ja.train"], dtype=np.int64), int(z["ja.num_entity"])
    gen = torch.Generator(device=dev).manual_seed(0)
    sampler = CompletionSampler(triples, num_ent, a.batch, a.negatives, dev, seed=(1, 2))
    uni = lambda n: uniform_batches(triples, num_ent, a.batch, a.negatives, dev, gen, n)      # noqa: E731
    fil = lambda n: filtered_batches(sampler, gen, n)                                         # noqa: E731
    if a.sampler_only:
        fil(a.batches)
        torch.cuda.synchronize()
        return {"sampler_only_batches": a.batches}
    uni(34), fil(34)                                                       # warm-up: two epochs each
    rows = []
    for _ in range(a.repeats):
        u_dev, u_wall = timed(uni, a.batches)
        f_dev, f_wall = timed(fil, a.batches)
        rows.append({"uniform_ms_per_batch": u_dev, "uniform_wall_ms_per_batch": u_wall,
                     "filtered_ms_per_batch": f_dev, "filtered_wall_ms_per_batch": f_wall})
    u = [r["uniform_ms_per_batch"] for r in rows]
    f = [r["filtered_ms_per_batch"] for r in rows]
    return {"what": "HIP events around %d back-to-back batches of the ja training triples, B = %d, K = %d; the events span the host's "
                    "launch loop, so a source that cannot keep the device busy is charged its launch gaps" % (a.batches, a.batch, a.negatives),
            "pairs": rows, "uniform_ms_per_batch_min_max": [min(u), max(u)], "filtered_ms_per_batch_min_max": [min(f), max(f)],
            "filtered_share_of_ja_step": float(np.median(f)) / STEP_MS, "ja_step_ms": STEP_MS}


def bench_epochs(a, dev):
    z = data.load_dbp5l_arrays(REAL)
    nr = int(z["n_relation_lines"]) + 1
    tri1 = np.concatenate((z["el.train"], z["el.val"])).astype(np.int64)          # supporter: train + val
    tri2 = z["ja.train"].astype(np.int64)
    n1, n2 = int(z["el.num_entity"]), int(z["ja.num_entity"])
    (ei1, et1), (ei2, et2) = data.edges_from_triples(tri1, False), data.edges_from_triples(tri2, False)
    g = [torch.from_numpy(x).to(dev) for x in (ei1, et1, ei2, et2)]
    feed = {"links": torch.from_numpy(z["seed_train_pairs"].astype(np.int64)).to(dev), "ent_bases1": [0, n1], "rel_bases1": [0, nr],
            "ent_bases2": [n1, n1 + n2], "rel_bases2": [nr, 2 * nr]}
    name_emb = np.random.default_rng(1).standard_normal((n1 + n2, 300)).astype(np.float32)
    out = {}
    for label, kw in (("uniform", {}), ("filtered", {"neg_sampler": "filtered"}),
                      ("filtered_captured", {"neg_sampler": "filtered", "capture_completion": True})):
        args = harness.make_args(a.dim, a.batch, a.negatives, dev, **kw)
        torch.manual_seed(0)
        model = JMAC(args, name_emb, 2 * nr, n1 + n2).to(dev)
        model.ent_info_att = model.ent_info_att.to(dev)
        model.train()
        opt = optim.Adam(model.parameters(), lr=1e-3)
        gen = torch.Generator(device=dev).manual_seed(0)
        state, walls, losses = {}, [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses.append(harness.train_completion_component(model, opt, g[0], g[1], g[2], g[3], feed, tri1, tri2, n1, n2, args, gen,
                                                             state=state))
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        out[label] = {"epoch_wall_s": walls, "mean_loss": losses, "steps_per_epoch": len(tri1) // a.batch + len(tri2) // a.batch}
        del model, opt, state
        torch.cuda.empty_cache()
    out["what"] = ("host clock around a final synchronise, train_completion_component on the el (train + val) + ja pair, dim = %d, three "
                   "epochs in a row per mode (the first pays warm-up and, captured, the two captures)" % a.dim)
    return out


def merge_trace(out, db):
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels "
                                       "where name like '%sample_%_kernel%' group by name").fetchall()
    res = json.load(open(out))
    res["kernel_trace"] = {"what": "rocprofv3 --kernel-trace of --sampler-only (a run of its own): durations in us",
                           "kernels": {n.split("::")[-1].split("(")[0]: {"launches": c, "mean_us": a / 1e3, "min_us": lo / 1e3, "max_us": hi / 1e3}
                                       for n, c, a, lo, hi in rows}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_ja.json"))
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--negatives", type=int, default=25)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sampler-only", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--merge-trace", default=None, metavar="DB")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.out, a.merge_trace)
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "batches": bench_batches(a, dev)}
    if not a.sampler_only and not a.skip_epochs:
        res["epochs"] = bench_epochs(a, dev)
    if not a.sampler_only:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
