"""What the truncated negative sampler costs next to the filtered one (real DBP-5L ja / el triples of
tests/golden/dbp5l_ja_el_data.npz, B = 1000, K = 25, M = 64; -> profiles/truncated_sampler.json):

  launch    one HIP event pair per launch, both entries in one process taking turns: --rounds rounds of --launches launches after
            5 warm-ups each, medians; jmac_sample_completion_batch against jmac_sample_completion_batch_truncated on the ja
            training triples, the table refreshed from the (untrained) model's normalised completion embeddings, n_hard = K and 0.
  refresh   NeighborTable.refresh at 11 805 x 11 805 x 300, M = 16 and --neighbors, on those embeddings and on independent unit
            rows: plain, screen="bf16" (with the screen's own statistics), and metric="manhattan".
  epochs    host clock around a final synchronise of one train_completion_component epoch on the el + ja pair at dim = 300 with
            capture_completion: "filtered" against "truncated", three epochs in a row each (the first pays warm-up and captures).

    python tools/truncated_sampler_timing.py --out profiles/truncated_sampler.json
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
from jmac_amd.sampling import CompletionSampler, NeighborTable  # noqa: E402

REAL = os.path.join(ROOT, "tests", "golden", "dbp5l_ja_el_data.npz")


def per_launch_us(fn, n, warm=5):
    """Device time of every one of n calls of fn (one event pair each), in microseconds."""
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]


def summary(us):
    return {"median_us": float(np.median(us)), "min_us": float(min(us)), "max_us": float(max(us)), "launches": len(us)}


def setup(a, dev):
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

    def model():
        args = harness.make_args(a.dim, a.batch, a.negatives, dev)
        torch.manual_seed(0)
        m = JMAC(args, name_emb, 2 * nr, n1 + n2).to(dev)
        m.ent_info_att = m.ent_info_att.to(dev)
        return m

    def embeddings(m):
        m.eval()
        with torch.no_grad():
            (_, c1), (_, c2) = m.get_emb_blocks([(g[0], g[1], feed["ent_bases1"], feed["rel_bases1"]),
                                                 (g[2], g[3], feed["ent_bases2"], feed["rel_bases2"])], on_device=True)
        m.train()
        return c1, c2
    return tri1, tri2, n1, n2, g, feed, model, embeddings


def bench_launch(a, dev, tri, num_ent, emb):
    tab = NeighborTable(num_ent, a.neighbors, dev).refresh(emb)
    gen = torch.Generator(device=dev).manual_seed(0)
    launchers, us = {}, {}
    for label, kw in (("filtered", {}), ("truncated", {"neighbors": tab}), ("truncated_n_hard_0", {"neighbors": tab, "n_hard": 0})):
        s = CompletionSampler(tri, num_ent, a.batch, a.negatives, dev, seed=(1, 2), **kw)
        s.new_epoch(gen)

        def launch(s=s):
            s.next_batch()
            s.skip(-1)                                                     # the device wraps to batch 0 by itself: one order throughout
        launchers[label] = launch
    for _ in range(a.rounds):                                              # the three sources take turns: drift hits them alike
        for label, launch in launchers.items():
            us.setdefault(label, []).append(per_launch_us(launch, a.launches))
    out = {label: dict(summary([x for r in rounds for x in r]), round_medians_us=[float(np.median(r)) for r in rounds])
           for label, rounds in us.items()}
    out["truncated_over_filtered"] = out["truncated"]["median_us"] / out["filtered"]["median_us"]
    out["what"] = ("one HIP event pair per next_batch() (both kernels of the entry), %d rounds of %d launches per source in turns, 5 "
                   "warm-ups in front of each; ja training triples, T = %d, num_ent = %d, B = %d, K = %d, M = %d; one batch order "
                   "throughout (the batch number wraps on the device)"
                   % (a.rounds, a.launches, len(tri), num_ent, a.batch, a.negatives, a.neighbors))
    return out


def bench_refresh(a, dev, num_ent, emb):
    """Two inputs of the same shape: "emb", the initialised model's completion embeddings (rows close to one another), and "unit",
    independent normalised Gaussian rows.  The screened form's statistics say how many columns the bf16 bound left per row."""
    from jmac_amd import scoring
    unit = torch.nn.functional.normalize(torch.randn(emb.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5)), dim=1)
    out = {"shape": [num_ent, num_ent, int(emb.shape[1])]}
    for m in sorted({a.neighbors, 16}):
        tab = NeighborTable(num_ent, m, dev)
        for name, x in (("emb", emb), ("unit", unit)):
            row = out.setdefault("m=%d" % m, {}).setdefault(name, {})
            for label, kw in (("inner", {}), ("inner_bf16_screen", {"screen": "bf16"}), ("manhattan", {"metric": "manhattan"})):
                row[label] = summary(per_launch_us(lambda: tab.refresh(x, **kw), 5, warm=2))
            st = scoring.sim_topk(x, x, m, screen="bf16", return_stats=True)[1]
            row["screen_stats"] = {k: v for k, v in st.items() if k != "n_rescored"}
            s = x @ x.T
            row["mean_score"], row["kth_score_mean"] = float(s.mean()), float(s.topk(m, dim=1).values[:, -1].mean())
    return out


def bench_epochs(a, dev, ctx):
    tri1, tri2, n1, n2, g, feed, model, embeddings = ctx
    out = {}
    for label, mode in (("filtered_captured", "filtered"), ("truncated_captured", "truncated")):
        args = harness.make_args(a.dim, a.batch, a.negatives, dev, neg_sampler=mode, capture_completion=True, neg_neighbors=a.neighbors)
        m = model()
        m.train()
        opt = optim.Adam(m.parameters(), lr=1e-3)
        gen = torch.Generator(device=dev).manual_seed(0)
        state = {"embeddings": embeddings(m)} if mode == "truncated" else {}
        walls, losses = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses.append(harness.train_completion_component(m, opt, g[0], g[1], g[2], g[3], feed, tri1, tri2, n1, n2, args, gen,
                                                             state=state))
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        steps = len(tri1) // a.batch + len(tri2) // a.batch
        out[label] = {"epoch_wall_s": walls, "mean_loss": losses, "steps_per_epoch": steps,
                      "ms_per_step_epochs_2_3": [1e3 * w / steps for w in walls[1:]]}
        del m, opt, state
        torch.cuda.empty_cache()
    out["what"] = ("host clock around a final synchronise, train_completion_component on the el (train + val) + ja pair, dim = %d, "
                   "capture_completion, three epochs in a row per mode (the first pays warm-up, the table and the two captures)" % a.dim)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "truncated_sampler.json"))
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--negatives", type=int, default=25)
    ap.add_argument("--neighbors", type=int, default=64)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-epochs", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("truncated_sampler_timing: no HIP device; nothing is timed on a CPU")
    dev = torch.device("cuda")
    ctx = setup(a, dev)
    tri2, n2 = ctx[1], ctx[3]
    emb = ctx[7](ctx[6]())[1].contiguous()                                 # ja: the pair's second KG
    res = {"device": torch.cuda.get_device_name(0), "launch": bench_launch(a, dev, tri2, n2, emb),
           "refresh": bench_refresh(a, dev, n2, emb)}
    if not a.skip_epochs:
        res["epochs"] = bench_epochs(a, dev, ctx)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
