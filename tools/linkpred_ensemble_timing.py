"""Cross-KG ensemble link prediction on the whole ja validation split (8 633 queries, N = 11 805, d = 300, two layers of seeded
tables per KG, seed links of the five-KG fixture), measured in ONE process -- warm-up first, then alternating rounds:
  single     scoring.linkpred_ranks(index=...) on ja alone: the baseline the (S + 1) x expectation is stated against
  S = 1, 2   scoring.linkpred_ranks_ensemble with el, and with el + en, as supporting KGs
  assembled  the same ranks from the public pieces: linkpred_dist per member ([B, N_s] matrices), a column gather through the
             link, where(present, d_s, d_0), the weighted sum, filtered_rank (its CSR is built outside the timed window)
  dense      S = 1 with a synthetic support of N rows and EVERY row linked, so that no tile is skipped: by the identity (the
             support's rows are read in order) and by a random permutation (every 1 200-byte row gathered from elsewhere) --
             the first against 2 x single is the ensemble kernel's own overhead, the second against the first the gathered reads
"device" is HIP-event time around a window of --reps calls, per call; peak memory is what one call allocates above the tables.
The ranks of the ensemble and of the assembled form are compared (they differ only where fp32 rounding decides: the assembled
form rounds per layer and sums the members in a different order).  Also prints the share of (query tile, candidate tile,
supporting member) triples whose slabs the tile kernel skips.
Prints a text summary (-> profiles/linkpred_ensemble_timing.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jmac_amd import data, scoring

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
TILE = 64


def load(supports):
    """(kgs, {support: link map of ja's rows, numpy})"""
    kgs, s_train, _, _ = data.kgs_from_arrays(data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_all_data.npz")), "ja")
    links = {}
    for s in supports:
        pairs = s_train[("ja", s)] if ("ja", s) in s_train else s_train[(s, "ja")][:, ::-1]
        links[s] = scoring.link_map(pairs, kgs["ja"].num_entity, kgs[s].num_entity).numpy()
    return kgs, links


def skipped_share(h, links, N):
    """Share of (query tile, candidate tile, supporting member) triples without a linked head or without a linked candidate."""
    skipped = total = 0
    for link in links:
        q = np.array([(link[h[i:i + TILE]] >= 0).any() for i in range(0, len(h), TILE)])
        c = np.array([(link[i:i + TILE] >= 0).any() for i in range(0, N, TILE)])
        run = np.outer(q, c)
        skipped += run.size - int(run.sum())
        total += run.size
    return skipped / max(total, 1)


def measure(forms, reps, rounds):
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    dev = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            dev[k].append(ev[0].elapsed_time(ev[1]) / reps)
    return dev


def peak_of(fn):
    """MB a call allocates above what is resident"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def med(v):
    return sorted(v)[len(v) // 2]


def assembled(members, h, r, gold, fp, fi):
    comp0, rel0, _, w0 = members[0]
    d0 = scoring.linkpred_dist(comp0, rel0, h, r)
    total = w0 * d0
    for comp, rel, link, w in members[1:]:
        lh = link[h.long()].long()
        ds = scoring.linkpred_dist(comp, rel, lh.clamp(min=0), r)[:, link.long().clamp(min=0)]
        present = (lh >= 0)[:, None] & (link >= 0)[None, :]
        total = total + w * torch.where(present, ds, d0)
    return scoring.filtered_rank(total, gold, fp, fi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--kernels-only", action="store_true", help="the ensemble launches alone (the process to put under a profiler)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from jmac_amd.sampling import TrueTailIndex
    supports = ["el", "en"]
    kgs, links = load(supports)
    ja = kgs["ja"]
    N, d = ja.num_entity, 300
    gen = torch.Generator(device="cuda").manual_seed(1234)
    tabs = {l: ([torch.randn(kgs[l].num_entity, d, device="cuda", generator=gen) for _ in range(2)],
                [torch.randn(ja.num_relation, d, device="cuda", generator=gen) for _ in range(2)]) for l in ["ja"] + supports}
    val = ja.val_data
    h, r, t = (torch.from_numpy(val[:, c].copy()).cuda() for c in range(3))
    index = TrueTailIndex.from_dict(ja.true_tail, "cuda")
    dlinks = {s: torch.from_numpy(links[s]).cuda() for s in supports}
    weights = {1: (0.5, 0.5), 2: (0.5, 0.3, 0.2)}

    def members(S):
        return [(tabs["ja"][0], tabs["ja"][1], None, weights[S][0])] + \
               [(tabs[s][0], tabs[s][1], dlinks[s], w) for s, w in zip(supports[:S], weights[S][1:])]

    forms = {"single-KG linkpred_ranks": lambda: scoring.linkpred_ranks(tabs["ja"][0], tabs["ja"][1], h, r, t, index=index)}
    for S in (1, 2):
        forms["ensemble S = %d" % S] = lambda m=members(S): scoring.linkpred_ranks_ensemble(m, h, r, t, index=index)
    dense = ([torch.randn(N, d, device="cuda", generator=gen) for _ in range(2)], tabs["el"][1])
    for tag, lk in (("identity", torch.arange(N, dtype=torch.int32, device="cuda")),
                    ("permuted", torch.randperm(N, device="cuda", generator=gen).to(torch.int32))):
        m = [members(1)[0], (dense[0], dense[1], lk, 0.5)]
        forms["dense S = 1, %s links" % tag] = lambda m=m: scoring.linkpred_ranks_ensemble(m, h, r, t, index=index)
    if a.kernels_only:
        for _ in range(4):
            for k, fn in forms.items():
                fn()
        torch.cuda.synchronize()
        return
    fp, fi = scoring.build_filter_csr(val[:, 0].tolist(), val[:, 1].tolist(), ja.true_tail, "cuda")
    for S in (1, 2):
        forms["assembled S = %d" % S] = lambda m=members(S): assembled(m, h, r, t, fp, fi)
    print("device: %s" % torch.cuda.get_device_name(0))
    print("ja validation split: B = %d, N = %d, d = %d, two layers; supports %s" %
          (len(val), N, d, ", ".join("%s (%d rows, %d linked)" % (s, kgs[s].num_entity, (links[s] >= 0).sum()) for s in supports)))
    dev = measure(forms, a.reps, a.rounds)
    peak = {k: peak_of(fn) for k, fn in forms.items()}
    base = med(dev["single-KG linkpred_ranks"])
    for k in forms:
        print("  %-28s %s  median %.3f ms  spread %.1f %%  peak memory above the tables %.0f MB" %
              (k, " ".join("%.3f" % m for m in dev[k]), med(dev[k]), 100.0 * (max(dev[k]) - min(dev[k])) / min(dev[k]), peak[k]))
    di, dp = med(dev["dense S = 1, identity links"]), med(dev["dense S = 1, permuted links"])
    print("dense S = 1 (no tile skipped): identity links %.3f ms = %.2f x (2 x single); permuted links %.3f ms = %.2f x identity" %
          (di, di / (2 * base), dp, dp / di))
    for S in (1, 2):
        e, m = med(dev["ensemble S = %d" % S]), med(dev["assembled S = %d" % S])
        ls = [links[s] for s in supports[:S]]
        rk_e = forms["ensemble S = %d" % S]()
        rk_a = forms["assembled S = %d" % S]()
        print("S = %d: ensemble %.3f ms = %.2f x single; ratio to (S + 1) x single = %.2f; assembled / ensemble = %.2f; member-slabs "
              "skipped %.1f %%; ranks differing from the assembled form: %d of %d" %
              (S, e, e / base, e / ((S + 1) * base), m / e, 100.0 * skipped_share(val[:, 0], ls, N),
               int((rk_e != rk_a).sum()), len(val)))


if __name__ == "__main__":
    main()
