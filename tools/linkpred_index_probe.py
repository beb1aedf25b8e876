"""Link prediction from the device-resident known-tail index, measured in ONE process (warm-up first, then alternating rounds):
  (a) ranks: `build_filter_csr` + `linkpred_ranks(filt_ptr, filt_idx)` against `linkpred_ranks(index=...)` on the real ja validation
      and test splits, d = 300, two layers of seeded tables;
  (b) top-k: `linkpred_topk` against `linkpred_dist` -> mask the listed entries -> `torch.topk`, k = 10, on the ja validation split in
      one call, on the five-KG union's entity count (56 589) with 16 384 queries, and on N = 2 000 000, B = 1 000 (d = 300, two layers).
"device" is HIP-event time around the launches alone (the CSR form's host loop runs before the first event); "call" is a host clock
from the call to the end of a final synchronise, host work included.  Peak memory is what a call allocates above the tables.
`--kernels-only` runs the top-k launches of the first two sizes (the process to put under `rocprofv3 --kernel-trace --stats`).
Prints a text summary (-> profiles/linkpred_index_timing.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jmac_amd import data, scoring
from jmac_amd.sampling import TrueTailIndex

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def measure(forms, reps, rounds):
    """forms: {name: (host_prologue or None, launch)}; per round and form: device ms per call (events around `launch` only) and
    call ms (host clock around prologue + launch + synchronise), the forms taking turns inside every round."""
    for pro, fn in forms.values():
        for _ in range(2):
            fn(pro() if pro else None)
    torch.cuda.synchronize()
    dev, call = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(rounds):
        for k, (pro, fn) in forms.items():
            d = c = 0.0
            for _ in range(reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arg = pro() if pro else None
                ev[0].record()
                fn(arg)
                ev[1].record()
                torch.cuda.synchronize()
                c += (time.perf_counter() - t0) * 1e3
                d += ev[0].elapsed_time(ev[1])
            dev[k].append(d / reps)
            call[k].append(c / reps)
    return dev, call


def med(v):
    return sorted(v)[len(v) // 2]


def line(name, what, ms):
    return "  %-44s %-6s %s  median %.3f ms  spread %.1f %%" % (name, what, " ".join("%.3f" % m for m in ms), med(ms),
                                                              100.0 * (max(ms) - min(ms)) / min(ms))


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def tables(N, nrel, d, gen):
    return ([torch.randn(N, d, device="cuda", generator=gen) for _ in range(2)],
            [torch.randn(nrel, d, device="cuda", generator=gen) for _ in range(2)])


def materialised_topk(comp, rel, h, r, k, index):
    """The two-step form: the [B, N] matrix, the listed entries set to +inf, torch.topk -- all on the device."""
    dist = scoring.linkpred_dist(comp, rel, h, r)
    code = (h.to(torch.int64) << 32) | r.to(torch.int64)
    pos = torch.searchsorted(index.key_code, code).clamp_(max=len(index.key_code) - 1)
    found = index.key_code[pos] == code
    lo = index.tail_ptr[pos].to(torch.int64)
    n = torch.where(found, index.tail_ptr[pos + 1].to(torch.int64) - lo, torch.zeros_like(lo))
    row = torch.repeat_interleave(torch.arange(len(h), device=h.device), n)
    off = torch.arange(int(n.sum()), device=h.device) - torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
    dist[row, index.tail_idx[lo[row] + off].to(torch.int64)] = float("inf")
    val, idx = torch.topk(dist, k, dim=1, largest=False)
    return idx, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-2m", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1234)
    kgs, _, _, _ = data.kgs_from_arrays(data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz")), "ja")
    ja = kgs["ja"]
    comp, rel = tables(ja.num_entity, ja.num_relation, 300, gen)
    index = TrueTailIndex.from_dict(ja.true_tail, "cuda")
    cases = [("ja validation split, one call", lambda: (comp, rel, index, torch.from_numpy(ja.val_data[:, 0].copy()).cuda(),
                                                         torch.from_numpy(ja.val_data[:, 1].copy()).cuda()), 3)]

    def synthetic(N, B, nrel=200, T=400000):
        g = np.random.default_rng(N)
        tr = np.stack((g.integers(0, N, T), g.integers(0, nrel, T), g.integers(0, N, T)), 1)
        q = tr[g.choice(T, B, replace=False)]
        c, x = tables(N, nrel, 300, gen)
        return c, x, TrueTailIndex.from_triples(tr, "cuda"), torch.from_numpy(q[:, 0].copy()).cuda(), torch.from_numpy(q[:, 1].copy()).cuda()

    if a.kernels_only:
        cases.append(("five-KG union's entity count", lambda: synthetic(56589, 16384), 1))
        for _, make, _ in cases:
            c, x, ix, h, r = make()
            for _ in range(4):
                scoring.linkpred_topk(c, x, h, r, 10, index=ix)
        torch.cuda.synchronize()
        return
    print("device: %s" % torch.cuda.get_device_name(0))
    print("(a) ranks, d = 300, two layers, N = %d; ms per evaluation (%d rounds of 3, alternating):" % (ja.num_entity, a.rounds))
    for split, d_ in (("validation", ja.val_data), ("test", ja.test_data)):
        hl, rl = d_[:, 0].tolist(), d_[:, 1].tolist()
        forms = {"build_filter_csr + linkpred_ranks(fp, fi)": (lambda: scoring.build_filter_csr(hl, rl, ja.true_tail, "cuda"),
                                                              lambda f: scoring.linkpred_ranks(comp, rel, d_[:, 0], d_[:, 1], d_[:, 2], f[0], f[1])),
                 "linkpred_ranks(index=...)": (None, lambda f: scoring.linkpred_ranks(comp, rel, d_[:, 0], d_[:, 1], d_[:, 2], index=index))}
        dev, call = measure(forms, 3, a.rounds)
        print(" ja %s split, %d queries:" % (split, len(d_)))
        for k in forms:
            print(line(k, "device", dev[k]))
            print(line(k, "call", call[k]))
        c0, c1 = list(forms)
        print("  device: indexed - CSR = %+.3f ms (CSR round-to-round spread %.3f ms); call-time ratio CSR / indexed = %.1f"
              % (med(dev[c1]) - med(dev[c0]), max(dev[c0]) - min(dev[c0]), med(call[c0]) / med(call[c1])))
    print("(b) top-k, k = 10, d = 300, two layers; ms per call (%d rounds, alternating):" % a.rounds)
    cases.append(("five-KG union's entity count", lambda: synthetic(56589, 16384), 2))
    if not a.skip_2m:
        cases.append(("N = 2 000 000", lambda: synthetic(2000000, 1000), 1))
    for tag, make, reps in cases:
        c, x, ix, h, r = make()
        forms = {"linkpred_dist + mask + torch.topk": (None, lambda f: materialised_topk(c, x, h, r, 10, ix)),
                 "linkpred_topk(index=...)": (None, lambda f: scoring.linkpred_topk(c, x, h, r, 10, index=ix))}
        peaks = {k: peak_of(lambda: fn(None)) for k, (_, fn) in forms.items()}
        dev, call = measure(forms, reps, a.rounds)
        print(" %s: B = %d, N = %d (B x N x 4 = %.0f MB):" % (tag, len(h), c[0].shape[0], len(h) * c[0].shape[0] * 4 / 2 ** 20))
        for k in forms:
            print(line(k, "device", dev[k]))
            print(line(k, "call", call[k]))
        m0, m1 = list(forms)
        print("  device ratio materialised / fused = %.2f; peak memory above the tables: %.0f MB materialised, %.0f MB fused"
              % (med(dev[m0]) / med(dev[m1]), peaks[m0], peaks[m1]))
        del forms, c, x, ix
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
