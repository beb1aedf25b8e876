"""The stable one-to-one alignment beside the top-k it starts from, in ONE process: forms alternating after warm-up, timed with
device events, five rounds with spreads, at 10 500^2 (bench.py's CSLS shape) and 30 000^2 (BASELINE config 5), d = 300,
csls_k = 10, k = 16, on the same operands and the same precomputed csls_terms:
  top-k alone        scoring.alignment_topk          the many-to-one candidate lists
  stable alignment   scoring.stable_alignment        the same top-k + deferred acceptance + viable refills until nobody is left open
with the run's refills / proposals / unmatched and the peak device memory above the tables (torch.cuda.max_memory_allocated).
At 30 000^2 the stable alignment's peak is ASSERTED to stay within one jmac_sim_csls_topk_workspace_bytes(n1, n2, k) plus
O((n1 + n2) k) bytes of state.
`--kernels-only N` runs six calls of each form at N^2 and nothing else (the process to put under
`rocprofv3 --kernel-trace --stats`: the products against the matching kernels and the torch plumbing between them).
`--noise X`: the second table is the first plus X / sqrt(d) of unit noise per coordinate (default 3.0: Hits@1 well below 1, so
suitors do compete).  Prints a text summary (-> profiles/stable_align_timing.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jmac_amd import _lib, scoring

D, CSLS_K, K = 300, 10, 16


def tables(n, gen, noise):
    b = torch.nn.functional.normalize(torch.randn(n, D, device="cuda", generator=gen) + 0.3 * torch.randn(1, D, device="cuda", generator=gen), dim=1)
    a = torch.nn.functional.normalize(b + noise * torch.randn(n, D, device="cuda", generator=gen) / D ** 0.5, dim=1)
    return a, b


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def alternate(forms, reps, rounds):
    for fn in forms.values():                                   # warm-up: allocator, occupancy queries, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            out[k].append(timed(fn, reps))
    return out


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def line(name, ms):
    return "  %-20s %s  median %.3f ms  spread %.1f %%" % (name, " ".join("%.3f" % m for m in ms), sorted(ms)[len(ms) // 2],
                                                         100.0 * (max(ms) - min(ms)) / min(ms))


def forms_of(a, b, terms):
    # metric="inner" on unit rows: the tables ARE the operands
    return {"top-k alone": lambda: scoring.alignment_topk(a, b, K, CSLS_K, "inner", terms=terms),
            "stable alignment": lambda: scoring.stable_alignment(a, b, K, CSLS_K, "inner", terms=terms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--noise", type=float, default=3.0)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10500, 30000])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    if a.kernels_only:
        e1, e2 = tables(a.kernels_only, gen, a.noise)
        terms = scoring.csls_terms(e1, e2, CSLS_K)
        for fn in forms_of(e1, e2, terms).values():
            for _ in range(6):
                fn()
        torch.cuda.synchronize()
        return
    print("device: %s" % torch.cuda.get_device_name(0))
    L = _lib.lib()
    for n in a.sizes:
        e1, e2 = tables(n, gen, a.noise)
        terms = scoring.csls_terms(e1, e2, CSLS_K)
        ws = int(L.jmac_sim_csls_topk_workspace_bytes(n, n, K))
        print("n1 = n2 = %d, d = %d, csls_k = %d, k = %d, noise %.1f (top-k workspace %.1f MB, one stored matrix %.1f MB):"
              % (n, D, CSLS_K, K, a.noise, ws / 2 ** 20, n * n * 4 / 2 ** 20))
        fs = forms_of(e1, e2, terms)
        peaks = {}
        for k, fn in fs.items():
            peaks[k], out = peak_of(fn)
            if k == "stable alignment":
                m1, _, stats = out
                hits = float((m1 == torch.arange(n, device="cuda")).float().mean())
                top1 = float((scoring.alignment_topk(e1, e2, 1, CSLS_K, "inner", terms=terms)[0][:, 0] == torch.arange(n, device="cuda")).float().mean())
                print("  stats: %s; match1[i] == i for %.2f %% of the suitors (greedy top-1: %.2f %%)" % (stats, 100 * hits, 100 * top1))
            del out
        reps = 5 if n <= 12000 else 2
        r = alternate(fs, reps, a.rounds)
        print(" ms per call (%d rounds of %d, alternating):" % (a.rounds, reps))
        for k, ms in r.items():
            print(line(k, ms))
        m = {k: sorted(v)[len(v) // 2] for k, v in r.items()}
        print("  stable alignment / top-k alone = %.2f; peak device memory above the tables: %.1f MB top-k alone, %.1f MB stable alignment"
              % (m["stable alignment"] / m["top-k alone"], peaks["top-k alone"] / 2 ** 20, peaks["stable alignment"] / 2 ** 20))
        if n == 30000:
            # lists (int32 + fp32) and a refill's new lists, k each; the int64 result and the O(n) state vectors
            state = 2 * n * (K * 16 + 128)
            assert peaks["stable alignment"] <= ws + state, (peaks["stable alignment"], ws, state)
            print("  asserted: stable alignment peak %.1f MB <= one top-k workspace %.1f MB + %.1f MB of O((n1 + n2) k) state"
                  % (peaks["stable alignment"] / 2 ** 20, ws / 2 ** 20, state / 2 ** 20))
        del e1, e2, terms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
