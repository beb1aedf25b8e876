"""The EnTr refresh's scoring, materialised against matrix-free, in ONE process: `alignment_quality` + the two `max` calls of
its consumer (entr.py) against `alignment_stats`, alternating after warm-up, timed with device events, on
  (a) the real el + ja pair's shape: N1 = 5 231, N2 = 11 805, 1 112 listed each, seeded unit rows, d = 300;
  (b) BASELINE config 5: N1 = N2 = 30 000, 3 000 listed;
  (c) everything listed: n1 = n2 = N = 12 000 (no flop advantage: only the epilogue and the missing matrix traffic differ);
and the statistics launch against the plain jmac_sim_matrix_f32 launch on (c)'s product: the epilogue's cost as a ratio.
`--kernels-only` runs just those two launches (the process to put under `rocprofv3 --kernel-trace --stats`).
Prints a text summary (-> profiles/align_stats_timing.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jmac_amd import scoring


def unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, device="cuda", generator=gen), dim=1)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def alternate(forms, reps, rounds):
    """forms: {name: fn}; returns {name: [ms per call, one figure per round]}, the forms taking turns inside every round."""
    for fn in forms.values():                                   # warm-up: allocator, occupancy queries, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            out[k].append(timed(fn, reps))
    return out


def line(name, ms):
    return "  %-34s %s  median %.3f ms  spread %.1f %%" % (name, " ".join("%.3f" % m for m in ms), sorted(ms)[len(ms) // 2],
                                                         100.0 * (max(ms) - min(ms)) / min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    tab = unit(24000, 300, gen)
    A, B = tab[:12000], tab[12000:]
    out = torch.empty((12000, 12000), device="cuda")
    kern = {"jmac_sim_matrix_f32 (stores S)": lambda: scoring.sim_matrix(A, B, out=out),
            "jmac_sim_softmax_stats_f32": lambda: scoring.sim_softmax_stats(A, B),
            "jmac_sim_softmax_stats_f32 rows": lambda: scoring.sim_softmax_stats(A, B, cols=False)}
    if a.kernels_only:
        for fn in kern.values():
            for _ in range(12):
                fn()
        torch.cuda.synchronize()
        return
    print("device: %s" % torch.cuda.get_device_name(0))
    print("12 000 x 12 000 x 300 product, ms per launch (%d rounds of 10, alternating):" % a.rounds)
    r = alternate(kern, 10, a.rounds)
    for k, ms in r.items():
        print(line(k, ms))
    med = {k: sorted(v)[len(v) // 2] for k, v in r.items()}
    print("  epilogue cost: stats / stored = %.3f, rows only / stored = %.3f" % (
        med["jmac_sim_softmax_stats_f32"] / med["jmac_sim_matrix_f32 (stores S)"],
        med["jmac_sim_softmax_stats_f32 rows"] / med["jmac_sim_matrix_f32 (stores S)"]))
    for tag, N1, N2, n in (("(a) el + ja pair", 5231, 11805, 1112), ("(b) config 5", 30000, 30000, 3000), ("(c) all listed", 12000, 12000, 12000)):
        e1, e2 = unit(N1, 300, gen), unit(N2, 300, gen)
        l1 = torch.randperm(N1, generator=torch.Generator().manual_seed(1))[:n].tolist()
        l2 = torch.randperm(N2, generator=torch.Generator().manual_seed(2))[:n].tolist()

        def stored():
            H, simi, _ = scoring.alignment_quality(e1, e2, l1, l2)
            v = simi.max(dim=1)[0]
            return H, v, simi[:64].max(dim=1)[1]

        def free():
            return scoring.alignment_stats(e1, e2, l1, l2)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        stored()
        torch.cuda.synchronize()
        peak_s = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        free()
        torch.cuda.synchronize()
        peak_f = torch.cuda.max_memory_allocated() - base
        reps = 3 if N1 * N2 > 2e8 else 10
        r = alternate({"alignment_quality + max, max": stored, "alignment_stats": free}, reps, a.rounds)
        print("%s: N1 = %d, N2 = %d, %d listed; ms per refresh scoring (%d rounds of %d, alternating), host list handling included:"
              % (tag, N1, N2, n, a.rounds, reps))
        for k, ms in r.items():
            print(line(k, ms))
        m = {k: sorted(v)[len(v) // 2] for k, v in r.items()}
        print("  ratio stored / matrix-free = %.2f; peak device memory above the tables: %.1f MB stored, %.1f MB matrix-free"
              % (m["alignment_quality + max, max"] / m["alignment_stats"], peak_s / 2 ** 20, peak_f / 2 ** 20))
        del e1, e2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
