"""Alignment evaluation and inference, stored against matrix-free, in ONE process: forms alternating after warm-up, timed with device
events, five rounds with spreads, at 10 500^2 (bench.py's CSLS shape), 30 000^2 (BASELINE config 5) and 60 000^2, all at d = 300,
csls_k = 10, k = 10 for the top-k:
  evaluator     scoring.alignment_test()                 against  alignment_test(matrix_free=True)
  predictions   csls_sim(sim_matrix) + row_topk           against  alignment_topk (its csls_terms included)
with the peak device memory above the tables (torch.cuda.max_memory_allocated).  A stored form whose matrices do not fit the
device is reported as such and skipped.  At 30 000^2 the matrix-free evaluator's peak is ASSERTED to stay within the larger of the
two sim_topk workspaces (they are used one after the other) plus O(n1 + n2) vectors.
`--kernels-only N` runs twelve calls of each form at N^2 and nothing else (the process to put under
`rocprofv3 --kernel-trace --stats`: which of the three products carries a difference).
Prints a text summary (-> profiles/align_eval_timing.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jmac_amd import _lib, scoring

D, CSLS_K, K = 300, 10, 10


def tables(n, gen):
    """Two unit-row tables, row i of the second a noisy copy of row i of the first (an evaluation whose ranks are not all 1)."""
    b = torch.nn.functional.normalize(torch.randn(n, D, device="cuda", generator=gen) + 0.3 * torch.randn(1, D, device="cuda", generator=gen), dim=1)
    a = torch.nn.functional.normalize(b + 3.0 * torch.randn(n, D, device="cuda", generator=gen) / D ** 0.5, dim=1)
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
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def line(name, ms):
    return "  %-44s %s  median %.3f ms  spread %.1f %%" % (name, " ".join("%.3f" % m for m in ms), sorted(ms)[len(ms) // 2],
                                                         100.0 * (max(ms) - min(ms)) / min(ms))


def forms_of(a, b):
    # metric="inner" on unit rows: the tables ARE the operands (the cosine form would time two row_normalize copies in both)
    return {
        "evaluator": {"stored": lambda: scoring.alignment_test(a, b, metric="inner", csls_k=CSLS_K),
                      "matrix-free": lambda: scoring.alignment_test(a, b, metric="inner", csls_k=CSLS_K, matrix_free=True)},
        "predictions": {"stored": lambda: scoring.row_topk(scoring.csls_sim(scoring.sim_matrix(a, b), CSLS_K), K),
                        "matrix-free": lambda: scoring.alignment_topk(a, b, K, CSLS_K, "inner")},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10500, 30000, 60000])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    if a.kernels_only:
        e1, e2 = tables(a.kernels_only, gen)
        for fs in forms_of(e1, e2).values():
            for fn in fs.values():
                for _ in range(12):
                    fn()
        torch.cuda.synchronize()
        return
    print("device: %s" % torch.cuda.get_device_name(0))
    free_b, _ = torch.cuda.mem_get_info()
    L = _lib.lib()
    for n in a.sizes:
        e1, e2 = tables(n, gen)
        ws = max(int(L.jmac_sim_topk_workspace_bytes(n, n, CSLS_K)), int(L.jmac_sim_csls_topk_workspace_bytes(n, n, K)))
        print("n1 = n2 = %d, d = %d, csls_k = %d, top-k k = %d (sim_topk workspace %.1f MB, one stored matrix %.1f MB):"
              % (n, D, CSLS_K, K, ws / 2 ** 20, n * n * 4 / 2 ** 20))
        reps = 10 if n <= 12000 else 3
        for what, fs in forms_of(e1, e2).items():
            need = (2 if what == "predictions" else 1) * n * n * 4 + 3 * ws          # stored: S (+ the rescored copy) + column pass scratch
            if need > 0.9 * free_b:
                fs = {k: v for k, v in fs.items() if k != "stored"}
                print("  %s: the stored form needs ~%.1f GB here and is skipped" % (what, need / 2 ** 30))
            peaks = {k: peak_of(fn) for k, fn in fs.items()}
            r = alternate(fs, reps, a.rounds)
            print(" %s, ms per call (%d rounds of %d, alternating):" % (what, a.rounds, reps))
            for k, ms in r.items():
                print(line(k, ms))
            m = {k: sorted(v)[len(v) // 2] for k, v in r.items()}
            if "stored" in m:
                print("  ratio stored / matrix-free = %.2f; peak device memory above the tables: %.1f MB stored, %.1f MB matrix-free"
                      % (m["stored"] / m["matrix-free"], peaks["stored"] / 2 ** 20, peaks["matrix-free"] / 2 ** 20))
            else:
                print("  peak device memory above the tables: %.1f MB matrix-free" % (peaks["matrix-free"] / 2 ** 20))
            if what == "evaluator" and n == 30000:
                # sim_topk's outputs next to its workspace: idx int32 + its int64 copy + values, k each; then the O(n) vectors
                vectors = 2 * n * (CSLS_K * 16 + 64)
                assert peaks["matrix-free"] <= ws + vectors, (peaks["matrix-free"], ws, vectors)
                print("  asserted: matrix-free evaluator peak %.1f MB <= one sim_topk workspace %.1f MB + %.1f MB of O(n) vectors"
                      % (peaks["matrix-free"] / 2 ** 20, ws / 2 ** 20, vectors / 2 ** 20))
        del e1, e2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
