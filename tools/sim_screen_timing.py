"""jmac_sim_topk_f32 against jmac_sim_topk_screened_f32 on the same tensors (-> profiles/sim_screen_timing.txt).

Shapes (k = 25): 3000 x 30000 x 300 (config 5's get_neg) and 2264 x 13996 x 256 (ja-en), each on two inputs:
    unit    unit-norm random rows, the queries a random subset of the table's rows (bench.py's get_neg operands)
    emb     get_emb rows of a freshly initialised JMAC model on a power-law graph of that many entities, same query choice
Per case, in ONE process: both entries are asserted to return the same indices and values bit for bit; then, after 5 warm-up calls
each, `rounds` rounds in which the two entries take turns, device events around `reps` back-to-back calls.  "spread" is (max - min)
/ min over a form's rounds; the screened entry counts as faster only if its slowest round beats the fp32 entry's fastest.  The list
statistics (columns rescored per row, rows that overflowed) come from the entry's n_rescored output.  Per-stage device times:
the kernels of 10 further calls of each entry under torch.profiler, in a pass of its own after the timed rounds (its own clock;
only the split between the stages is read from it).  Each case runs in a child process under a time limit; the parent stops at
the first child that fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 25
CASES = [(3000, 30000, 300, "unit"), (3000, 30000, 300, "emb"), (2264, 13996, 256, "unit"), (2264, 13996, 256, "emb")]
STAGES = [("screen_prepare_kernel", "prepare (bf16 copies, norms)"), ("screen_gemm_kernel<false", "sample product (bf16)"),
          ("row_topk_kernel", "sample row top-k"), ("screen_gemm_kernel<true", "filter product (bf16)"),
          ("screen_select_kernel", "prune + rescore + select"), ("sim_gemm_kernel", "fp32 product (sample + filter)"),
          ("cand_select_kernel", "fp32 entry's select")]


def med(v):
    return sorted(v)[len(v) // 2]


def operands(L, N, d, kind):
    import numpy as np
    import torch
    gen = torch.Generator(device="cuda").manual_seed(L + N)
    if kind == "unit":
        tab = torch.nn.functional.normalize(torch.randn(N, d, device="cuda", generator=gen))
    else:
        from jmac_amd import harness, synth
        from jmac_amd.model import JMAC
        torch.manual_seed(0)
        nr = 400
        ei, et = synth.power_law_graph(N, 8 * N, nr, seed=7)[:2]
        args = harness.make_args(dim=d, dropout=0.0)
        name_emb = np.random.default_rng(0).standard_normal((N, 300)).astype(np.float32)
        model = JMAC(args, name_emb, nr, N).cuda().eval()
        ei, et = torch.as_tensor(np.asarray(ei), device="cuda"), torch.as_tensor(np.asarray(et), device="cuda")
        with torch.no_grad():
            (tab, _), = model.get_emb_blocks([(ei, et, [0, N], [0, nr])], on_device=True)
        tab = tab.contiguous()
        del model
    q = tab[torch.randperm(N, device="cuda", generator=gen)[:L]].contiguous()
    return q, tab


def stage_times(fn, calls=10):
    """{kernel name: (device us per call, launches per call)} of `calls` calls of fn under torch.profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if t > 0:
            out[ev.key] = (t / calls, ev.count / calls)
    return out


def run_case(L, N, d, kind, reps, rounds):
    import torch
    from jmac_amd import scoring
    q, tab = operands(L, N, d, kind)
    fp32 = lambda: scoring.sim_topk(q, tab, K, return_values=True)                     # noqa: E731
    scr = lambda: scoring.sim_topk(q, tab, K, return_values=True, screen="bf16")       # noqa: E731
    idx0, val0 = fp32()
    idx1, val1, st = scoring.sim_topk(q, tab, K, return_values=True, screen="bf16", return_stats=True)
    assert torch.equal(idx0, idx1) and torch.equal(val0.view(torch.int32), val1.view(torch.int32)), "the screened entry differs"
    print("%d x %d x %d, k = %d, %s rows: indices and values identical; rescored columns per row mean %.1f max %d, overflow rows %d of %d"
          % (L, N, d, K, kind, st["rescored_mean"], st["rescored_max"], st["overflow_rows"], L))
    forms = {"jmac_sim_topk_f32": fp32, "jmac_sim_topk_screened_f32": scr}
    for fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    for k, v in ms.items():
        print("  %-28s %s  median %.3f ms  spread %.1f %%" % (k, " ".join("%.3f" % x for x in v), med(v), 100.0 * (max(v) - min(v)) / min(v)))
    a, b = ms["jmac_sim_topk_f32"], ms["jmac_sim_topk_screened_f32"]
    print("  fp32 / screened (medians) %.2f; slowest screened round %.3f ms against fastest fp32 round %.3f ms: %s"
          % (med(a) / med(b), max(b), min(a), "faster beyond the spread" if max(b) < min(a) else "NOT faster beyond the spread"))
    for name, fn in forms.items():
        try:
            kt = stage_times(fn)
        except Exception as e:                 # the profiler is optional: the event timings above stand without it
            print("  (no per-stage times for %s: %r)" % (name, e))
            continue
        total = sum(t for t, _ in kt.values())
        print("  %s, kernels under the profiler, us per call (total %.0f):" % (name, total))
        for key, (t, n) in sorted(kt.items(), key=lambda kv: -kv[1][0]):
            label = next((lab for pat, lab in STAGES if pat in key.replace(" ", "")), "")
            print("    %8.1f us  %4.1f launches  %-34s %s" % (t, n, label, key[:110]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=4, default=None, metavar=("L", "N", "d", "KIND"), help="run one case in this process")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=200, help="seconds per case")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if a.case is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("sim_screen_timing: no HIP device; nothing is timed on a CPU")
        run_case(int(a.case[0]), int(a.case[1]), int(a.case[2]), a.case[3], a.reps, a.rounds)
        return
    for c in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case"] + [str(v) for v in c] + ["--reps", str(a.reps), "--rounds", str(a.rounds)]
        res = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if a.out:
            with open(a.out, "a") as f:
                f.write(res.stdout)
        if res.returncode != 0:
            sys.exit("sim_screen_timing: case %s ended with status %d; stopping" % (c, res.returncode))


if __name__ == "__main__":
    main()
