"""The screened alignment top-k against the fp32 entries on the same tensors (-> profiles/align_screen_timing.txt).

Cases, each in ONE child process of its own (the parent stops at the first child that fails):
    topk L N d        scoring.alignment_topk, csls_k = 10, k = 16, the terms computed once beforehand: jmac_sim_csls_topk_f32 against
                      jmac_sim_csls_topk_screened_f32 (3000 x 30000 x 300 and 13996 x 13996 x 256); then the whole call, csls_terms'
                      two products included.  Per-stage device times from 10 further calls under torch.profiler.
    refill R N d      the stable matching's refill: jmac_sim_csls_topk_viable_f32 against its screened form for R gathered rows of a
                      3000-row instance at the config-5 width (30000 x 300), R = 1, 32, 256, 2048.  The reviewers' words are
                      those of the run after its first fixpoint on the initial lists; the rows are its exhausted suitors first.
    stable / auction  one scoring.stable_alignment / auction_alignment end to end at 13996 x 13996 x 256, screen=None against "bf16"
Operands: unit-norm random rows; the queries are noisy copies of a random subset of the table's rows (cosine to their source about
0.3, the level of the best of 14 000 random rows), so that the matching has something to decide.  In every case both forms are
asserted to return the same bits first; then, after warm-up calls, `rounds` rounds in which the two forms take turns, device
events around `reps` back-to-back calls (one call for the end-to-end runs, which read the host).  "spread" is (max - min) / min
over a form's rounds; the screened form counts as faster only if its slowest round beats the fp32 form's fastest."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sim_screen_timing import med, stage_times  # noqa: E402

K, CSLS_K = 16, 10
CASES = [("topk", 3000, 30000, 300), ("topk", 13996, 13996, 256),
         ("refill", 1, 30000, 300), ("refill", 32, 30000, 300), ("refill", 256, 30000, 300), ("refill", 2048, 30000, 300),
         ("stable", 13996, 13996, 256), ("auction", 13996, 13996, 256)]
STAGES = [("screen_prepare_kernel", "prepare (bf16 copies, norms)"), ("screen_gemm_kernel<false", "sample product (bf16)"),
          ("screen_sample_align_kernel", "sample -> c_lo"), ("row_topk_kernel", "sample row top-k"),
          ("screen_gemm_kernel<true", "filter product (bf16)"), ("screen_select_kernel", "prune + rescore + select"),
          ("screen_overflow_kernel", "overflowing rows"), ("sim_gemm_kernel", "fp32 product (sample + filter)"),
          ("csls_inplace_kernel", "fp32 entry: sample -> c"), ("viable_inplace_kernel", "fp32 entry: sample -> c, masked"),
          ("cand_select", "fp32 entry's select")]


def operands(L, N, d):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(L + N)
    tab = torch.nn.functional.normalize(torch.randn(N, d, device="cuda", generator=gen))
    src = tab[torch.randperm(N, device="cuda", generator=gen)[:L]]
    noise = torch.nn.functional.normalize(torch.randn(L, d, device="cuda", generator=gen))
    return torch.nn.functional.normalize(src + 3.0 * noise).contiguous(), tab


def same(x, y):
    import torch
    return all(torch.equal(p, q) if p.dtype != torch.float32 else torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x, y))


def rounds_of(forms, reps, rounds, warm=5):
    """{name: [ms per call of every round]}: the forms take turns, device events around `reps` back-to-back calls"""
    import torch
    for fn in forms.values():
        for _ in range(warm):
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
    return ms


def report(ms, fp32, scr):
    for k, v in ms.items():
        print("  %-42s %s  median %.3f ms  spread %.1f %%" % (k, " ".join("%.3f" % x for x in v), med(v), 100.0 * (max(v) - min(v)) / min(v)))
    a, b = ms[fp32], ms[scr]
    print("  fp32 / screened (medians) %.2f; slowest screened round %.3f ms against fastest fp32 round %.3f ms: %s"
          % (med(a) / med(b), max(b), min(a), "faster beyond the spread" if max(b) < min(a) else "NOT faster beyond the spread"))


def stages(forms):
    for name, fn in forms.items():
        try:
            kt = stage_times(fn)
        except Exception as e:                 # the profiler is optional: the event timings stand without it
            print("  (no per-stage times for %s: %r)" % (name, e))
            continue
        print("  %s, kernels under the profiler, us per call (total %.0f):" % (name, sum(t for t, _ in kt.values())))
        for key, (t, n) in sorted(kt.items(), key=lambda kv: -kv[1][0]):
            label = next((lab for pat, lab in STAGES if pat in key.replace(" ", "")), "")
            print("    %8.1f us  %4.1f launches  %-34s %s" % (t, n, label, key[:100]))


def case_topk(L, N, d, reps, rounds):
    from jmac_amd import scoring
    q, tab = operands(L, N, d)
    terms = scoring.csls_terms(q, tab, CSLS_K, "inner")
    assert same(terms, scoring.csls_terms(q, tab, CSLS_K, "inner", screen="bf16")), "the screened csls_terms differ"
    want = scoring.alignment_topk(q, tab, K, CSLS_K, "inner", terms=terms)
    idx, val, st = scoring.alignment_topk(q, tab, K, CSLS_K, "inner", terms=terms, screen="bf16", return_stats=True)
    assert same((idx, val), want), "the screened entry differs"
    print("alignment_topk %d x %d x %d, k = %d, csls_k = %d: indices and values identical; rescored columns per row mean %.1f max %d, "
          "overflow rows %d of %d" % (L, N, d, K, CSLS_K, st["rescored_mean"], st["rescored_max"], st["overflow_rows"], L))
    forms = {"jmac_sim_csls_topk_f32": lambda: scoring.alignment_topk(q, tab, K, CSLS_K, "inner", terms=terms),
             "jmac_sim_csls_topk_screened_f32": lambda: scoring.alignment_topk(q, tab, K, CSLS_K, "inner", terms=terms, screen="bf16")}
    report(rounds_of(forms, reps, rounds), *forms)
    whole = {"alignment_topk (terms included)": lambda: scoring.alignment_topk(q, tab, K, CSLS_K, "inner"),
             "alignment_topk (terms included), screen": lambda: scoring.alignment_topk(q, tab, K, CSLS_K, "inner", screen="bf16")}
    report(rounds_of(whole, reps, rounds), *whole)
    stages(forms)


def case_refill(R, N, d, reps, rounds):
    import torch
    from jmac_amd import scoring
    L = 3000
    q, tab = operands(L, N, d)
    r1, r2 = scoring.csls_terms(q, tab, CSLS_K, "inner")
    st = scoring._StableState(*scoring._csls_topk(q, tab, K, r1, r2, "inner"), N)
    exhausted, _ = st.step()
    ids = st.exhausted_ids(exhausted).to(torch.int64)
    rest = torch.ones(L, dtype=torch.bool, device="cuda")
    rest[ids] = False
    rows = torch.cat([ids, rest.nonzero().flatten()])[:R].sort().values
    rid = rows.to(torch.int32).contiguous()
    sub, r1s = q.index_select(0, rows).contiguous(), r1.index_select(0, rows).contiguous()
    n = torch.empty(R, dtype=torch.int32, device="cuda")
    forms = {"jmac_sim_csls_topk_viable_f32": lambda: scoring._csls_topk(sub, tab, K, r1s, r2, "inner", rid, st.best),
             "jmac_sim_csls_topk_viable_screened_f32": lambda: scoring._csls_topk(sub, tab, K, r1s, r2, "inner", rid, st.best, screen="bf16",
                                                                                  n_rescored=n)}
    a, b = (fn() for fn in forms.values())
    assert same(a, b), "the screened viable entry differs"
    held = int((st.best != 0).sum())
    print("refill of %d rows (%d of them exhausted; %d of %d reviewers hold a suitor) x %d x %d, k = %d: identical; rescored per row "
          "mean %.1f max %d, overflow rows %d" % (R, min(R, exhausted), held, N, N, d, K, float(n[n >= 0].float().mean()) if bool((n >= 0).any()) else 0,
                                                  int(n.max()), int((n == -1).sum())))
    report(rounds_of(forms, reps, rounds), *forms)


def case_run(which, L, N, d, rounds):
    import torch
    from jmac_amd import scoring
    q, tab = operands(L, N, d)
    terms = scoring.csls_terms(q, tab, CSLS_K, "inner")
    if which == "stable":
        run = lambda screen: scoring.stable_alignment(q, tab, K, CSLS_K, "inner", terms=terms, screen=screen)          # noqa: E731
    else:
        run = lambda screen: scoring.auction_alignment(q, tab, K, CSLS_K, "inner", terms=terms, eps=1e-2, screen=screen)          # noqa: E731
    a, b = run(None), run("bf16")
    assert same(a[:-1], b[:-1]), "the screened run differs"
    scr = b[-1].pop("screen")
    assert a[-1] == b[-1], (a[-1], b[-1])
    print("%s_alignment %d x %d x %d, k = %d (terms given): identical results and statistics %s; screen %s" % (which, L, N, d, K, a[-1], scr))
    forms = {"%s_alignment" % which: lambda: run(None), "%s_alignment, screen" % which: lambda: run("bf16")}
    report(rounds_of(forms, 1, rounds, warm=1), *forms)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=4, default=None, metavar=("WHAT", "L", "N", "d"), help="run one case in this process")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=200, help="seconds per case")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if a.case is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("align_screen_timing: no HIP device; nothing is timed on a CPU")
        what, L, N, d = a.case[0], int(a.case[1]), int(a.case[2]), int(a.case[3])
        if what == "topk":
            case_topk(L, N, d, a.reps, a.rounds)
        elif what == "refill":
            case_refill(L, N, d, a.reps, a.rounds)
        else:
            case_run(what, L, N, d, a.rounds)
        sys.stdout.flush()
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
            sys.exit("align_screen_timing: case %s ended with status %d; stopping" % (c, res.returncode))


if __name__ == "__main__":
    main()
