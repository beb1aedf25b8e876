"""The screened alignment ranks against the fp32 entry on the same tensors (-> profiles/rank_screen_timing.txt).

Cases, each in ONE child process of its own (the parent stops at the first child that fails): a shape (3000 x 30000 x 300 and
13996 x 13996 x 256) and a gold mix, csls_k = 10:
    easy    the queries are noisy copies of their gold rows (cosine to the gold about 0.7: it is the best column of nearly every row)
    mixed   the same queries, 10 % of the rows get a random gold column
    hard    every gold column is random
Per case, with the terms computed once beforehand: jmac_sim_csls_rank_f32 (scoring.alignment_ranks) against
jmac_sim_csls_rank_screened_f32 called directly with finish = 0 (no host read; the rows it leaves unranked are reported) and
against scoring.alignment_ranks(screen="bf16"), which finishes those rows with the fp32 entry; then the whole evaluation --
csls_terms' two products and the ranks, what scoring.alignment_test(matrix_free=True) runs -- without and with the screen.
All forms are asserted to return the same ranks first; then, after 5 warm-up calls, `rounds` rounds in which the forms take
turns, device events around `reps` back-to-back calls.  "spread" is (max - min) / min over a form's rounds; a screened form counts
as faster only if its slowest round beats the fp32 form's fastest.  Per-stage device times come from 10 further calls under
torch.profiler; `--calls N` runs N calls of every form and nothing else, for a kernel trace taken from outside
(rocprofv3 --kernel-trace --stats -- python tools/rank_screen_timing.py --case easy 3000 30000 300 --calls 10).
`JMAC_LIB_PATH` selects another build of the library (the RK_CAP comparison: the constant is compiled in)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from align_screen_timing import report, rounds_of  # noqa: E402
from sim_screen_timing import stage_times  # noqa: E402

CSLS_K = 10
SHAPES = [(3000, 30000, 300), (13996, 13996, 256)]
CASES = [(mix, L, N, d) for L, N, d in SHAPES for mix in ("easy", "mixed", "hard")]
STAGES = [("screen_prepare_kernel", "prepare (bf16 copies, norms)"), ("screen_gold_kernel", "gold values"),
          ("screen_gemm_kernel<true", "count / list product (bf16)"), ("screen_rank_resolve_kernel", "resolve (rescore the lists)"),
          ("csls_gold_kernel", "fp32 entry: gold values"), ("sim_gemm_kernel", "fp32 product, count epilogue")]


def operands(mix, L, N, d):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(L + N)
    tab = torch.nn.functional.normalize(torch.randn(N, d, device="cuda", generator=gen))
    gold = torch.randperm(N, device="cuda", generator=gen)[:L]
    noise = torch.nn.functional.normalize(torch.randn(L, d, device="cuda", generator=gen))
    q = torch.nn.functional.normalize(tab[gold] + noise).contiguous()
    if mix != "easy":
        rand = torch.randint(0, N, (L,), device="cuda", generator=gen)
        pick = torch.rand(L, device="cuda", generator=gen) < (0.1 if mix == "mixed" else 2.0)
        gold = torch.where(pick, rand, gold)
    return q, tab, gold.to(torch.int32).contiguous()


def raw_entry(q, tab, terms, gold):
    """jmac_sim_csls_rank_screened_f32 with finish = 0 on held buffers: () -> (rank, n_rescored)"""
    import torch
    from jmac_amd._lib import check, lib, ptr, stream, workspace
    n1, d = q.shape
    n2 = tab.shape[0]
    rank = torch.empty(n1, dtype=torch.int32, device="cuda")
    nres = torch.empty(n1, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib().jmac_sim_csls_rank_screened_workspace_bytes(n1, n2, d))
    ws = workspace(ws_bytes, q.device)

    def call():
        check(lib().jmac_sim_csls_rank_screened_f32(ptr(q), d, ptr(tab), d, n1, n2, d, ptr(terms[0]), ptr(terms[1]), ptr(gold), ptr(rank),
                                                    ptr(nres), 0, ptr(ws), ws_bytes, stream()), "jmac_sim_csls_rank_screened_f32")
        return rank, nres
    return call


def run_case(mix, L, N, d, reps, rounds, calls):
    import torch
    from jmac_amd import scoring
    q, tab, gold = operands(mix, L, N, d)
    terms = scoring.csls_terms(q, tab, CSLS_K, "inner")
    t2 = scoring.csls_terms(q, tab, CSLS_K, "inner", screen="bf16")
    assert torch.equal(terms[0], t2[0]) and torch.equal(terms[1], t2[1]), "the screened csls_terms differ"
    raw = raw_entry(q, tab, terms, gold)
    forms = {"jmac_sim_csls_rank_f32": lambda: scoring.alignment_ranks(q, tab, gold, CSLS_K, "inner", terms=terms),
             "jmac_sim_csls_rank_screened_f32, finish = 0": raw,
             "alignment_ranks(screen), rows finished": lambda: scoring.alignment_ranks(q, tab, gold, CSLS_K, "inner", terms=terms, screen="bf16")}
    whole = {"terms + ranks": lambda: scoring.alignment_ranks(q, tab, gold, CSLS_K, "inner"),
             "terms + ranks, screen": lambda: scoring.alignment_ranks(q, tab, gold, CSLS_K, "inner", screen="bf16")}
    if calls:
        for fn in list(forms.values()) + list(whole.values()):
            for _ in range(calls):
                fn()
        torch.cuda.synchronize()
        return
    want = forms["jmac_sim_csls_rank_f32"]()
    got, st = scoring.alignment_ranks(q, tab, gold, CSLS_K, "inner", terms=terms, screen="bf16", return_stats=True)
    assert torch.equal(got, want), "the screened ranks differ"
    rank, nres = raw()
    done = nres >= 0
    assert torch.equal(rank[done], want[done]) and bool((rank[~done] == 0).all()) and torch.equal(nres.cpu(), st["n_rescored"])
    assert torch.equal(whole["terms + ranks, screen"](), want) and torch.equal(whole["terms + ranks"](), want)
    print("ranks %d x %d x %d, csls_k = %d, %s golds (Hits@1 %.1f %%, median rank %d): identical ranks; rescored columns per row mean %.1f "
          "max %d over the rows that fit, overflow rows %d of %d (%.1f %%)"
          % (L, N, d, CSLS_K, mix, 100.0 * float((want == 1).float().mean()), int(want.median()), st["rescored_mean"], st["rescored_max"],
             st["overflow_rows"], L, 100.0 * st["overflow_rows"] / L))
    ms = rounds_of(forms, reps, rounds)
    names = list(forms)
    report({k: ms[k] for k in names[:2]}, names[0], names[1])
    report({k: ms[k] for k in (names[0], names[2])}, names[0], names[2])
    report(rounds_of(whole, reps, rounds), *whole)
    for name in names[:2]:
        try:
            kt = stage_times(forms[name])
        except Exception as e:                 # the profiler is optional: the event timings stand without it
            print("  (no per-stage times for %s: %r)" % (name, e))
            continue
        print("  %s, kernels under the profiler, us per call (total %.0f):" % (name, sum(t for t, _ in kt.values())))
        for key, (t, n) in sorted(kt.items(), key=lambda kv: -kv[1][0]):
            label = next((lab for pat, lab in STAGES if pat in key.replace(" ", "")), "")
            print("    %8.1f us  %4.1f launches  %-34s %s" % (t, n, label, key[:100]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=4, default=None, metavar=("MIX", "L", "N", "d"), help="run one case in this process")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="with --case: this many calls of every form, untimed (for an outside kernel trace)")
    ap.add_argument("--limit", type=int, default=200, help="seconds per case")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if a.case is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("rank_screen_timing: no HIP device; nothing is timed on a CPU")
        run_case(a.case[0], int(a.case[1]), int(a.case[2]), int(a.case[3]), a.reps, a.rounds, a.calls)
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
            sys.exit("rank_screen_timing: case %s ended with status %d; stopping" % (c, res.returncode))


if __name__ == "__main__":
    main()
