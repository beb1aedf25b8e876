"""Manhattan-metric alignment without the n1 x n2 matrix, timed against the bare L1 score kernel (-> profiles/align_manhattan_timing.txt).

Per shape (unit rows, d = 300, csls_k = 10), in ONE process, warm-up first, then rounds in which the forms take turns; device time
from HIP events around `reps` back-to-back calls:

    l1_scores                       jmac_l1_score_f32 into a preallocated [n1, n2] matrix: the yardstick, 2 n1 n2 d lane instructions
                                    and one matrix written
    csls_terms                      two fused top-k passes (a against b, b against a): 2 x the yardstick's instructions, no matrix
    alignment_ranks(terms)          one pass with the count epilogue
    alignment_topk(k = 10, terms)   sample + filter pass + selection
    stored: l1 -> 1 - x -> csls_rank   the stored composition of the same ranks

"x yardstick" is device time per pass over the yardstick's; "VALU" is 2 n1 n2 d lane instructions per pass over the time, as a share of
the fp32 vector issue peak (256 CUs x 4 SIMDs x 32 lanes / clock x 2.4 GHz = 78.6 T lane instructions / s).  Each shape runs in a
child process of its own under a time limit; the parent stops at the first child that fails."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_ISSUE_PEAK = 256 * 4 * 32 * 2.4e9
SHAPES = [(10000, 10000, 300), (3000, 30000, 300)]


def med(v):
    return sorted(v)[len(v) // 2]


def measure(forms, reps, rounds):
    """{name: [ms per call, one entry per round]}: events around `reps` calls, the forms alternating inside every round."""
    import torch
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps)
    return out


def run_shape(n1, n2, d, reps, rounds):
    import torch
    from jmac_amd import scoring
    M, ck = "manhattan", 10
    gen = torch.Generator(device="cuda").manual_seed(n1 + n2)
    a = torch.nn.functional.normalize(torch.randn(n1, d, device="cuda", generator=gen))
    b = torch.nn.functional.normalize(torch.randn(n2, d, device="cuda", generator=gen))
    gold = torch.randint(0, n2, (n1,), device="cuda", generator=gen, dtype=torch.int32)
    terms = scoring.csls_terms(a, b, ck, M)
    dist = torch.empty((n1, n2), dtype=torch.float32, device="cuda")

    def stored():
        scoring.l1_scores(a, b, out=dist)
        return scoring.csls_rank(1.0 - dist, ck, gold)

    # the timed forms compute what the stored composition computes, at this size
    assert torch.equal(scoring.alignment_ranks(a, b, gold, ck, M, terms=terms), stored())
    forms = {"l1_scores (yardstick)": (1, lambda: scoring.l1_scores(a, b, out=dist)),
             "csls_terms": (2, lambda: scoring.csls_terms(a, b, ck, M)),
             "alignment_ranks(terms)": (1, lambda: scoring.alignment_ranks(a, b, gold, ck, M, terms=terms)),
             "alignment_topk(k=10, terms)": (1, lambda: scoring.alignment_topk(a, b, 10, ck, M, terms=terms)),
             "stored: l1 -> 1 - x -> csls_rank": (1, stored)}
    ms = measure({k: fn for k, (_, fn) in forms.items()}, reps, rounds)
    base = med(ms["l1_scores (yardstick)"])
    instr = 2.0 * n1 * n2 * d
    print("%d x %d x %d, csls_k = %d; ms per call, %d rounds of %d calls, alternating:" % (n1, n2, d, ck, rounds, reps))
    for k, (passes, _) in forms.items():
        m = med(ms[k])
        print("  %-34s %s  median %.3f ms  spread %.1f %%  passes %d  x yardstick per pass %.3f  VALU %.3f"
              % (k, " ".join("%.3f" % v for v in ms[k]), m, 100.0 * (max(ms[k]) - min(ms[k])) / min(ms[k]), passes, m / passes / base,
                 instr * passes / (m * 1e-3) / VALU_ISSUE_PEAK))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=None, help="run one shape in this process")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    a = ap.parse_args()
    if a.shape is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("align_manhattan_timing: no HIP device; nothing is timed on a CPU")
        run_shape(*a.shape, a.reps, a.rounds)
        return
    for s in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape"] + [str(v) for v in s] + ["--reps", str(a.reps), "--rounds", str(a.rounds)]
        rc = subprocess.run(cmd, timeout=a.limit).returncode
        if rc != 0:
            sys.exit("align_manhattan_timing: shape %s ended with status %d; stopping" % (s, rc))


if __name__ == "__main__":
    main()
