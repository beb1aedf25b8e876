"""The optimal one-to-one alignment (scoring.auction_alignment) beside the stable one (scoring.stable_alignment), in ONE process on
the same seeded operands and the same precomputed csls_terms, at 10 500^2, d = 300, csls_k = 10, k = 16 -- the alignment-evaluation
size of bench.py's `sim` object:
  stable alignment            the top-k + deferred acceptance + viable refills
  auction, default forms      the library picks the launch form of every batch of rounds from the open count
  auction, grid form only     every batch as one bid and one resolve launch per round (the same bits)
After one warm-up call each the forms alternate; a call is timed with the host clock around it (every call ends in host reads of
its own).  Per auction run: rounds, bids, batches (host reads), refills and refill rows, and the precision match1[i] == i beside the
stable matching's and the greedy top-1's.  There is no pass bar on the time.
`--noise X`: the second table is the first plus X / sqrt(d) of unit noise per coordinate (default 3.0: rows do compete).
`--max-rounds N` bounds an auction run (its `complete` is printed).  Writes a text summary (-> profiles/auction_alignment.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jmac_amd import scoring

D, CSLS_K, K = 300, 10, 16


def tables(n, gen, noise):
    b = torch.nn.functional.normalize(torch.randn(n, D, device="cuda", generator=gen) + 0.3 * torch.randn(1, D, device="cuda", generator=gen), dim=1)
    a = torch.nn.functional.normalize(b + noise * torch.randn(n, D, device="cuda", generator=gen) / D ** 0.5, dim=1)
    return a, b


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10500)
    ap.add_argument("--noise", type=float, default=3.0)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--max-rounds", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=3, help="timed calls per form")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "auction_alignment.txt"))
    a = ap.parse_args()
    n = a.n
    gen = torch.Generator(device="cuda").manual_seed(0)
    e1, e2 = tables(n, gen, a.noise)
    terms = scoring.csls_terms(e1, e2, CSLS_K)
    forms = {"stable alignment": lambda: scoring.stable_alignment(e1, e2, K, CSLS_K, "inner", terms=terms),
             "auction, default forms": lambda: scoring.auction_alignment(e1, e2, K, CSLS_K, "inner", terms=terms, eps=a.eps,
                                                                         max_rounds=a.max_rounds),
             "auction, grid form only": lambda: scoring.auction_alignment(e1, e2, K, CSLS_K, "inner", terms=terms, eps=a.eps,
                                                                          max_rounds=a.max_rounds, form=1)}
    lines = ["device: %s" % torch.cuda.get_device_name(0),
             "n1 = n2 = %d, d = %d, csls_k = %d, k = %d, noise %.1f, eps %g (one stored matrix would be %.1f MB)"
             % (n, D, CSLS_K, K, a.noise, a.eps, n * n * 4 / 2 ** 20)]
    gold = torch.arange(n, device="cuda")
    top1 = scoring.alignment_topk(e1, e2, 1, CSLS_K, "inner", terms=terms)[0][:, 0]
    lines.append("greedy top-1: match == i for %.2f %% of the rows" % (100 * float((top1 == gold).float().mean())))
    outs, ms = {}, {k: [] for k in forms}
    for k, fn in forms.items():                                   # warm-up: allocator, code objects
        outs[k] = wall_ms(fn)[1]
    for _ in range(a.rounds):
        for k, fn in forms.items():
            ms[k].append(wall_ms(fn)[0])
    for k in forms:
        m1, stats = outs[k][0], outs[k][-1]
        lines.append("%s:" % k)
        lines.append("  wall ms per call: %s  median %.2f" % (" ".join("%.2f" % x for x in ms[k]), sorted(ms[k])[len(ms[k]) // 2]))
        lines.append("  stats: %s" % stats)
        matched = m1 >= 0
        lines.append("  match1[i] == i for %.2f %% of the matched rows" % (100 * float(((m1 == gold) & matched).sum()) / max(1, int(matched.sum()))))
    d0, d1 = outs["auction, default forms"], outs["auction, grid form only"]
    lines.append("default forms and grid form only agree bitwise: %s"
                 % bool(torch.equal(d0[0], d1[0]) and torch.equal(d0[1], d1[1]) and torch.equal(d0[2], d1[2])))
    v = d0[1][d0[0] >= 0].double().sum().item()
    s_m1, s_v1 = outs["stable alignment"][0], outs["stable alignment"][1]
    lines.append("total rescored similarity: auction %.4f, stable matching %.4f" % (v, s_v1[s_m1 >= 0].double().sum().item()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
