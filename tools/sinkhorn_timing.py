"""The Sinkhorn half-step beside the statistics launch it is modelled on, in ONE process, the forms taking turns after warm-up,
every sample one call between two device events with a device synchronise behind it:
  jmac_sim_lse_f32 rows only (col_add given), columns only (row_add given) -- the two half-steps of an iteration;
  jmac_sim_softmax_stats_f32 rows + columns -- the same product with the larger epilogue, the yardstick;
  sinkhorn_potentials, 10 iterations (20 products, no host read);
on (a) the real ja x en table sizes, 11 805 x 13 996, and (b) config 5's 10 500 x 10 500, seeded unit rows, d = 300.
Prints a text summary and writes it to --out (-> profiles/sinkhorn_timing.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jmac_amd import scoring

SCALE = 50.0


def unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, device="cuda", generator=gen), dim=1)


def sample(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def alternate(forms, warmup, samples):
    """forms: {name: fn}; {name: [ms, one per sample]}, the forms taking turns."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(samples):
        for k, fn in forms.items():
            out[k].append(sample(fn))
    return out


def summary(ms):
    s = sorted(ms)
    n = len(s)
    return s[n // 2], s[0], s[n // 4], s[(3 * n) // 4], s[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "sinkhorn_timing.txt"))
    a = ap.parse_args()
    if a.samples < 20 or a.warmup < 5:
        raise SystemExit("at least 20 samples behind 5 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("sinkhorn_timing: no GPU; a timing taken anywhere else says nothing")
    lines = ["device: %s" % torch.cuda.get_device_name(0),
             "ms per call: median [min, quartiles, max] of %d samples behind %d warm-ups, forms alternating, device events, d = 300, "
             "scale = %g" % (a.samples, a.warmup, SCALE)]
    gen = torch.Generator(device="cuda").manual_seed(0)
    for tag, n1, n2 in (("(a) ja x en tables", 11805, 13996), ("(b) config 5", 10500, 10500)):
        A, B = unit(n1, 300, gen), unit(n2, 300, gen)
        f, g = torch.randn(n1, device="cuda", generator=gen), torch.randn(n2, device="cuda", generator=gen)
        forms = {"sim_lse rows only": lambda: scoring.sim_lse(A, B, SCALE, col_add=g, cols=False),
                 "sim_lse columns only": lambda: scoring.sim_lse(A, B, SCALE, row_add=f, rows=False),
                 "sim_lse rows + columns": lambda: scoring.sim_lse(A, B, SCALE, g, f),
                 "sim_softmax_stats rows + columns": lambda: scoring.sim_softmax_stats(A, B, SCALE),
                 "sinkhorn_potentials, 10 iterations": lambda: scoring.sinkhorn_potentials(A, B, SCALE, 10, metric="inner")}
        r = alternate(forms, a.warmup, a.samples)
        lines.append("%s: %d x %d, %.1f GFLOP per product" % (tag, n1, n2, 2e-9 * n1 * n2 * 300))
        med = {}
        for k, ms in r.items():
            m, lo, q1, q3, hi = summary(ms)
            med[k] = m
            lines.append("  %-36s %8.3f  [%.3f, %.3f .. %.3f, %.3f]  interquartile spread %.1f %%" % (k, m, lo, q1, q3, hi, 100.0 * (q3 - q1) / m))
        y = med["sim_softmax_stats rows + columns"]
        lines.append("  against the statistics launch: rows only %.3f, columns only %.3f, rows + columns %.3f; an iteration's two "
                     "half-steps %.3f ms, sinkhorn_potentials / 10 = %.3f ms; %.1f TFLOP/s inside sinkhorn_potentials"
                     % (med["sim_lse rows only"] / y, med["sim_lse columns only"] / y, med["sim_lse rows + columns"] / y,
                        med["sim_lse rows only"] + med["sim_lse columns only"], med["sinkhorn_potentials, 10 iterations"] / 10.0,
                        20 * 2e-9 * n1 * n2 * 300 / med["sinkhorn_potentials, 10 iterations"]))
        del A, B, f, g
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
