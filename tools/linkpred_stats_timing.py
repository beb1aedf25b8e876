"""What link-prediction confidence costs: jmac_linkpred_stats_f32 in prediction mode (no gold) and in evaluation mode (gold) against
jmac_linkpred_rank_indexed_f32 -- the yardstick: the same prep and tile kernels with the compare-and-count epilogue -- on the
same operands: the ja KG of the fixture (N = 11 805, its real known-tail index), d = 300, two layers of seeded tables, for the
whole validation split (B = 8 633) and for its first 1 000 queries.  The entry points are called through ctypes on buffers
allocated once, so a window holds launches only.  ONE process: warm-up, then --rounds rounds in which the forms take turns,
HIP events around --reps calls each.  "x rank" is the median over the yardstick's median; "spread" is (max - min) / min over a
form's rounds; "VALU" is 2 layers d B N lane instructions per call over the time, as a share of the fp32 vector issue peak (256
CUs x 4 SIMDs x 32 lanes / clock x 2.4 GHz).  Run it under a time limit; prints a text summary
(-> profiles/linkpred_stats_timing.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jmac_amd import _lib, data, scoring

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
VALU_ISSUE_PEAK = 256 * 4 * 32 * 2.4e9


def med(v):
    return sorted(v)[len(v) // 2]


def measure(forms, reps, rounds):
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[k].append(ev[0].elapsed_time(ev[1]) / reps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40, help="calls per timed window")
    ap.add_argument("--scale", type=float, default=0.05)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from jmac_amd.sampling import TrueTailIndex
    kgs, _, _, _ = data.kgs_from_arrays(data.load_dbp5l_arrays(os.path.join(GOLDEN, "dbp5l_ja_el_data.npz")), "ja")
    ja = kgs["ja"]
    N, d, nl = ja.num_entity, 300, 2
    gen = torch.Generator(device="cuda").manual_seed(1234)
    ent = [torch.randn(N, d, device="cuda", generator=gen) for _ in range(nl)]
    rel = [0.1 * torch.randn(ja.num_relation, d, device="cuda", generator=gen) for _ in range(nl)]
    arr, keep, _, _ = scoring._link_layers(ent, rel, False)
    index = TrueTailIndex.from_dict(ja.true_tail, "cuda")
    ix, keep_ix = scoring._tail_index(index, ent[0].device)
    L, st = _lib.lib(), _lib.stream()
    print("device: %s" % torch.cuda.get_device_name(0))
    print("ja: N = %d, d = %d, %d layers, index of %d keys / %d tails; scale %g; %d rounds of %d calls, the forms taking turns"
          % (N, d, nl, len(index.key_code), index.tail_idx.numel(), a.scale, a.rounds, a.reps))
    for B in (len(ja.val_data), 1000):
        q = ja.val_data[:B]
        h, r, g = (torch.from_numpy(q[:, c].copy()).to(device="cuda", dtype=torch.int32) for c in range(3))
        listed = sum(len(ja.true_tail.get((int(x), int(y)), ())) > 0 for x, y in zip(q[:, 0], q[:, 1]))
        rank = torch.empty(B, dtype=torch.int32, device="cuda")
        near = torch.empty(B, dtype=torch.int32, device="cuda")
        dmin, lsum, ent_o, logp = (torch.empty(B, dtype=torch.float32, device="cuda") for _ in range(4))
        wr_bytes = L.jmac_linkpred_rank_workspace_bytes(B, d, nl)
        ws_bytes = L.jmac_linkpred_stats_workspace_bytes(B, N, d, nl)
        wr, ws = _lib.workspace(wr_bytes, "cuda"), _lib.workspace(ws_bytes, "cuda")

        def rank_call():
            _lib.check(L.jmac_linkpred_rank_indexed_f32(arr, nl, h.data_ptr(), r.data_ptr(), 0, g.data_ptr(), ix, B, N, d, rank.data_ptr(),
                                                        wr.data_ptr(), wr_bytes, st))

        def stats_call(gold):
            _lib.check(L.jmac_linkpred_stats_f32(arr, nl, h.data_ptr(), r.data_ptr(), 0, gold, ix, B, N, d, a.scale, near.data_ptr(),
                                                 dmin.data_ptr(), lsum.data_ptr(), ent_o.data_ptr(), logp.data_ptr() if gold else None,
                                                 ws.data_ptr(), ws_bytes, st))

        forms = {"rank_indexed_f32 (yardstick)": rank_call,
                 "stats_f32, prediction mode": lambda: stats_call(None),
                 "stats_f32, evaluation mode": lambda: stats_call(g.data_ptr())}
        ms = measure(forms, a.reps, a.rounds)
        base = med(ms["rank_indexed_f32 (yardstick)"])
        instr = 2.0 * nl * d * B * N
        print("B = %d (%d queries with a list); workspace %.1f MB (rank call %.1f MB; B x N x 4 = %.1f MB); ms per call:"
              % (B, listed, ws_bytes / 2 ** 20, wr_bytes / 2 ** 20, B * N * 4 / 2 ** 20))
        for k in forms:
            m = med(ms[k])
            print("  %-30s %s  median %.3f ms  spread %.1f %%  x rank %.3f  VALU %.3f"
                  % (k, " ".join("%.3f" % v for v in ms[k]), m, 100.0 * (max(ms[k]) - min(ms[k])) / min(ms[k]), m / base,
                     instr / (m * 1e-3) / VALU_ISSUE_PEAK))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
