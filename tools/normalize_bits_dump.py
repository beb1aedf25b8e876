"""Every output of the row normalise + dropout entry points of norm.hip, as raw bytes, for comparing two builds of the library bit
for bit (profiles/normalize_one_body.txt, section 2).  One process per build; JMAC_LIB_PATH selects the library:

  JMAC_LIB_PATH=<build A> python tools/normalize_bits_dump.py --write DIR      # one file per tensor + index.txt
  JMAC_LIB_PATH=<build B> python tools/normalize_bits_dump.py --check DIR      # recomputes, compares with the files, exit 1 on a difference

Entry points: jmac_row_normalize_drop_{fwd,bwd}_f32 (mask NULL and a mask), jmac_row_normalize_dropseed_{fwd,bwd}_f32,
jmac_rows_normalize_dropseed_fwd_f32, jmac_row_normalize_dropseed_bwd_rows_f32 (with / without add, map none / permutation,
accumulate 0 / 1), jmac_bn_tanh_normalize_dropseed_fwd_f32, jmac_bn_tanh_bwd_normadj_f32 (training and eval, with / without gy2),
jmac_row_normalize_{fwd,bwd}_f32.  d = 12, 64, 300, 512 and (where the entry takes it) 516; N = 1, 5, 1031, 2049; p_drop 0, 0.05, 0.4;
destinations and gradients pitched 2d (3d as well at p_drop 0.4); one all-zero row and one row of 1e-20.  Fixed seeds.
--digest stores SHA-256 of the bytes instead of the bytes (where the directory has no room for ~2 GB)."""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jmac_amd import _lib, encoder, ops  # noqa: E402

DEV = "cuda"
DS, NS, PS = (12, 64, 300, 512, 516), (1, 5, 1031, 2049), (0.0, 0.05, 0.4)


class Sink:
    def __init__(self, root, check, digest):
        self.root, self.check, self.digest = root, check, digest
        self.count, self.nbytes, self.differ, self.groups = 0, 0, [], {}
        if not check:
            os.makedirs(root, exist_ok=True)
            self.index = open(os.path.join(root, "index.txt"), "w")
        else:
            self.names = [ln.rstrip("\n") for ln in open(os.path.join(root, "index.txt"))]

    def put(self, name, t):
        torch.cuda.synchronize()
        raw = t.detach().contiguous().cpu().numpy().tobytes()
        if self.digest:
            raw = hashlib.sha256(raw).digest() + len(raw).to_bytes(8, "little")
        path = os.path.join(self.root, "%05d.bin" % self.count)
        if self.check:
            if self.names[self.count] != name:
                raise SystemExit("case order differs at %d: %s / %s" % (self.count, self.names[self.count], name))
            with open(path, "rb") as f:
                if f.read() != raw:
                    self.differ.append(name)
        else:
            with open(path, "wb") as f:
                f.write(raw)
            self.index.write(name + "\n")
        grp = name.split("/")[0]
        self.groups[grp] = self.groups.get(grp, 0) + 1
        self.count += 1
        self.nbytes += t.numel() * t.element_size()


def rows(N, d, gen, scale=1.0):
    x = torch.randn(N, d, device=DEV, generator=gen) * scale
    if N > 3:
        x[1] = 0.0
        x[3] = 1e-20
    else:
        x[0] = 1e-20
    return x


def pitched(N, d, pitch):
    buf = torch.zeros(N, pitch * d, device=DEV)
    return buf[:, d:2 * d], buf


def shape_cases(N, d, out):
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + d)
    tag = "N%d-d%d" % (N, d)
    x = rows(N, d, gen)
    seed = torch.tensor([(0x1234ABCD << 32) | 0x9E3779B9], dtype=torch.int64, device=DEV)
    base = torch.randn(N, d, device=DEV, generator=gen)
    add = torch.randn(N, d, device=DEV, generator=gen)
    perm = torch.randperm(N, device=DEV, generator=gen)
    # jmac_row_normalize_{fwd,bwd}_f32 (any d)
    xs = x.clone().requires_grad_(True)
    y = ops.row_normalize(xs)
    y.backward(base)
    out.put("plain/%s/y" % tag, y)
    out.put("plain/%s/gx" % tag, xs.grad)
    # BatchNorm side of the fused entries
    w = torch.rand(d, device=DEV, generator=gen) + 0.5
    b = torch.rand(d, device=DEV, generator=gen) * 0.4 - 0.2
    rm0 = torch.randn(d, device=DEV, generator=gen) * 0.1
    rv0 = torch.rand(d, device=DEV, generator=gen) + 0.5
    xb = torch.randn(N, d, device=DEV, generator=gen) * 0.5 + 0.1
    xe = rows(N, d, gen, 0.5)                                   # eval with mean 0, bias 0: a zero row and one below eps in c1
    g2 = torch.randn(N, d, device=DEV, generator=gen)
    for p in PS:
        mask = (torch.rand(N, d, device=DEV, generator=gen) < 1.0 - p).float() if p > 0 else None
        for pitch in ((2, 3) if p == 0.4 else (2,)):
            what = "%s/p%g-ld%dd" % (tag, p, pitch)
            g = torch.randn(N, pitch * d, device=DEV, generator=gen)[:, d:2 * d]
            for form, kw in (("mask", {"mask": mask}), ("seed", {"seed": seed})):
                yv, buf = pitched(N, d, pitch)
                inv, drop = encoder._norm_drop_fwd(x, p, True, yv, **kw)
                out.put("%s_fwd/%s/y" % (form, what), buf)
                out.put("%s_fwd/%s/inv" % (form, what), inv[:N])
                for acc in (0, 1):
                    gx, gbuf = pitched(N, d, pitch)
                    if acc:
                        gx.copy_(base)
                    encoder._norm_drop_bwd(x, inv, drop, g, gx, bool(acc))
                    out.put("%s_bwd/%s/acc%d" % (form, what, acc), gbuf)
            if d > 512:
                continue
            inv, drop = encoder._norm_drop_fwd(x, p, True, pitched(N, d, 2)[0], seed=seed)
            for mname, rmap in (("none", None), ("perm", perm)):
                yv, buf = pitched(N, d, pitch)
                xr, inv1, _ = encoder._gather_norm_drop_fwd(x, rmap, p, True, yv, seed=seed)
                out.put("rows_fwd/%s-%s/x_rows" % (what, mname), xr)
                out.put("rows_fwd/%s-%s/y" % (what, mname), buf)
                out.put("rows_fwd/%s-%s/inv" % (what, mname), inv1[:N])
                for with_add in (True, False):
                    for acc in (0, 1):
                        got = encoder._norm_drop_bwd_scatter(x, inv, drop, g, add if with_add else None, rmap,
                                                             dst=base.clone() if acc else None)
                        out.put("rows_bwd/%s-%s/add%d-acc%d" % (what, mname, with_add, acc), got)
                for training in (True, False):
                    xin = xb if training else xe
                    bias = b if training else torch.zeros_like(b)
                    rm, rv = (rm0.clone() if training else torch.zeros_like(rm0)), rv0.clone()
                    y1 = torch.empty(N, d, device=DEV)
                    yr1 = torch.full((N, d), float("nan"), device=DEV) if rmap is not None else None
                    yn1, nbuf = pitched(N, d, pitch)
                    mean, invstd, invn = ops.bn_tanh_norm_fwd_raw(xin, w, bias, rm, rv, training, 0.1, 1e-5, y1, yn1,
                                                                  encoder._seed_drop(p, True, seed), rmap, yr1)
                    name = "bn_fwd/%s-%s-%s" % (what, mname, "train" if training else "eval")
                    for k, t in (("y", y1), ("y_rows", yr1), ("yn", nbuf), ("inv", invn[:N]), ("mean", mean), ("invstd", invstd),
                                 ("running_mean", rm), ("running_var", rv)):
                        if t is not None:
                            out.put("%s/%s" % (name, k), t)
                    for with_g2 in (True, False):
                        gx, gbw = ops.bn_tanh_bwd_normadj_raw(xin, y1, invn, encoder._seed_drop(p, True, seed), g,
                                                              g2 if with_g2 else None, rmap, w, mean, invstd, training)
                        name = "bn_bwd/%s-%s-%s-gy2_%d" % (what, mname, "train" if training else "eval", with_g2)
                        out.put(name + "/gx", gx)
                        out.put(name + "/gbw", gbw)


def all_cases(out):
    for d in DS:
        for N in NS:
            shape_cases(N, d, out)


def main(cases=all_cases):
    """--write / --check of every tensor that ``cases(sink)`` puts (tools/aggregate_bits_dump.py runs its own cases through it)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--write")
    ap.add_argument("--check")
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--list", type=int, default=40, help="differing tensors named in the report")
    a = ap.parse_args()
    if bool(a.write) == bool(a.check):
        ap.error("one of --write DIR, --check DIR")
    out = Sink(a.write or a.check, bool(a.check), a.digest)
    print("library:", _lib.LIB_PATH)
    cases(out)
    print("  " + ", ".join("%s %d" % kv for kv in sorted(out.groups.items())) + " tensors")
    if not a.check:
        print("WROTE: %d tensors (%.0f MB)%s" % (out.count, out.nbytes / 1e6, ", as digests" if a.digest else ""))
        return 0
    for name in out.differ[:a.list]:
        print("  differs:", name)
    print("RESULT: %d tensors (%.0f MB) compared%s, %d differ" % (out.count, out.nbytes / 1e6, " by digest" if a.digest else "",
                                                                  len(out.differ)))
    return 1 if out.differ else 0


if __name__ == "__main__":
    sys.exit(main())
