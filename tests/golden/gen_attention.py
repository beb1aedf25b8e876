#!/usr/bin/env python3
"""Golden vectors of the layer's per-edge attention weights: runs the REFERENCE's RelationAwareLayer (and, for layer_dbpv1, the
DBPv1 RelationalAwareLayer), imported the way gen_golden.py imports them (build container only), on the inputs and param.* of the
committed layer fixtures, and records what modules.helper.message_passing.scatter_softmax returns inside the forward -- the first
call of a forward is the neighbour branch [E,1], the second the self loop [N,1].  Arrays only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_attention.py      # writes tests/golden/attention.npz

Keys: alpha_<fixture> [E] (the softmax) and alpha_scaled_<fixture> [E] (after the reference's `/= edge_norm`, i.e. times sqrt(deg)).
The two reference trees have modules of the same names, so each variant runs in a child process with its own sys.path.  The GPU
box never runs this file; it only reads the fixture."""
import argparse
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("JMAC_REFERENCE", "/root/reference")

np.int = int        # noqa  (aliases removed in numpy >= 1.24 that the reference still uses)
np.float = float    # noqa
if not hasattr(np, "bool"):
    np.bool = bool  # noqa

ROOT_CASES = ["layer_tiny", "layer_rand200", "layer_d300", "layer_ja_train", "layer_noedge"]


def run_variant(variant, out_path):
    import torch
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "oracle", "_shim"))
    sys.path.insert(0, os.path.join(REF, "JMAC_DBPv1") if variant == "dbpv1" else REF)
    import modules.helper.message_passing as mp
    if variant == "dbpv1":
        from models.jmac_model import RelationalAwareLayer
        cases = ["layer_dbpv1"]
        make = lambda d, nr, slope: RelationalAwareLayer(d, d, nr, rel_dim=d, act=torch.tanh,
                                                         args=types.SimpleNamespace(leaky_relu_w=slope, opn="sub"))
    else:
        from src.jmac_model import RelationAwareLayer
        cases = ROOT_CASES
        make = lambda d, nr, slope: RelationAwareLayer(d, d, rel_dim=d, act=torch.tanh,
                                                       args=types.SimpleNamespace(leaky_relu_w=slope, comp_op="sub"))
    calls = []
    inner = mp.scatter_softmax

    def recording(score, index, dim=0):
        out = inner(score, index, dim=dim)
        calls.append(out.detach().clone())          # the caller divides its result in place
        return out

    mp.scatter_softmax = recording
    out = {}
    for case in cases:
        g = np.load(os.path.join(HERE, case + ".npz"))
        n, d, nr = int(g["n"]), int(g["d"]), int(g["nr"])
        layer = make(d, nr, float(g["slope"]))
        layer.load_state_dict({k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}, strict=False)
        layer.eval()                                # the weights are pre-BN: the BatchNorm state does not enter
        ei, et = torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_type"])
        del calls[:]
        with torch.no_grad():
            layer(torch.from_numpy(g["X"]), torch.from_numpy(g["R"]), ei, et)
            norm = layer.compute_norm(ei, n)
        assert len(calls) == 2 and calls[0].shape == (ei.shape[1], 1) and calls[1].shape == (n, 1), [c.shape for c in calls]
        alpha = calls[0].reshape(-1)
        name = case[len("layer_"):]
        out["alpha_" + name] = alpha.numpy().astype(np.float32)
        out["alpha_scaled_" + name] = (alpha / norm).numpy().astype(np.float32)
        print("  %-10s E=%d  sum(alpha)=%.6f over %d destinations" % (name, ei.shape[1], float(alpha.sum()), len(set(ei[0].tolist()))))
    np.savez(out_path, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="all", choices=["all", "root", "dbpv1"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.variant != "all":
        run_variant(a.variant, a.out)
        return
    merged = {}
    with tempfile.TemporaryDirectory() as tmp:
        for v in ("root", "dbpv1"):
            part = os.path.join(tmp, v + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v, "--out", part], check=True)
            z = np.load(part)
            merged.update({k: z[k] for k in z.files})
    path = os.path.join(HERE, "attention.npz")
    np.savez_compressed(path, **merged)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
