#!/usr/bin/env python3
"""Golden vectors of the alignment evaluator under metric='manhattan': runs the REFERENCE's modules.finding.evaluation.test and
similarity.sim (imported the way gen_golden.py imports them, build container only) on the e1 / e2 of the committed align_eval.npz,
for normalize in {False, True} x csls_k in {0, 10}, and stores arrays only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_align_manhattan.py      # writes tests/golden/align_manhattan.npz

Keys: hits_/mr_/mrr_/sim_ + "n<0|1>_csls<0|10>".  The GPU box never runs this file; it only reads the fixture."""
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("JMAC_REFERENCE", "/root/reference")

np.int = int        # noqa  (aliases removed in numpy >= 1.24 that the reference still uses)
np.float = float    # noqa
if not hasattr(np, "bool"):
    np.bool = bool  # noqa


def main():
    sys.path.insert(0, REF)
    from modules.finding.evaluation import test
    from modules.finding.similarity import sim
    z = np.load(os.path.join(HERE, "align_eval.npz"))
    e1, e2 = z["e1"], z["e2"]
    lg = logging.getLogger("golden")
    lg.setLevel(logging.ERROR)
    out = {}
    for normalize in (False, True):
        for k in (0, 10):
            tag = "n%d_csls%d" % (int(normalize), k)
            top_k, hits, mr, mrr = test(e1, e2, None, [1, 5, 10], 1, metric="manhattan", normalize=normalize, csls_k=k, accurate=True,
                                        logger=lg)
            out["hits_" + tag] = np.asarray(hits, dtype=np.float64)
            out["mr_" + tag] = np.float64(mr)
            out["mrr_" + tag] = np.float64(mrr)
            out["sim_" + tag] = sim(e1, e2, metric="manhattan", normalize=normalize, csls_k=k).astype(np.float32)
            print(tag, hits, mr, mrr)
    path = os.path.join(HERE, "align_manhattan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
