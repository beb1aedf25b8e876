#!/usr/bin/env python3
"""Golden-vector generator for the neighbour table: runs the REFERENCE's ``find_neighbours`` (modules/train/batch.py:156-164,
imported from the reference tree, build container only) on seeded embeddings and stores inputs + its lists as a small fixture.

    JMAC_REFERENCE=<reference tree> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_neighbours.py
                                                                        # writes tests/golden/neighbours_small.npz

Nothing from the reference is copied: it is imported, called, and only arrays are saved.  Accommodation applied at import time
(gen_golden.py's no. 2): the ``np.int`` / ``np.float`` / ``np.bool`` aliases are restored.  The GPU box never runs this file.

``find_neighbours`` keeps ``np.argpartition``'s k smallest of the negated fp32 products: a SET of k entities per row, in no order,
so the fixture stores each row sorted by id."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

np.int = int        # noqa
np.float = float    # noqa
if not hasattr(np, "bool"):
    np.bool = bool  # noqa

N, D, K = 300, 20, 16


def embeddings():
    """The (300, 20) rows of tests/test_gpu_sampling_truncated.py: standard normal, L2-normalised, fp32."""
    e = np.random.default_rng(20261021).standard_normal((N, D))
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)


def main():
    sys.path.insert(0, os.environ["JMAC_REFERENCE"])                      # the reference tree (gen_golden.py's variable)
    from modules.train.batch import find_neighbours
    emb = embeddings()
    ents = np.arange(N)
    dic = find_neighbours(ents, ents, emb, emb, K)
    nbr = np.array([sorted(dic[i]) for i in range(N)], dtype=np.int32)
    assert nbr.shape == (N, K)
    path = os.path.join(HERE, "neighbours_small.npz")
    np.savez_compressed(path, emb=emb, k=np.int64(K), neighbours=nbr)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
