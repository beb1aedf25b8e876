"""numpy restatement of the negative sampler's stream definition (include/jmac_hip.h, jmac_sample_completion_batch):
candidate i of batch row b = word i % 4 of philox4x32_10((b, lo32(step0), i / 4, hi32(step0)), key = (lo32(seed0), lo32(seed1)));
m = word * num_ent, c = m >> 32; invalid if lo32(m) < 2^32 mod num_ent, if c is a true tail of the row's (h, r), or if c equals
a candidate accepted before it; the row's negatives are its first K valid candidates."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of uint64 holding 32-bit words -> four arrays of output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def words(rows, step0, seed, first_block, n_blocks):
    """uint64 [len(rows), 4 * n_blocks]: candidates 4 * first_block ... of each row's stream, as raw 32-bit words."""
    rows = np.asarray(rows, dtype=np.uint64)
    s = int(step0) & 0xFFFFFFFFFFFFFFFF
    blk = np.arange(first_block, first_block + n_blocks, dtype=np.uint64)
    b, k = np.broadcast_arrays(rows[:, None], blk[None, :])
    out = philox4x32_10(b, np.full(b.shape, s & 0xFFFFFFFF, np.uint64), k, np.full(b.shape, s >> 32, np.uint64),
                        int(seed[0]) & 0xFFFFFFFF, int(seed[1]) & 0xFFFFFFFF)
    return np.stack(out, axis=2).reshape(len(rows), 4 * n_blocks)


def negatives(rows, tails, num_ent, K, seed, step0):
    """int64 [len(rows), K]; ``tails[i]``: the true tails of row i's (h, r) (any iterable)."""
    rows = list(rows)
    thr = (1 << 32) % num_ent
    out = np.empty((len(rows), K), dtype=np.int64)
    got = [[] for _ in rows]
    forbidden = [set(int(x) for x in t) for t in tails]
    todo, first = list(range(len(rows))), 0
    while todo:
        w = words([rows[i] for i in todo], step0, seed, first, 16)
        m = w * np.uint64(num_ent)
        cand, low = (m >> np.uint64(32)).astype(np.int64), (m & M32).astype(np.int64)
        for j, i in enumerate(todo):
            acc, bad = got[i], forbidden[i]
            for c, l in zip(cand[j].tolist(), low[j].tolist()):
                if l >= thr and c not in bad and c not in acc:
                    acc.append(c)
                    if len(acc) == K:
                        break
        todo = [i for i in todo if len(got[i]) < K]
        first += 16
    for i, acc in enumerate(got):
        out[i] = acc
    return out


def batch(triples, perm, true_tail, num_ent, B, K, seed, step0, step1):
    """(batch_h, batch_r, batch_t) of the launch that reads step = (step0, step1); ``true_tail``: data.true_tail_dict(triples)."""
    tr = np.asarray(triples, dtype=np.int64)[np.asarray(perm, dtype=np.int64)[step1 * B:(step1 + 1) * B]]
    neg = negatives(range(B), [true_tail[(int(h), int(r))] for h, r in tr[:, :2]], num_ent, K, seed, step0)
    return np.tile(tr[:, 0], K + 1), np.tile(tr[:, 1], K + 1), np.concatenate((tr[:, 2], neg.reshape(-1)))
