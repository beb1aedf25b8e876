"""numpy restatement of the truncated negative sampler (include/jmac_hip.h, jmac_sample_completion_batch_truncated), on
tests/sampler_ref.py's Philox words.  Row b with gold tail t, true-tail set F of its (h, r) and neighbour row n = nbr[t, 0..M):

  lane l is ELIGIBLE if n_l is in [0, num_ent), n_l is not in F and no j < l has n_j == n_l; A = eligible lanes;
  want1 = min(n_hard, A).
  Stage 1: candidate i = word i % 4 of philox4x32_10((b, lo32(step0), 0x80000000 | i / 4, hi32(step0)), key); m = word * M,
  s = m >> 32; invalid if lo32(m) < 2^32 mod M, if lane s is not eligible, or if s was accepted before; the first want1 valid
  candidates give neg[0..want1) = n_s.
  Stage 2: sampler_ref's rule on sampler_ref's counters (third word i / 4 from 0) for slots want1..K, a candidate being invalid
  also when it equals a value stage 1 placed."""
import numpy as np

from sampler_ref import words

HARD = 0x80000000


def eligible(nbr_row, tails, num_ent):
    """[M] bools; ``tails``: the true tails of the row's (h, r) (the gold tail among them)."""
    bad, seen, out = set(int(x) for x in tails), set(), []
    for n in (int(x) for x in nbr_row):
        out.append(0 <= n < num_ent and n not in bad and n not in seen)
        seen.add(n)
    return out


def _walk(rows, todo, step0, seed, base, visit, done):
    """Feed every unfinished row its stream, 64 words at a time, from block ``base`` on: visit(i, word) per word until done(i)."""
    first = 0
    while todo:
        w = words([rows[i] for i in todo], step0, seed, base + first, 16)
        for j, i in enumerate(todo):
            for word in w[j].tolist():
                visit(i, word)
                if done(i):
                    break
        todo = [i for i in todo if not done(i)]
        first += 16


def negatives(rows, tails, nbr_rows, num_ent, K, n_hard, seed, step0, gold=None):
    """int64 [len(rows), K]; ``tails[i]``: the true tails of row i's (h, r); ``nbr_rows[i]``: the [M] neighbour row of row i's gold
    tail.  ``gold`` is needed only where a key leaves fewer than K entities (the kernel repeats the gold tail there)."""
    rows = list(rows)
    forb = [set(int(x) for x in t) for t in tails]
    elig = [eligible(nbr_rows[i], forb[i], num_ent) for i in range(len(rows))]
    want1 = [min(n_hard, sum(e)) for e in elig]
    want = [min(K, max(0, num_ent - len(f))) for f in forb]
    slots, got = [[] for _ in rows], [[] for _ in rows]
    M = len(nbr_rows[0]) if len(rows) else 1
    thr1, thr2 = (1 << 32) % M, (1 << 32) % num_ent

    def hard(i, word):
        m = word * M
        s = m >> 32
        if (m & 0xFFFFFFFF) >= thr1 and elig[i][s] and s not in slots[i]:
            slots[i].append(s)
            got[i].append(int(nbr_rows[i][s]))

    def fill(i, word):
        m = word * num_ent
        c = m >> 32
        if (m & 0xFFFFFFFF) >= thr2 and c not in forb[i] and c not in got[i]:
            got[i].append(c)

    _walk(rows, [i for i in range(len(rows)) if want1[i] > 0], step0, seed, HARD, hard, lambda i: len(slots[i]) >= want1[i])
    _walk(rows, [i for i in range(len(rows)) if want[i] > want1[i]], step0, seed, 0, fill, lambda i: len(got[i]) >= want[i])
    out = np.empty((len(rows), K), dtype=np.int64)
    for i, acc in enumerate(got):
        out[i] = acc + [int(gold[i])] * (K - len(acc)) if len(acc) < K else acc
    return out


def batch(triples, perm, true_tail, nbr, num_ent, B, K, n_hard, seed, step0, step1):
    """(batch_h, batch_r, batch_t) of the launch that reads step = (step0, step1); ``nbr``: the [num_ent, M] table."""
    tr = np.asarray(triples, dtype=np.int64)[np.asarray(perm, dtype=np.int64)[step1 * B:(step1 + 1) * B]]
    nbr = np.asarray(nbr)
    neg = negatives(range(B), [true_tail[(int(h), int(r))] for h, r in tr[:, :2]], nbr[tr[:, 2]], num_ent, K, n_hard, seed, step0,
                    gold=tr[:, 2])
    return np.tile(tr[:, 0], K + 1), np.tile(tr[:, 1], K + 1), np.concatenate((tr[:, 2], neg.reshape(-1)))
