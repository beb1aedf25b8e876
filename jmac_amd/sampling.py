"""Completion batches built on the device: the reference's filtered negative sampler as one launch per batch.

Replaces ``completion_data_processing`` (train.py:262-285: the ``(h, r) -> tails`` dictionary), ``TrainDataset``
(modules/load/data_loader.py:36-47: ``np.random.choice(all_ent[mask], num_negative, replace=False)`` per triple, in DataLoader
worker processes) and the ``repeat`` / ``cat`` of train.py:347-352:

    TrueTailIndex       the dictionary as a CSR on the device, built once per triple list (i.e. once per EnTr refresh)
    CompletionSampler   persistent batch buffers + ``jmac_sample_completion_batch`` (csrc/sample.hip): ``next_batch()`` is one
                        launch, no host read, and returns THE SAME tensors every time -- a step that starts with it captures
                        in a hipGraph and every replay trains on the next batch of the epoch
    NeighborTable       ``generate_neighbours`` / ``find_neighbours`` (modules/train/batch.py:121-164): every entity's ``m`` nearest
                        entities in one persistent int32 buffer, refreshed in place by the fused top-k; a sampler that is given
                        one draws its first ``n_hard`` negatives from the gold tail's row (``--neg_sampling truncated``:
                        ``jmac_sample_completion_batch_truncated``)

The draw is the reference's distribution (uniform, without replacement, from the entities that are not a true tail of the
row's ``(h, r)``) over a Philox stream of its own -- include/jmac_hip.h states it; tests/sampler_ref.py restates it in numpy.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, check_index_range, lib, mark_index_range, ptr, require_device, stream, workspace


class TrueTailIndex:
    """``(h, r) -> sorted distinct tails`` of a triple list (what ``data.true_tail_dict`` returns as a dictionary) as a CSR:
    ``keys`` int64 [nk, 2] in lexicographic order, ``tail_ptr`` int32 [nk + 1], ``tail_idx`` int32, and ``key_of_triple``
    int32 [T]: the CSR row that holds triple i's ``(h, r)`` (None for an index built ``from_dict``: only the sampler reads it).
    ``key_code`` int64 [nk] = ``h << 32 | r``: strictly ascending (the same order, ids < 2^31) -- what the link-prediction
    kernels binary-search (``jmac_tail_index_t``: scoring.linkpred_ranks / linkpred_topk with ``index=``).  Ids are rows of the
    candidate table, i.e. KG-local.  For head prediction build the index from the triples' columns ``[2, 1, 0]``."""

    def __init__(self, keys, tail_ptr, tail_idx, key_of_triple=None):
        self.keys, self.tail_ptr, self.tail_idx, self.key_of_triple = keys, tail_ptr, tail_idx, key_of_triple
        self.key_code = ((keys[:, 0] << 32) | keys[:, 1]).contiguous()

    @classmethod
    def from_triples(cls, triples, device) -> "TrueTailIndex":
        t = torch.as_tensor(np.asarray(triples, dtype=np.int64).reshape(-1, 3) if not isinstance(triples, torch.Tensor) else triples)
        t = t.to(device=device, dtype=torch.int64).reshape(-1, 3)
        if not len(t):
            raise ValueError("TrueTailIndex: empty triple list")
        if len(t) >= 1 << 31 or int(t.min()) < 0 or int(t.max()) >= 1 << 31:
            raise ValueError("TrueTailIndex: ids must lie in [0, 2^31) and the list must have fewer than 2^31 triples")
        nrel, nent = int(t[:, 1].max()) + 1, int(t[:, 2].max()) + 1
        hr, key_of_triple = torch.unique(t[:, 0] * nrel + t[:, 1], return_inverse=True)       # sorted: (h, r) lexicographic
        pair = torch.unique(key_of_triple * nent + t[:, 2])                                    # sorted: by key, then tail
        counts = torch.bincount(torch.div(pair, nent, rounding_mode="floor"), minlength=len(hr))
        tail_ptr = torch.zeros(len(hr) + 1, dtype=torch.int64, device=t.device)
        tail_ptr[1:] = torch.cumsum(counts, 0)
        keys = torch.stack((torch.div(hr, nrel, rounding_mode="floor"), hr % nrel), 1)
        return cls(keys, tail_ptr.to(torch.int32), (pair % nent).to(torch.int32), key_of_triple.to(torch.int32))

    @classmethod
    def from_dict(cls, true_tail, device) -> "TrueTailIndex":
        """The same CSR from a ``{(h, r): tails}`` dictionary (``data.true_tail_dict``, ``KnowledgeGraph.true_tail``):
        ``from_dict(true_tail_dict(t), dev)`` equals ``from_triples(t, dev)`` field by field (``key_of_triple`` aside)."""
        if not len(true_tail):
            raise ValueError("TrueTailIndex: empty dictionary")
        items = sorted(true_tail.items(), key=lambda kv: (int(kv[0][0]), int(kv[0][1])))
        keys = np.array([k for k, _ in items], dtype=np.int64).reshape(-1, 2)
        lens = np.fromiter((len(v) for _, v in items), dtype=np.int64, count=len(items))
        flat = (np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for _, v in items]) if lens.sum()
                else np.zeros(0, dtype=np.int64))
        if len(flat) >= 1 << 31 or keys.min() < 0 or keys.max() >= 1 << 31 or (len(flat) and (flat.min() < 0 or flat.max() >= 1 << 31)):
            raise ValueError("TrueTailIndex: ids must lie in [0, 2^31) and the lists must hold fewer than 2^31 tails")
        nent = int(flat.max()) + 1 if len(flat) else 1
        pair = np.unique(np.repeat(np.arange(len(items), dtype=np.int64), lens) * nent + flat)     # sorted: by key, then tail
        tail_ptr = np.zeros(len(items) + 1, dtype=np.int64)
        tail_ptr[1:] = np.cumsum(np.bincount(pair // nent, minlength=len(items)))
        return cls(torch.from_numpy(keys).to(device), torch.from_numpy(tail_ptr.astype(np.int32)).to(device),
                   torch.from_numpy((pair % nent).astype(np.int32)).to(device), None)

    def c_struct(self):
        """``jmac_tail_index_t`` over this index's device buffers (keep the index alive while a launch reads it)."""
        from ._lib import TailIndex
        return TailIndex(ptr(self.key_code), len(self.key_code), ptr(self.tail_ptr), ptr(self.tail_idx))

    def longest(self) -> int:
        p = self.tail_ptr
        return int((p[1:] - p[:-1]).max())


class NeighborTable:
    """``idx`` int32 ``[num_ent, m]`` on the device: row e lists the ``m`` entities nearest to entity e, best first -- the
    dictionary of ``generate_neighbours`` (modules/train/batch.py:121-164) as one buffer whose address never changes, so a
    captured step that samples from it stays valid across refreshes.  Like the reference's list, a row computed by ``refresh``
    contains the entity itself (its own nearest neighbour); the sampler never draws it for a gold tail t because t is a true
    tail of the row's (h, r).  ``1 <= m <= min(64, num_ent)`` (the fused top-k's bound)."""

    def __init__(self, num_ent: int, m: int, device):
        self.num_ent, self.m = int(num_ent), int(m)
        if not 1 <= self.num_ent < 1 << 31:
            raise ValueError("NeighborTable: num_ent must lie in [1, 2^31)")
        if not 1 <= self.m <= min(64, self.num_ent):
            raise ValueError("NeighborTable: m must lie in [1, min(64, num_ent)] (got %d, num_ent = %d)" % (self.m, self.num_ent))
        self.idx = torch.zeros((self.num_ent, self.m), dtype=torch.int32, device=torch.device(device))
        self._val = None                                                   # 'manhattan': the L1 entry insists on a value output

    @classmethod
    def from_indices(cls, idx, device=None) -> "NeighborTable":
        """A table from a caller's ``[num_ent, m]`` int32 / int64 array or tensor (entries in ``[0, num_ent)``: IndexError
        otherwise).  Repeats inside a row are allowed: the kernel counts an entity once."""
        if not isinstance(idx, torch.Tensor):
            idx = torch.from_numpy(np.ascontiguousarray(np.asarray(idx)))
        if idx.dim() != 2 or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError("NeighborTable.from_indices: an int32 / int64 [num_ent, m] array is expected (got %s %s)"
                             % (idx.dtype, tuple(idx.shape)))
        table = cls(idx.shape[0], idx.shape[1], idx.device if device is None else device)
        check_index_range(idx, table.num_ent, "NeighborTable.from_indices")
        table.idx.copy_(idx)
        return table

    def refresh(self, emb: torch.Tensor, metric: str = "inner", screen=None) -> "NeighborTable":
        """Fill the table in place with the ``m`` nearest rows of ``emb`` ``[num_ent, d]`` (fp32, device) for every row of ``emb``.
        ``"inner"``: largest inner product first, ``find_neighbours``' ``np.matmul`` (``jmac_sim_topk_f32``; ``screen="bf16"``: its
        screened form, the same bits); ``"manhattan"``: smallest L1 distance first (``jmac_l1_csls_topk_f32`` without CSLS terms).
        Ties -> lower index first.  The kernels write the int32 table itself: no host read, no copy."""
        from .scoring import _check_screen, _rows16
        if metric not in ("inner", "manhattan"):
            raise ValueError("NeighborTable.refresh: metric must be 'inner' or 'manhattan' (got %r)" % (metric,))
        _check_screen("NeighborTable.refresh", screen, metric)
        if emb.dim() != 2 or emb.shape[0] != self.num_ent:
            raise ValueError("NeighborTable.refresh: emb must be [%d, d] (got %s)" % (self.num_ent, tuple(emb.shape)))
        require_device(emb, self.idx)
        a = _rows16(emb.detach())
        n, d = a.shape
        L = lib()
        if metric == "manhattan":
            if self._val is None:
                self._val = torch.empty((n, self.m), dtype=torch.float32, device=a.device)
            ws_bytes = int(L.jmac_l1_csls_topk_workspace_bytes(n, n, d, self.m))
            ws = workspace(ws_bytes, a.device)
            check(L.jmac_l1_csls_topk_f32(ptr(a), d, ptr(a), d, n, n, d, None, None, self.m, ptr(self._val), ptr(self.idx), ptr(ws),
                                          ws_bytes, stream()), "jmac_l1_csls_topk_f32")
        elif screen is None:
            ws_bytes = int(L.jmac_sim_topk_workspace_bytes(n, n, self.m))
            ws = workspace(ws_bytes, a.device)
            check(L.jmac_sim_topk_f32(ptr(a), d, ptr(a), d, n, n, d, self.m, None, ptr(self.idx), ptr(ws), ws_bytes, stream()),
                  "jmac_sim_topk_f32")
        else:
            ws_bytes = int(L.jmac_sim_topk_screened_workspace_bytes(n, n, d, self.m))
            ws = workspace(ws_bytes, a.device)
            check(L.jmac_sim_topk_screened_f32(ptr(a), d, ptr(a), d, n, n, d, self.m, None, ptr(self.idx), None, ptr(ws), ws_bytes,
                                               stream()), "jmac_sim_topk_screened_f32")
        return self


class CompletionSampler:
    """The batches of one KG's completion epochs (train.py:338-352), on the device.

    ``new_epoch(generator)`` draws the epoch's order; ``len(sampler)`` full batches follow (the ragged last batch is skipped:
    train.py:342-346); ``next_batch()`` returns ``{"batch_h", "batch_r", "batch_t"}`` for ``JMAC.completion_loss``, each
    int64 ``[B (K + 1)]``; ``neg`` is the ``[B, K]`` view of the negatives.  ``seed``: two int64 words (or one int: the second
    word is 0) that key the Philox stream; None draws them from torch's generator of the device.

    ``neighbors`` (a ``NeighborTable`` of the same ``num_ent``): the first ``n_hard`` (default: all ``K``) negatives of a row
    come from the gold tail's neighbours that are not a true tail, the rest from the uniform draw (include/jmac_hip.h,
    jmac_sample_completion_batch_truncated; tests/trunc_sampler_ref.py).  The table is read at every launch: refresh it in place."""

    def __init__(self, triples, num_ent: int, batch_size: int, num_negative: int, device, seed=None, neighbors: NeighborTable = None,
                 n_hard: int = None):
        device = torch.device(device)
        tr = np.ascontiguousarray(np.asarray(triples.cpu() if isinstance(triples, torch.Tensor) else triples, dtype=np.int64).reshape(-1, 3))
        self.num_ent, self.B, self.K, self.T = int(num_ent), int(batch_size), int(num_negative), len(tr)
        if not 1 <= self.K <= 64:
            raise ValueError("CompletionSampler: num_negative must lie in [1, 64] (got %d)" % self.K)
        if self.B < 1 or self.T < self.B:
            raise ValueError("CompletionSampler: need 1 <= batch_size <= len(triples) (got %d, %d)" % (self.B, self.T))
        if not 1 <= self.num_ent < 1 << 31:
            raise ValueError("CompletionSampler: num_ent must lie in [1, 2^31)")
        if neighbors is None and n_hard is not None:
            raise ValueError("CompletionSampler: n_hard needs a NeighborTable (neighbors=)")
        self.neighbors, self.n_hard = neighbors, self.K if n_hard is None else int(n_hard)
        if neighbors is not None:
            if neighbors.num_ent != self.num_ent:
                raise ValueError("CompletionSampler: the NeighborTable covers %d entities, the sampler %d" % (neighbors.num_ent, self.num_ent))
            if not 0 <= self.n_hard <= self.K:
                raise ValueError("CompletionSampler: n_hard must lie in [0, num_negative] (got %d)" % self.n_hard)
        if tr[:, [0, 2]].min() < 0 or tr[:, [0, 2]].max() >= self.num_ent or tr[:, 1].min() < 0:   # the reference: IndexError
            raise IndexError("CompletionSampler: triple ids out of range: entities in [%d, %d], valid range [0, %d); relations >= %d"
                             % (tr[:, [0, 2]].min(), tr[:, [0, 2]].max(), self.num_ent, tr[:, 1].min()))
        self.triples = torch.from_numpy(tr).to(device)
        self.index = TrueTailIndex.from_triples(self.triples, device)
        if self.num_ent - self.index.longest() < self.K:        # np.random.choice(..., replace=False) raises ValueError there
            raise ValueError("CompletionSampler: a (head, relation) with %d true tails leaves fewer than num_negative = %d of the "
                             "%d entities" % (self.index.longest(), self.K, self.num_ent))
        require_device(self.triples)                            # the batches are built by a kernel: there is no CPU path
        if neighbors is not None and neighbors.idx.device != self.triples.device:
            raise ValueError("CompletionSampler: the NeighborTable lives on %s, the sampler on %s" % (neighbors.idx.device, self.triples.device))
        n = self.B * (self.K + 1)
        # The kernel rewrites these three in place on every launch WITHOUT bumping their _version.  Nothing on the completion path
        # caches on their identity or version: losses._PAIR_INDEX keys on the link columns only, model._link_columns on the links
        # tensor, and check_index_range is settled by the marks below (the triples were range-checked above; a negative is in
        # [0, num_ent) by construction), so no launch of a step reads anything back.
        self.batch_h = mark_index_range(torch.zeros(n, dtype=torch.int64, device=device), self.num_ent)
        self.batch_r = mark_index_range(torch.zeros(n, dtype=torch.int64, device=device), int(tr[:, 1].max()) + 1)
        self.batch_t = mark_index_range(torch.zeros(n, dtype=torch.int64, device=device), self.num_ent)
        self.neg = self.batch_t[self.B:].view(self.B, self.K)
        self._batch = {"batch_h": self.batch_h, "batch_r": self.batch_r, "batch_t": self.batch_t}
        self.perm = torch.arange(self.T, dtype=torch.int64, device=device)
        self.step = torch.zeros(2, dtype=torch.int64, device=device)      # [0] launches so far, [1] batch number in the epoch
        if seed is None:
            self.seed = torch.empty(2, dtype=torch.int64, device=device).random_()
        else:
            words = [int(seed), 0] if np.ndim(seed) == 0 else [int(s) for s in seed]
            if len(words) != 2:
                raise ValueError("CompletionSampler: seed is one int or two")
            self.seed = torch.tensor(words, dtype=torch.int64).to(device)
        self._served = None                                                # batches handed out eagerly this epoch (None: no epoch yet)

    def __len__(self):
        return self.T // self.B

    def new_epoch(self, generator=None):
        """A new order, written into the SAME ``perm`` buffer (a captured launch stays valid), and batch number 0.  The
        draw counter ``step[0]`` runs on, so no epoch repeats an earlier epoch's negatives."""
        self.perm.copy_(torch.randperm(self.T, device=self.perm.device, generator=generator))
        self.step[1:].zero_()
        self._served = 0
        return self

    def skip(self, n: int):
        """Account on the host for ``n`` batches produced by replays of a captured ``next_batch()``."""
        self._served += int(n)

    def next_batch(self):
        """Launch; the same three tensors every time.  Raises StopIteration after ``len(self)`` eager calls of an epoch (a
        call inside a stream capture does not run and is not counted: its replays are, through ``skip``)."""
        if self._served is None:
            raise RuntimeError("CompletionSampler: call new_epoch() first")
        if not torch.cuda.is_current_stream_capturing():
            if self._served >= len(self):
                raise StopIteration
            self._served += 1
        ix = self.index
        if self.neighbors is not None:
            nb = self.neighbors
            check(lib().jmac_sample_completion_batch_truncated(
                ptr(self.triples), self.T, ptr(self.perm), ptr(ix.key_of_triple), ptr(ix.tail_ptr), ptr(ix.tail_idx), self.num_ent,
                self.B, self.K, ptr(nb.idx), nb.idx.stride(0), nb.m, self.n_hard, ptr(self.seed), ptr(self.step), ptr(self.batch_h),
                ptr(self.batch_r), ptr(self.batch_t), stream()), "jmac_sample_completion_batch_truncated")
            return self._batch
        check(lib().jmac_sample_completion_batch(ptr(self.triples), self.T, ptr(self.perm), ptr(ix.key_of_triple), ptr(ix.tail_ptr),
                                                 ptr(ix.tail_idx), self.num_ent, self.B, self.K, ptr(self.seed), ptr(self.step),
                                                 ptr(self.batch_h), ptr(self.batch_r), ptr(self.batch_t), stream()),
              "jmac_sample_completion_batch")
        return self._batch
