"""Completion / alignment scoring on libjmac_hip.so (boundary B3).

    l1_scores            == torch.cdist(er, table, p=1)                      src/jmac_model.py:312
    linkpred_dist        == JMAC.forward_linkpred after forward_base          src/jmac_model.py:301-313
    filtered_rank        == filter + sort + np.where of CompletionEvaluator   src/validate.py:50-64
    sim_topk / get_neg   == mm + topk                                         modules/utils/util.py:31-54
    align_entropy        == first half of compute_alignment_quality           train.py:235-248
    alignment_quality    == compute_alignment_quality                         train.py:231-259
    alignment_stats      == what seed_enlargement_triple_transferring reads of it (entropy, row / column maxima and
                            arg-maxima of the two softmax matrices) without any N1 x N2 matrix   train.py:138-169
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check, check_index_range, lib, ptr, require_device, stream, workspace


def _rows16(t: torch.Tensor, allow_bf16: bool = False) -> torch.Tensor:
    """fp32 (or bf16 where the kernel has a bf16-table form), contiguous, row length padded to a multiple of 4
    elements with zeros (16-byte fp32 rows / 8-byte bf16 rows)."""
    if t.dtype != torch.float32 and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise TypeError("fp32%s only (got %s)" % (" / bf16" if allow_bf16 else "", t.dtype))
    d = t.shape[1]
    if d % 4:
        t = torch.nn.functional.pad(t, (0, 4 - d % 4))
    return t.contiguous()


def l1_scores(er: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None,
              accumulate: bool = False) -> torch.Tensor:
    """``torch.cdist(er, table, p=1)`` -> fp32 [B, N].  A bf16 ``table`` selects the bf16-operand kernel
    (``er`` is rounded to bf16 to match; the accumulation stays fp32) -- BASELINE config 3."""
    require_device(er, table)
    bf16 = table.dtype == torch.bfloat16
    if bf16 and er.dtype != torch.bfloat16:
        er = er.to(torch.bfloat16)
    er, table = _rows16(er, bf16), _rows16(table, bf16)       # zero padding adds |0-0| = 0
    B, d = er.shape
    N = table.shape[0]
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=er.device)
        accumulate = False
    fn, name = (lib().jmac_l1_score_bf16, "jmac_l1_score_bf16") if bf16 else (lib().jmac_l1_score_f32, "jmac_l1_score_f32")
    check(fn(ptr(er), er.shape[1], ptr(table), table.shape[1], B, N, d, ptr(out), out.stride(0),
             1 if accumulate else 0, stream()), name)
    return out


def linkpred_dist(comp_layers: Sequence[torch.Tensor], comp_rel_layers: Sequence[torch.Tensor], e_index, r_index,
                  pred_head: bool = False, table_dtype=torch.float32) -> torch.Tensor:
    """sum over layers of cdist(E_l[h] +/- R_l[r], E_l, p=1) (src/jmac_model.py:302-313).  table_dtype=bfloat16
    rounds the query rows and the candidate table to bf16 (fp32 accumulation) -- BASELINE config 3."""
    dev = comp_layers[0].device
    e_index = torch.as_tensor(e_index, dtype=torch.long, device=dev)
    r_index = torch.as_tensor(r_index, dtype=torch.long, device=dev)
    dist = None
    for ent, rel in zip(comp_layers, comp_rel_layers):
        e, r = ent[e_index], rel[r_index]
        er = e - r if pred_head else e + r                               # jmac_model.py:308-311
        if table_dtype == torch.bfloat16:
            er, ent = er.to(torch.bfloat16), ent.to(torch.bfloat16)
        dist = l1_scores(er, ent, out=dist, accumulate=dist is not None)
    return dist


def _link_layers(comp_layers, comp_rel_layers, bf16: bool):
    """(jmac_link_layer_t array, tensors to keep alive, N, d) of the (entity table, relation table) layers."""
    from ._lib import LinkLayer
    require_device(*comp_layers, *comp_rel_layers)
    nl = len(comp_layers)
    if nl != len(comp_rel_layers) or not 1 <= nl <= 4:
        raise ValueError("1..4 layers of (entity table, relation table)")
    N, d = comp_layers[0].shape
    keep, arr = [], (LinkLayer * nl)()
    for l, (ent, rel) in enumerate(zip(comp_layers, comp_rel_layers)):
        if ent.shape != (N, d) or rel.shape[1] != d:
            raise ValueError("layer tables disagree in shape")
        ent, rel = ent.detach().float().contiguous(), rel.detach().float().contiguous()
        tab = _rows16(ent.to(torch.bfloat16), True) if bf16 else ent
        keep += [ent, rel, tab]
        arr[l] = LinkLayer(ptr(ent), ent.stride(0), ptr(rel), rel.stride(0), ptr(tab), tab.stride(0))
    return arr, keep, N, d


def _query_column(x, n: int, what: str, dev) -> torch.Tensor:
    """A column of query ids (list, numpy array or tensor), range-checked, as a contiguous int32 device tensor."""
    check_index_range(x, n, what)
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64).reshape(-1)))
    return x.to(device=dev, dtype=torch.int32).contiguous()


def _tail_index(index, dev):
    """(byref(jmac_tail_index_t) or None, the struct to keep alive) of a sampling.TrueTailIndex."""
    import ctypes
    if index is None:
        return None, None
    require_device(index.key_code, index.tail_ptr, index.tail_idx)
    if index.key_code.device != dev:
        raise ValueError("index lives on %s, the tables on %s" % (index.key_code.device, dev))
    st = index.c_struct()
    return ctypes.byref(st), st


def linkpred_ranks(comp_layers: Sequence[torch.Tensor], comp_rel_layers: Sequence[torch.Tensor], e_index, r_index, gold,
                   filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                   pred_head: bool = False, table_dtype=torch.float32, index=None) -> torch.Tensor:
    """Filtered ranks of the gold tails -- ``filtered_rank(linkpred_dist(...), gold, filt_ptr, filt_idx)`` without the
    [B, N] distance matrix (forward_linkpred src/jmac_model.py:302-313 + the ranking loop of src/validate.py:50-64, i.e. what
    CompletionEvaluator.test needs).  The distance of a candidate is one running fp32 sum over (layer, k) where the
    materialised path rounds once more per layer: same rank unless the gold is tied with a neighbour at fp32 rounding.
    ``index``: a sampling.TrueTailIndex instead of the per-batch CSR -- every query's filter is looked up on the device
    (the same ranks as the CSR of the same lists; a query whose (h, r) the index does not hold ranks raw).  ``e_index``,
    ``r_index`` and ``gold`` may be lists, numpy arrays or device tensors."""
    if index is not None and (filt_ptr is not None or filt_idx is not None):
        raise ValueError("linkpred_ranks: pass either index or filt_ptr / filt_idx, not both")
    bf16 = table_dtype == torch.bfloat16
    arr, keep, N, d = _link_layers(comp_layers, comp_rel_layers, bf16)
    nl, dev = len(comp_layers), comp_layers[0].device
    h = _query_column(e_index, N, "e_index", dev)
    r = _query_column(r_index, comp_rel_layers[0].shape[0], "r_index", dev)
    g = _query_column(gold, N, "gold", dev)
    B = h.numel()
    if r.numel() != B or g.numel() != B:
        raise ValueError("e_index, r_index and gold must have one entry per query")
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    L = lib()
    ws_bytes = int(L.jmac_linkpred_rank_workspace_bytes(B, d, nl))
    ws = workspace(ws_bytes, dev)
    if index is not None:
        ix, _keep_ix = _tail_index(index, dev)
        name = "jmac_linkpred_rank_indexed_bf16" if bf16 else "jmac_linkpred_rank_indexed_f32"
        check(getattr(L, name)(arr, nl, ptr(h), ptr(r), 1 if pred_head else 0, ptr(g), ix, B, N, d, ptr(rank), ptr(ws), ws_bytes,
                               stream()), name)
        return rank
    fn, name = (L.jmac_linkpred_rank_bf16, "jmac_linkpred_rank_bf16") if bf16 else (L.jmac_linkpred_rank_f32, "jmac_linkpred_rank_f32")
    check(fn(arr, nl, ptr(h), ptr(r), 1 if pred_head else 0, ptr(g), ptr(filt_ptr), ptr(filt_idx), B, N, d, ptr(rank), ptr(ws),
             ws_bytes, stream()), name)
    return rank


def linkpred_topk(comp_layers: Sequence[torch.Tensor], comp_rel_layers: Sequence[torch.Tensor], e_index, r_index, k: int,
                  index=None, pred_head: bool = False, table_dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """The model's predictions: ``(idx int64 [B, k], dist fp32 [B, k])``, the k nearest candidates of every ``(h, r)`` under
    linkpred_ranks' distance, ascending (equal distances: lower index first), without the [B, N] matrix.  ``index``: a
    sampling.TrueTailIndex whose listed tails -- the facts already known -- are excluded (None: nothing is).  A query with
    fewer than k candidates left ends its row with ``idx = -1, dist = +inf``.  1 <= k <= 64.  The distances are bit for bit
    those the ranks are decided on: ``linkpred_ranks(gold=idx[:, j], index=index)`` is ``j + 1``."""
    bf16 = table_dtype == torch.bfloat16
    arr, keep, N, d = _link_layers(comp_layers, comp_rel_layers, bf16)
    nl, dev = len(comp_layers), comp_layers[0].device
    k = int(k)
    if not 1 <= k <= 64 or k > N:
        raise ValueError("linkpred_topk: k must lie in [1, min(64, N)] (got %d, N = %d)" % (k, N))
    h = _query_column(e_index, N, "e_index", dev)
    r = _query_column(r_index, comp_rel_layers[0].shape[0], "r_index", dev)
    B = h.numel()
    if r.numel() != B:
        raise ValueError("e_index and r_index must have one entry per query")
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    val = torch.empty((B, k), dtype=torch.float32, device=dev)
    L = lib()
    ws_bytes = int(L.jmac_linkpred_topk_workspace_bytes(B, N, d, nl, k))
    ws = workspace(ws_bytes, dev)
    ix, _keep_ix = _tail_index(index, dev)
    name = "jmac_linkpred_topk_bf16" if bf16 else "jmac_linkpred_topk_f32"
    check(getattr(L, name)(arr, nl, ptr(h), ptr(r), 1 if pred_head else 0, ix, B, N, d, k, ptr(val), ptr(idx), ptr(ws), ws_bytes,
                           stream()), name)
    return idx.to(torch.int64), val


def link_map(pairs, n_target: int, n_support: int, device=None) -> torch.Tensor:
    """int32 [n_target] link map of a supporting KG from ``pairs`` [L, 2] of (target row, support row): entry n is the support
    row aligned with target row n, -1 where no pair names n.  A target row listed twice keeps the SMALLEST support row.
    Ids outside their KG raise ValueError.  (The ``match`` vectors of the alignment methods are link maps already.)"""
    p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    p = p.astype(np.int64).reshape(-1, 2)
    n_target, n_support = int(n_target), int(n_support)
    if len(p) and (p[:, 0].min() < 0 or p[:, 0].max() >= n_target or p[:, 1].min() < 0 or p[:, 1].max() >= n_support):
        raise ValueError("link_map: pair ids outside [0, %d) x [0, %d)" % (n_target, n_support))
    link = np.full(n_target, n_support, dtype=np.int64)
    np.minimum.at(link, p[:, 0], p[:, 1])
    link[link == n_support] = -1
    return torch.from_numpy(link.astype(np.int32)).to(device) if device is not None else torch.from_numpy(link.astype(np.int32))


def _link_members(members, who: str):
    """(jmac_link_member_t array, tensors to keep alive, N, d, n_layers, relation rows every member has) of
    ``[(comp_layers, comp_rel_layers, link_or_None, weight), ...]``: member 0 is the target, the others read through their link
    maps (int32 / int64 [N] device tensors with values in [-1, rows of that member]), range-checked here before any launch."""
    import math
    from ._lib import LinkMember
    if not 1 <= len(members) <= 4:
        raise ValueError("%s: 1..4 members (the target, then up to 3 supporting KGs)" % who)
    arr, keep = (LinkMember * len(members))(), []
    N = d = nl = None
    nrel = None
    for g, (comp_layers, comp_rel_layers, link, weight) in enumerate(members):
        lay, kp, rows, dg = _link_layers(comp_layers, comp_rel_layers, False)
        if g == 0:
            N, d, nl, dev = rows, dg, len(comp_layers), comp_layers[0].device
        if dg != d or len(comp_layers) != nl or comp_layers[0].device != dev:
            raise ValueError("%s: member %d disagrees with the target in d, layers or device" % (who, g))
        weight = float(weight)
        if not (math.isfinite(weight) and weight >= 0.0):
            raise ValueError("%s: weights must be finite and >= 0 (member %d: %r)" % (who, g, weight))
        if (g == 0) != (link is None):
            raise ValueError("%s: the target (member 0) has no link map, every supporting member has one" % who)
        if link is not None:
            require_device(link)
            if link.dim() != 1 or link.numel() != N or link.device != dev:
                raise ValueError("%s: member %d's link map must hold one entry per target row (%d) on %s" % (who, g, N, dev))
            if link.dtype != torch.int32:
                if link.dtype != torch.int64:
                    raise TypeError("%s: link maps are int32 or int64 (got %s)" % (who, link.dtype))
                link = link.to(torch.int32)
            link = link.contiguous()
            check_index_range(link, rows, "member %d's link map" % g, lo=-1)
            kp.append(link)
        rr = min(int(x.shape[0]) for x in comp_rel_layers)
        nrel = rr if nrel is None else min(nrel, rr)
        keep += [lay, kp]
        arr[g] = LinkMember(lay, ptr(link), rows, weight)
    return arr, keep, N, d, nl, nrel


def linkpred_ranks_ensemble(members, e_index, r_index, gold, index=None, pred_head: bool = False) -> torch.Tensor:
    """linkpred_ranks(index=...) on the cross-KG ensemble distance.  ``members`` = ``[(comp_layers, comp_rel_layers, link, weight),
    ...]``: member 0 is the target KG (``link`` None), a supporting member s scores query (h, r) and candidate n in its OWN
    tables at the rows ``link_s[h]`` and ``link_s[n]`` (``link_map``; relation ids are shared).  With d_g the single-KG distance
    of member g, D = w_0 d_0, then D = fma(w_s, d_s if both rows are linked else d_0, D) for s = 1, 2, ..: a missing link falls
    back to the target's own distance.  The ranks are decided on D exactly as linkpred_ranks decides on d_0 (same tie rule);
    the filter ``index`` is the TARGET's sampling.TrueTailIndex.  One member with weight 1 is linkpred_ranks bit for bit.
    No [B, N] matrix and no permuted table copies exist: the kernel reads supporting rows through the link maps."""
    arr, keep, N, d, nl, nrel = _link_members(members, "linkpred_ranks_ensemble")
    dev = members[0][0][0].device
    h = _query_column(e_index, N, "e_index", dev)
    r = _query_column(r_index, nrel, "r_index", dev)
    g = _query_column(gold, N, "gold", dev)
    B = h.numel()
    if r.numel() != B or g.numel() != B:
        raise ValueError("e_index, r_index and gold must have one entry per query")
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    L = lib()
    ws_bytes = int(L.jmac_linkpred_ens_rank_workspace_bytes(B, d, nl, len(members)))
    ws = workspace(ws_bytes, dev)
    ix, _keep_ix = _tail_index(index, dev)
    check(L.jmac_linkpred_ens_rank_f32(arr, len(members), nl, ptr(h), ptr(r), 1 if pred_head else 0, ptr(g), ix, B, N, d, ptr(rank),
                                       ptr(ws), ws_bytes, stream()), "jmac_linkpred_ens_rank_f32")
    return rank


def linkpred_topk_ensemble(members, e_index, r_index, k: int, index=None, pred_head: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """linkpred_topk on the cross-KG ensemble distance D of linkpred_ranks_ensemble: ``(idx int64 [B, k], D fp32 [B, k])``, the
    k nearest target rows the target's ``index`` does not list, ascending (equal: lower index first), padded with
    ``idx = -1, D = +inf``.  ``linkpred_ranks_ensemble(members, ..., gold=idx[:, j], index=index)`` is ``j + 1``."""
    arr, keep, N, d, nl, nrel = _link_members(members, "linkpred_topk_ensemble")
    dev = members[0][0][0].device
    k = int(k)
    if not 1 <= k <= 64 or k > N:
        raise ValueError("linkpred_topk_ensemble: k must lie in [1, min(64, N)] (got %d, N = %d)" % (k, N))
    h = _query_column(e_index, N, "e_index", dev)
    r = _query_column(r_index, nrel, "r_index", dev)
    B = h.numel()
    if r.numel() != B:
        raise ValueError("e_index and r_index must have one entry per query")
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    val = torch.empty((B, k), dtype=torch.float32, device=dev)
    L = lib()
    ws_bytes = int(L.jmac_linkpred_ens_topk_workspace_bytes(B, N, d, nl, len(members), k))
    ws = workspace(ws_bytes, dev)
    ix, _keep_ix = _tail_index(index, dev)
    check(L.jmac_linkpred_ens_topk_f32(arr, len(members), nl, ptr(h), ptr(r), 1 if pred_head else 0, ix, B, N, d, k, ptr(val), ptr(idx),
                                       ptr(ws), ws_bytes, stream()), "jmac_linkpred_ens_topk_f32")
    return idx.to(torch.int64), val


class LinkStats(namedtuple("LinkStats", "nearest dist_min sum entropy logp_gold scale")):
    """Per-query statistics of ``softmax_n(-scale * dist[b, n])`` over the query's candidate set (include/jmac_hip.h,
    jmac_linkpred_stats_*): ``nearest`` int64 [B] (-1: empty set), ``dist_min`` (+inf), ``sum`` = sum of exp(z - zmax) (0),
    ``entropy`` in nats (0), ``logp_gold`` (None without gold) and the ``scale`` they were taken at."""
    __slots__ = ()

    @property
    def confidence(self) -> torch.Tensor:
        """The top-1 probability 1 / sum; 0 where the candidate set is empty."""
        return torch.where(self.sum > 0, 1.0 / self.sum.clamp_min(1.0), torch.zeros_like(self.sum))

    @property
    def lse(self) -> torch.Tensor:
        """log sum_n exp(-scale * dist[b, n]) = -scale * dist_min + log(sum); -inf where the candidate set is empty."""
        return torch.where(self.sum > 0, -self.scale * self.dist_min + torch.log(self.sum), torch.full_like(self.sum, float("-inf")))


def _check_scale(who: str, scale) -> float:
    import math
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError("%s: scale must be finite and > 0 (got %r)" % (who, scale))
    return scale


def _link_stats_call(who: str, name: str, ws_name: str, head_args, ws_args, N: int, nrel: int, dev, e_index, r_index, scale, gold,
                     index, pred_head: bool) -> LinkStats:
    """The statistics entry point ``name`` on prepared tables (``head_args``: the arguments before h; ``ws_args``: those of the
    workspace query after B, N, d)."""
    scale = _check_scale(who, scale)
    h = _query_column(e_index, N, "e_index", dev)
    r = _query_column(r_index, nrel, "r_index", dev)
    B = h.numel()
    g = None if gold is None else _query_column(gold, N, "gold", dev)
    if r.numel() != B or (g is not None and g.numel() != B):
        raise ValueError("%s: e_index, r_index and gold must have one entry per query" % who)
    near = torch.empty(B, dtype=torch.int32, device=dev)
    dmin, lsum, ent = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
    logp = torch.empty(B, dtype=torch.float32, device=dev) if g is not None else None
    L = lib()
    d = ws_args[0]
    ws_bytes = int(getattr(L, ws_name)(B, N, *ws_args))
    ws = workspace(ws_bytes, dev)
    ix, _keep_ix = _tail_index(index, dev)
    check(getattr(L, name)(*head_args, ptr(h), ptr(r), 1 if pred_head else 0, ptr(g), ix, B, N, d, scale, ptr(near), ptr(dmin),
                           ptr(lsum), ptr(ent), ptr(logp), ptr(ws), ws_bytes, stream()), name)
    return LinkStats(near.to(torch.int64), dmin, lsum, ent, logp, scale)


def linkpred_stats(comp_layers: Sequence[torch.Tensor], comp_rel_layers: Sequence[torch.Tensor], e_index, r_index, scale: float,
                   gold=None, index=None, pred_head: bool = False, table_dtype=torch.float32) -> LinkStats:
    """How sure the model is: the statistics of ``softmax(-scale * dist)`` over the tails of every ``(h, r)``, dist being
    linkpred_ranks' / linkpred_topk's distance bit for bit, without the [B, N] matrix.  Without ``gold`` the candidates are
    those ``index`` (a sampling.TrueTailIndex) does not list -- linkpred_topk's set; with ``gold`` the gold tail joins them even
    where listed -- the filtered ranks' set -- and ``logp_gold`` is its log-probability.  Listed tails are masked before the
    sums, never subtracted.  ``scale`` > 0 is the temperature (``harness.calibrate_link_scale`` fits it)."""
    _check_scale("linkpred_stats", scale)
    bf16 = table_dtype == torch.bfloat16
    arr, keep, N, d = _link_layers(comp_layers, comp_rel_layers, bf16)
    nl = len(comp_layers)
    return _link_stats_call("linkpred_stats", "jmac_linkpred_stats_bf16" if bf16 else "jmac_linkpred_stats_f32",
                            "jmac_linkpred_stats_workspace_bytes", (arr, nl), (d, nl), N, comp_rel_layers[0].shape[0],
                            comp_layers[0].device, e_index, r_index, scale, gold, index, pred_head)


def linkpred_stats_ensemble(members, e_index, r_index, scale: float, gold=None, index=None, pred_head: bool = False) -> LinkStats:
    """linkpred_stats on the cross-KG ensemble distance D of linkpred_ranks_ensemble (``members`` as there; ``index`` is the
    TARGET's).  One member with weight 1 gives linkpred_stats' bits."""
    _check_scale("linkpred_stats_ensemble", scale)
    arr, keep, N, d, nl, nrel = _link_members(members, "linkpred_stats_ensemble")
    return _link_stats_call("linkpred_stats_ensemble", "jmac_linkpred_ens_stats_f32", "jmac_linkpred_ens_stats_workspace_bytes",
                            (arr, len(members), nl), (d, nl, len(members)), N, nrel, members[0][0][0].device, e_index, r_index, scale,
                            gold, index, pred_head)


def _topk_prob(idx: torch.Tensor, dist: torch.Tensor, st: LinkStats) -> torch.Tensor:
    """prob[b, j] = exp(-scale (dist[b, j] - dist_min[b])) / sum[b]; padded entries (idx = -1) get 0."""
    pad = idx < 0
    u = -st.scale * (dist.masked_fill(pad, 0.0) - st.dist_min.masked_fill(st.sum <= 0, 0.0)[:, None])
    return (torch.exp(u) / st.sum.clamp_min(1.0)[:, None]).masked_fill(pad, 0.0)


def linkpred_topk_prob(comp_layers: Sequence[torch.Tensor], comp_rel_layers: Sequence[torch.Tensor], e_index, r_index, k: int,
                       scale: float, index=None, pred_head: bool = False, table_dtype=torch.float32):
    """``(idx, dist, prob)``: linkpred_topk's predictions with their probabilities under ``softmax(-scale * dist)`` over ALL
    unlisted candidates (one top-k call and one linkpred_stats call in prediction mode); padded entries have ``prob = 0``."""
    _check_scale("linkpred_topk_prob", scale)
    idx, dist = linkpred_topk(comp_layers, comp_rel_layers, e_index, r_index, k, index=index, pred_head=pred_head, table_dtype=table_dtype)
    st = linkpred_stats(comp_layers, comp_rel_layers, e_index, r_index, scale, index=index, pred_head=pred_head, table_dtype=table_dtype)
    return idx, dist, _topk_prob(idx, dist, st)


def linkpred_topk_prob_ensemble(members, e_index, r_index, k: int, scale: float, index=None, pred_head: bool = False):
    """linkpred_topk_prob on the cross-KG ensemble distance."""
    _check_scale("linkpred_topk_prob_ensemble", scale)
    idx, dist = linkpred_topk_ensemble(members, e_index, r_index, k, index=index, pred_head=pred_head)
    st = linkpred_stats_ensemble(members, e_index, r_index, scale, index=index, pred_head=pred_head)
    return idx, dist, _topk_prob(idx, dist, st)


def build_filter_csr(heads, rels, true_tail: Dict, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pack er_vocab[(h, r)] lists (src/validate.py:53; knowledgegraph.py:62-86) as CSR over the batch."""
    ptr_l, idx = [0], []
    for h, r in zip(heads, rels):
        tails = np.unique(np.asarray(true_tail.get((int(h), int(r)), []), dtype=np.int64))
        idx.extend(tails.tolist())
        ptr_l.append(len(idx))
    return (torch.tensor(ptr_l, dtype=torch.int32, device=device),
            torch.tensor(idx if idx else [0], dtype=torch.int32, device=device))


def filtered_rank(dist: torch.Tensor, gold, filt_ptr: Optional[torch.Tensor] = None,
                  filt_idx: Optional[torch.Tensor] = None, descending: bool = False) -> torch.Tensor:
    """1-based rank of the gold tail under ascending distance (``descending``: under descending similarity); filtered
    entries are skipped.  Ties: an equal score counts as ranked before the gold iff its index is lower."""
    require_device(dist)
    if dist.dtype != torch.float32 or dist.stride(1) != 1:
        raise TypeError("dist must be fp32 with unit column stride")
    B, N = dist.shape
    check_index_range(gold, N, "gold")
    gold = torch.as_tensor(gold, device=dist.device).to(torch.int32).contiguous()
    rank = torch.empty(B, dtype=torch.int32, device=dist.device)
    check(lib().jmac_filtered_rank_f32(ptr(dist), dist.stride(0), ptr(gold), ptr(filt_ptr), ptr(filt_idx), B, N,
                                       1 if descending else 0, ptr(rank), stream()), "jmac_filtered_rank_f32")
    return rank


def sim_matrix(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a @ b.T on the fp32-input MFMA (exact fp32 products).  ``out``: optional preallocated [M, N] fp32 result."""
    require_device(a, b)
    a, b = _rows16(a), _rows16(b)
    M, d = a.shape
    N = b.shape[0]
    c = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=a.device)
    if c.shape != (M, N) or c.dtype != torch.float32 or not c.is_contiguous():
        raise ValueError("sim_matrix: out must be a contiguous fp32 [%d, %d] tensor" % (M, N))
    check(lib().jmac_sim_matrix_f32(ptr(a), d, ptr(b), d, M, N, d, ptr(c), N, stream()), "jmac_sim_matrix_f32")
    return c


def sim_topk(a: torch.Tensor, b: torch.Tensor, k: int, return_values: bool = False, screen: Optional[str] = None,
             return_stats: bool = False):
    """Indices [L,k] (int64) of the k most similar rows of b for every row of a (descending; ties -> lower index).

    ``screen="bf16"``: the same indices and values bit for bit from ``jmac_sim_topk_screened_f32`` -- the bf16 matrix cores
    decide which columns can be among a row's k best, those are rescored with the fp32 product's own instructions (row length
    <= 512).  ``return_stats`` (screened form only) appends a dict: mean / max columns rescored per row, the rows whose list
    overflowed and recomputed, and whether the shape was screened at all (one host read)."""
    if screen not in (None, "bf16"):
        raise ValueError("sim_topk: screen must be None or 'bf16', not %r" % (screen,))
    if return_stats and screen is None:
        raise ValueError("sim_topk: return_stats needs screen='bf16'")
    require_device(a, b)
    a, b = _rows16(a), _rows16(b)
    L_, d = a.shape
    N = b.shape[0]
    L = lib()
    idx = torch.empty((L_, k), dtype=torch.int32, device=a.device)
    val = torch.empty((L_, k), dtype=torch.float32, device=a.device) if return_values else None
    stats = None
    if screen is None:
        ws_bytes = int(L.jmac_sim_topk_workspace_bytes(L_, N, int(k)))
        ws = workspace(ws_bytes, a.device)
        check(L.jmac_sim_topk_f32(ptr(a), d, ptr(b), d, L_, N, d, int(k), ptr(val), ptr(idx), ptr(ws), ws_bytes, stream()),
              "jmac_sim_topk_f32")
    else:
        nres = torch.empty(L_, dtype=torch.int32, device=a.device) if return_stats else None
        ws_bytes = int(L.jmac_sim_topk_screened_workspace_bytes(L_, N, d, int(k)))
        ws = workspace(ws_bytes, a.device)
        check(L.jmac_sim_topk_screened_f32(ptr(a), d, ptr(b), d, L_, N, d, int(k), ptr(val), ptr(idx), ptr(nres), ptr(ws),
                                           ws_bytes, stream()), "jmac_sim_topk_screened_f32")
        if return_stats:
            stats = _screen_stats(nres)
    idx = idx.to(torch.int64)
    out = (idx, val) if return_values else idx
    if return_stats:
        return out + (stats,) if return_values else (out, stats)
    return out


def row_topk(s: torch.Tensor, k: int):
    require_device(s)
    s = s.contiguous()
    L_, N = s.shape
    idx = torch.empty((L_, k), dtype=torch.int32, device=s.device)
    val = torch.empty((L_, k), dtype=torch.float32, device=s.device)
    check(lib().jmac_row_topk_f32(ptr(s), N, L_, N, int(k), ptr(val), ptr(idx), stream()), "jmac_row_topk_f32")
    return val, idx.to(torch.int64)


COL_TOPK_KMAX = 16


def col_topk_values(s: torch.Tensor, k: int) -> torch.Tensor:
    """The k largest values of every column of s, [n2, k] descending == ``row_topk(s.t().contiguous(), k)[0]`` without
    the transpose (k <= 16; larger k takes the transposing path)."""
    require_device(s)
    s = s.contiguous()
    n1, n2 = s.shape
    if k > COL_TOPK_KMAX:
        return row_topk(s.t().contiguous(), k)[0]
    val = torch.empty((n2, k), dtype=torch.float32, device=s.device)
    L = lib()
    wsb = int(L.jmac_col_topk_workspace_bytes(n1, n2, int(k)))
    ws = workspace(wsb, s.device)
    check(L.jmac_col_topk_f32(ptr(s), n2, n1, n2, int(k), ptr(val), ptr(ws), wsb, stream()), "jmac_col_topk_f32")
    return val


def get_neg(ILL, emb_src: torch.Tensor, emb_dst: torch.Tensor, k: int, screen: Optional[str] = None) -> torch.Tensor:
    """Same contract as modules/utils/util.py:31-54: flattened [len(ILL)*k] int64 indices into emb_dst.  ``screen``: as
    ``sim_topk``'s (the same indices either way)."""
    ill = torch.as_tensor(ILL, dtype=torch.long, device=emb_src.device)
    return sim_topk(emb_src.index_select(0, ill), emb_dst, k, screen=screen).reshape(-1)


def align_entropy(e1: torch.Tensor, e2: torch.Tensor, scale: float = 20.0):
    """(entropy, row entropies [n1], column entropies [n2]) of softmax(scale * e1 e2^T)."""
    require_device(e1, e2)
    e1, e2 = _rows16(e1), _rows16(e2)
    n1, d = e1.shape
    n2 = e2.shape[0]
    L = lib()
    hr = torch.empty(n1, dtype=torch.float32, device=e1.device)
    hc = torch.empty(n2, dtype=torch.float32, device=e1.device)
    ws_bytes = int(L.jmac_softmax_entropy_workspace_bytes(n1, n2))
    ws = workspace(ws_bytes, e1.device)
    check(L.jmac_softmax_entropy_f32(ptr(e1), d, ptr(e2), d, n1, n2, d, float(scale), ptr(hr), ptr(hc), ptr(ws), ws_bytes,
                                     stream()), "jmac_softmax_entropy_f32")
    return hr.mean() + hc.mean(), hr, hc


def masked_row_softmax(s: torch.Tensor, row_mask: Optional[torch.Tensor], col_mask: Optional[torch.Tensor],
                       fill: float = -1.0, scale: float = 20.0) -> torch.Tensor:
    return row_softmax(s, row_mask, col_mask, fill, scale)[0]


def _mask8(m: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return m.to(torch.uint8).contiguous() if m is not None else None


def row_softmax(s: torch.Tensor, row_mask=None, col_mask=None, fill: float = -1.0, scale: float = 20.0,
                want_out: bool = True, want_entropy: bool = False):
    """softmax over each row of ``where(keep, s, fill) * scale`` (keep = row_mask[i] & col_mask[j]; None = all):
    (probabilities [n1,n2] or None, row entropies [n1] or None)."""
    require_device(s)
    s = s.contiguous()
    n1, n2 = s.shape
    out = torch.empty_like(s) if want_out else None
    ent = torch.empty(n1, dtype=torch.float32, device=s.device) if want_entropy else None
    rm, cm = _mask8(row_mask), _mask8(col_mask)
    check(lib().jmac_row_softmax_f32(ptr(s), n2, n1, n2, ptr(rm), ptr(cm), float(fill), float(scale), ptr(out), n2, ptr(ent),
                                     stream()), "jmac_row_softmax_f32")
    return out, ent


def col_softmax(s: torch.Tensor, row_mask=None, col_mask=None, fill: float = -1.0, scale: float = 20.0,
                want_out: bool = True, want_entropy: bool = False):
    """softmax over each COLUMN of the same masked, scaled matrix, returned transposed:
    ``torch.softmax(where(keep, s, fill).t() * scale, dim=1)`` [n2,n1] (or None) and the column entropies [n2] (or None)
    -- from the row-major ``s`` itself, i.e. without the second, transposed similarity GEMM."""
    require_device(s)
    s = s.contiguous()
    n1, n2 = s.shape
    out_t = torch.empty((n2, n1), dtype=torch.float32, device=s.device) if want_out else None
    ent = torch.empty(n2, dtype=torch.float32, device=s.device) if want_entropy else None
    rm, cm = _mask8(row_mask), _mask8(col_mask)
    L = lib()
    wsb = int(L.jmac_col_softmax_workspace_bytes(n1, n2))
    ws = workspace(wsb, s.device)
    check(L.jmac_col_softmax_f32(ptr(s), n2, n1, n2, ptr(rm), ptr(cm), float(fill), float(scale), ptr(out_t), n1, ptr(ent),
                                 ptr(ws), wsb, stream()), "jmac_col_softmax_f32")
    return out_t, ent


def alignment_quality(emb1: torch.Tensor, emb2: torch.Tensor, list1, list2, scale: float = 20.0):
    """compute_alignment_quality, train.py:231-259: (entropy, softmax rows [N1,N2], softmax cols [N2,N1]).
    The O(N*T) python membership scans of :252-253 become boolean masks; each of the two similarity matrices
    (:239 and :250) is ONE GEMM, its transposed softmax (:245, :257) is a column pass over the same matrix."""
    dev = emb1.device
    l1 = torch.as_tensor(list1, dtype=torch.long, device=dev)
    l2 = torch.as_tensor(list2, dtype=torch.long, device=dev)
    entropy, _, _ = align_entropy(emb1.index_select(0, l1), emb2.index_select(0, l2), scale)
    m1 = torch.zeros(emb1.shape[0], dtype=torch.bool, device=dev)
    m1[l1] = True
    m2 = torch.zeros(emb2.shape[0], dtype=torch.bool, device=dev)
    m2[l2] = True
    simi = sim_matrix(emb1, emb2)
    return entropy, row_softmax(simi, m1, m2, -1.0, scale)[0], col_softmax(simi, m1, m2, -1.0, scale)[0]


SoftmaxStats = namedtuple("SoftmaxStats", "row_max row_arg row_sum row_ent col_max col_arg col_sum col_ent")


def sim_softmax_stats(a: torch.Tensor, b: torch.Tensor, scale: float = 20.0, cols: bool = True) -> SoftmaxStats:
    """Per row (and, with ``cols``, per column) of S = a @ b.T, which is never written: the maximum (bit-identical to
    ``sim_matrix(a, b).max``), its first index (int32), sum_j e^(scale (S - max)) and the entropy of softmax(scale S).
    ``cols=False`` leaves the four column fields None."""
    require_device(a, b)
    a, b = _rows16(a), _rows16(b)
    n1, d = a.shape
    n2 = b.shape[0]
    if n1 == 0 or n2 == 0:
        raise ValueError("sim_softmax_stats: empty operand")
    dev = a.device

    def vec(n, dtype=torch.float32):
        return torch.empty(n, dtype=dtype, device=dev)
    r = [vec(n1), vec(n1, torch.int32), vec(n1), vec(n1)]
    c = [vec(n2), vec(n2, torch.int32), vec(n2), vec(n2)] if cols else [None] * 4
    L = lib()
    ws_bytes = int(L.jmac_sim_softmax_stats_workspace_bytes(n1, n2))
    ws = workspace(ws_bytes, dev)
    check(L.jmac_sim_softmax_stats_f32(ptr(a), d, ptr(b), d, n1, n2, d, float(scale), *[ptr(t) for t in r + c], ptr(ws), ws_bytes,
                                       stream()), "jmac_sim_softmax_stats_f32")
    return SoftmaxStats(*(r + c))


def _sim_lse_call(a, b, scale, col_add, row_add, row_shift, col_shift, row_out, col_out, ws, ws_bytes):
    """One jmac_sim_lse_f32 launch on prepared operands (``_rows16``) and caller-held vectors and workspace."""
    d = a.shape[1]
    check(lib().jmac_sim_lse_f32(ptr(a), d, ptr(b), d, a.shape[0], b.shape[0], d, float(scale), ptr(col_add), ptr(row_add),
                                 float(row_shift), float(col_shift), ptr(row_out), ptr(col_out), ptr(ws), ws_bytes, stream()),
          "jmac_sim_lse_f32")


def _offsets(v, n: int, what: str, dev):
    if v is None:
        return None
    v = v.contiguous()
    if v.shape != (n,) or v.dtype != torch.float32 or v.device != dev:
        raise ValueError("%s must be an fp32 vector of %d entries on the operands' device" % (what, n))
    return v


def sim_lse(a: torch.Tensor, b: torch.Tensor, scale: float, col_add=None, row_add=None, row_shift: float = 0.0,
            col_shift: float = 0.0, rows: bool = True, cols: bool = True):
    """``(row_out | None, col_out | None)`` of S = a @ b.T, which is never written (jmac_sim_lse_f32):
    ``row_out[i] = row_shift - log sum_j exp(scale S[i, j] + col_add[j])`` and
    ``col_out[j] = col_shift - log sum_i exp(scale S[i, j] + row_add[i])``; an absent offset vector is 0, the given ones must be
    finite.  A side that is not asked for (``rows`` / ``cols``) costs no epilogue work; the other side's bits do not change."""
    require_device(a, b)
    a, b = _rows16(a), _rows16(b)
    n1, n2 = a.shape[0], b.shape[0]
    if n1 == 0 or n2 == 0:
        raise ValueError("sim_lse: empty operand")
    if a.shape[1] != b.shape[1]:
        raise ValueError("sim_lse: the operands disagree in width")
    if not (rows or cols):
        raise ValueError("sim_lse: at least one of rows / cols")
    if not scale > 0:
        raise ValueError("sim_lse: scale must be positive")
    dev = a.device
    col_add, row_add = _offsets(col_add, n2, "col_add", dev), _offsets(row_add, n1, "row_add", dev)
    row_out = torch.empty(n1, dtype=torch.float32, device=dev) if rows else None
    col_out = torch.empty(n2, dtype=torch.float32, device=dev) if cols else None
    ws_bytes = int(lib().jmac_sim_lse_workspace_bytes(n1, n2))
    _sim_lse_call(a, b, scale, col_add, row_add, row_shift, col_shift, row_out, col_out, workspace(ws_bytes, dev), ws_bytes)
    return row_out, col_out


def _best_with_constant(x: torch.Tensor, l: torch.Tensor, arg: torch.Tensor, index_of: torch.Tensor, c: int, first_masked: int,
                        fill: float, scale: float):
    """Largest softmax entry and its index for lines of the masked matrix: ``x`` / ``l`` / ``arg`` are the maximum, the sum
    e^(scale (s - x)) and the arg-max over the line's KEPT entries (positions into ``index_of``, ascending ids), and ``c`` further
    entries, the lowest of them at index ``first_masked``, all hold ``fill``."""
    idx = index_of[arg.long()]
    if c == 0:
        return 1.0 / l, idx
    f = torch.full_like(x, fill)
    M = torch.maximum(x, f)
    denom = l * torch.exp(scale * (x - M)) + c * torch.exp(scale * (f - M))
    fm = torch.full_like(idx, first_masked)
    idx = torch.where(x < f, fm, torch.where(x == f, torch.minimum(idx, fm), idx))     # first maximum of the masked line
    return 1.0 / denom, idx


def _first_missing(sorted_ids: np.ndarray, n: int) -> int:
    """The lowest id in [0, n) that ``sorted_ids`` (ascending, distinct) does not list; n if it lists all."""
    gap = np.nonzero(sorted_ids != np.arange(len(sorted_ids)))[0]
    return int(gap[0]) if len(gap) else len(sorted_ids)


def alignment_stats(emb1: torch.Tensor, emb2: torch.Tensor, list1, list2, scale: float = 20.0):
    """What the EnTr refresh reads of compute_alignment_quality (train.py:231-259, consumer :160-169) WITHOUT its matrices:
    ``(entropy, row_best_prob [N1], row_best [N1] int64, col_best_prob [N2], col_best [N2] int64)`` with
    ``row_best_prob, row_best == alignment_quality(...)[1].max(1)`` and ``col_* == alignment_quality(...)[2].max(1)``.

    Outside list1 x list2 the masked matrix holds the constant f = -1, so a kept row with maximum x and sum
    l = sum e^(scale (s - x)) over its |list2| kept entries and c = N2 - |set(list2)| constant ones has
    M = max(x, f), best probability 1 / (l e^(scale (x - M)) + c e^(scale (f - M))); a row outside list1 is all-equal:
    1 / N2 at index 0.  Everything comes from ONE statistics launch on the n1 x n2 sub-product (``sim_softmax_stats``); a list
    with repeated entries takes a second one, because the entropy half counts a repeated entity as often as it is listed
    (train.py:236-237) and the masked half once.  ``list1`` / ``list2`` are host sequences."""
    require_device(emb1, emb2)
    dev = emb1.device
    N1, N2 = emb1.shape[0], emb2.shape[0]
    l1, l2 = np.asarray(list1, dtype=np.int64).reshape(-1), np.asarray(list2, dtype=np.int64).reshape(-1)
    if not len(l1) or not len(l2):
        raise ValueError("alignment_stats: empty list")
    check_index_range(l1, N1, "list1")
    check_index_range(l2, N2, "list2")
    u1, u2 = np.unique(l1), np.unique(l2)                       # ascending: the kernel's lowest position is the lowest id
    t1, t2 = torch.from_numpy(u1).to(dev), torch.from_numpy(u2).to(dev)
    st = sim_softmax_stats(emb1.index_select(0, t1), emb2.index_select(0, t2), scale)
    if len(u1) == len(l1) and len(u2) == len(l2):               # a permutation of the listed rows: the same means
        entropy = st.row_ent.mean() + st.col_ent.mean()
    else:
        se = sim_softmax_stats(emb1.index_select(0, torch.from_numpy(l1).to(dev)), emb2.index_select(0, torch.from_numpy(l2).to(dev)),
                               scale)
        entropy = se.row_ent.mean() + se.col_ent.mean()
    row_p = torch.full((N1,), 1.0 / N2, dtype=torch.float32, device=dev)
    row_i = torch.zeros(N1, dtype=torch.int64, device=dev)
    col_p = torch.full((N2,), 1.0 / N1, dtype=torch.float32, device=dev)
    col_i = torch.zeros(N2, dtype=torch.int64, device=dev)
    p, i = _best_with_constant(st.row_max, st.row_sum, st.row_arg, t2, N2 - len(u2), _first_missing(u2, N2), -1.0, scale)
    row_p[t1], row_i[t1] = p, i
    p, i = _best_with_constant(st.col_max, st.col_sum, st.col_arg, t1, N1 - len(u1), _first_missing(u1, N1), -1.0, scale)
    col_p[t2], col_i[t2] = p, i
    return entropy, row_p, row_i, col_p, col_i


# ---- DBPv1 call sites (row a18): ONE embedding table on both sides ------------------------------------------------
def get_neg_dbpv1(ILL, output_layer: torch.Tensor, k: int, screen: Optional[str] = None) -> torch.Tensor:
    """get_neg(ILL, output_layer, k), JMAC_DBPv1/modules/utils/util.py:35-58: the k most similar rows of the WHOLE
    table (own KG and the entity itself included) for every entity of ILL, flattened [len(ILL)*k] int64."""
    return get_neg(ILL, output_layer, output_layer, k, screen=screen)


def alignment_quality_dbpv1(embedding: torch.Tensor, list1, list2, scale: float = 20.0):
    """Trainer.compute_alignment_quality(embedding, list1, list2), JMAC_DBPv1/trainer/jmac_trainer.py:281-300:
    (entropy, softmax(simi*20, dim=1) [T1,T2], softmax(simi.t()*20, dim=1) [T2,T1]) with simi = E[list1] E[list2]^T.
    One similarity GEMM; the row pass yields softmax + row entropies, the column pass the transposed softmax +
    column entropies."""
    dev = embedding.device
    l1 = torch.as_tensor(list1, dtype=torch.long, device=dev)
    l2 = torch.as_tensor(list2, dtype=torch.long, device=dev)
    simi = sim_matrix(embedding.index_select(0, l1), embedding.index_select(0, l2))
    p_rows, h_rows = row_softmax(simi, None, None, 0.0, scale, True, True)
    p_cols, h_cols = col_softmax(simi, None, None, 0.0, scale, True, True)
    return h_rows.mean() + h_cols.mean(), p_rows, p_cols


def alignment_stats_dbpv1(embedding: torch.Tensor, list1, list2, scale: float = 20.0):
    """The [T1, T2] form of ``alignment_stats`` (no mask): ``(entropy, p_rows.max(1) values [T1], indices [T1] int64,
    p_cols.max(1) values [T2], indices [T2] int64)`` of ``alignment_quality_dbpv1`` from one statistics launch."""
    dev = embedding.device
    l1 = torch.as_tensor(list1, dtype=torch.long, device=dev)
    l2 = torch.as_tensor(list2, dtype=torch.long, device=dev)
    st = sim_softmax_stats(embedding.index_select(0, l1), embedding.index_select(0, l2), scale)
    return (st.row_ent.mean() + st.col_ent.mean(), 1.0 / st.row_sum, st.row_arg.long(), 1.0 / st.col_sum, st.col_arg.long())


# ---- alignment evaluation (next row f1: modules/finding/similarity.py:13-84, alignment.py:10-112) -------------
def csls_sim(sim: torch.Tensor, k: int) -> torch.Tensor:
    """csls_sim, similarity.py:58-78, with calculate_nearest_k defined as the exact mean of the k largest entries
    (the reference's np.partition(-sim, k+1)[:, :k] returns *some* k of the top k+1)."""
    require_device(sim)
    sim = sim.contiguous()
    n1, n2 = sim.shape
    r1 = row_topk(sim, k)[0].mean(1)
    r2 = col_topk_values(sim, k).mean(1)
    out = torch.empty_like(sim)
    check(lib().jmac_csls_apply_f32(ptr(sim), n2, n1, n2, ptr(r1), ptr(r2), ptr(out), n2, stream()), "jmac_csls_apply_f32")
    return out


def csls_rank(sim: torch.Tensor, k: int, gold) -> torch.Tensor:
    """1-based rank of column gold[i] in row i of ``csls_sim(sim, k)`` (descending, ties -> lower index first) without
    materialising the rescored matrix: the same r1 / r2 and the same ``2 s - r1 - r2`` arithmetic, consumed by the count."""
    require_device(sim)
    sim = sim.contiguous()
    n1, n2 = sim.shape
    r1 = row_topk(sim, k)[0].mean(1)
    r2 = col_topk_values(sim, k).mean(1)
    check_index_range(gold, n2, "gold")
    gold = torch.as_tensor(gold, device=sim.device).to(torch.int32).contiguous()
    rank = torch.empty(n1, dtype=torch.int32, device=sim.device)
    check(lib().jmac_csls_rank_f32(ptr(sim), n2, n1, n2, ptr(r1), ptr(r2), ptr(gold), ptr(rank), stream()), "jmac_csls_rank_f32")
    return rank


def _alignment_operands(embed1: torch.Tensor, embed2: torch.Tensor, metric: str, normalize: bool):
    """The two operands of sim() (similarity.py:13-55) for 'cosine', 'inner' (a product) and 'manhattan' (1 - L1 distance):
    L2-normalised rows for 'cosine' and under ``normalize``."""
    if normalize or metric == "cosine":
        from .ops import row_normalize
        return row_normalize(embed1.detach()), row_normalize(embed2.detach())
    if metric not in ("inner", "manhattan"):
        raise NotImplementedError("metric %r ('cosine', 'inner' and 'manhattan' are built; train.py:105-113 uses 'cosine')" % metric)
    return embed1, embed2


def _l1_metric(metric: str) -> bool:
    """Which machine a metric runs on: the L1 tile kernel ('manhattan') or the similarity product (every other one)."""
    return metric == "manhattan"


def alignment_sim(embed1: torch.Tensor, embed2: torch.Tensor, metric: str = "cosine", normalize: bool = False,
                  csls_k: int = 0) -> torch.Tensor:
    """sim(), similarity.py:13-55, for 'cosine', 'inner' and 'manhattan' (``1 - l1_scores``, similarity.py:47-49), stored."""
    embed1, embed2 = _alignment_operands(embed1, embed2, metric, normalize)
    s = 1.0 - l1_scores(embed1.detach(), embed2.detach()) if _l1_metric(metric) else sim_matrix(embed1, embed2)
    return csls_sim(s, csls_k) if csls_k > 0 else s


# ---- the same evaluation without the n1 x n2 matrix ------------------------------------------------------------------
CSLS_KMAX = 64


def _check_k(who: str, k, n2: int) -> int:
    k = int(k)
    if not 1 <= k <= CSLS_KMAX or k > n2:
        raise ValueError("%s: k must lie in [1, min(64, n2)] (got %d, n2 = %d)" % (who, k, n2))
    return k


def _check_screen(who: str, screen, metric: str = "inner"):
    """``screen`` is None or "bf16" (``sim_topk``'s rule); the L1 tile kernel has no bf16 form."""
    if screen not in (None, "bf16"):
        raise ValueError("%s: screen must be None or 'bf16', not %r" % (who, screen))
    if screen is not None and _l1_metric(metric):
        raise ValueError("%s: metric 'manhattan' has no screened form (screen must be None)" % who)


def _topk_bytes(metric: str, rows: int, n2: int, d: int, k: int, screen: Optional[str] = None) -> int:
    """Workspace bytes of the fused top-k of ``rows`` rows on the machine ``metric`` runs on (``screen``: of its screened form)."""
    if _l1_metric(metric):
        return int(lib().jmac_l1_csls_topk_workspace_bytes(rows, n2, d, k))
    if screen is not None:
        return int(lib().jmac_sim_csls_topk_screened_workspace_bytes(rows, n2, d, k))
    return int(lib().jmac_sim_csls_topk_workspace_bytes(rows, n2, k))


def _csls_topk(a: torch.Tensor, b: torch.Tensor, k: int, r1=None, r2=None, metric: str = "inner", row_id=None, best=None, ws=None,
               screen: Optional[str] = None, n_rescored: Optional[torch.Tensor] = None):
    """(idx int32 [n1, k], val fp32 [n1, k]) of jmac_{sim,l1}_csls_topk_f32 -- with ``best`` (and ``row_id``) of the _viable_f32 form --
    on prepared operands (``_rows16``).  ``ws``: a caller-held workspace of at least ``_topk_bytes`` bytes, whose head is used.
    ``screen="bf16"``: the same bits from the _screened_f32 forms; ``n_rescored`` (int32 [n1], optional) takes their per-row counts."""
    _check_screen("_csls_topk", screen, metric)
    n1, d = a.shape
    n2 = b.shape[0]
    idx = torch.empty((n1, k), dtype=torch.int32, device=a.device)
    val = torch.empty((n1, k), dtype=torch.float32, device=a.device)
    ws_bytes = _topk_bytes(metric, n1, n2, d, k, screen)
    ws = workspace(ws_bytes, a.device) if ws is None else ws
    name = ("jmac_l1_csls_topk" if _l1_metric(metric) else "jmac_sim_csls_topk") + ("" if best is None else "_viable") + \
        ("_f32" if screen is None else "_screened_f32")
    viable = () if best is None else (ptr(row_id), ptr(best))
    counts = () if screen is None else (ptr(n_rescored),)
    check(getattr(lib(), name)(ptr(a), d, ptr(b), d, n1, n2, d, ptr(r1), ptr(r2), *viable, k, ptr(val), ptr(idx), *counts, ptr(ws),
                               ws_bytes, stream()), name)
    return idx, val


def _screen_stats(n_rescored: torch.Tensor) -> dict:
    """``sim_topk``'s statistics dict from a screened entry's per-row counts (one host read)."""
    n = n_rescored.cpu()
    seen = n[n >= 0].to(torch.float64)
    return dict(rows=int(n.numel()), screened=bool(n.numel() == 0 or int(n.min()) > -2), overflow_rows=int((n == -1).sum()),
                rescored_mean=float(seen.mean()) if len(seen) else 0.0, rescored_max=int(seen.max()) if len(seen) else 0,
                n_rescored=n)


def csls_terms(a: torch.Tensor, b: torch.Tensor, csls_k: int, metric: str = "inner",
               screen: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(r1 [n1], r2 [n2])`` of csls_sim (similarity.py:58-78) for S = a @ b.T, which is never written: r1[i] is the mean of
    the ``csls_k`` largest entries of row i, r2[j] of column j.  Two fused top-k products: ``sim_topk(a, b)`` for the rows,
    ``sim_topk(b, a)`` for the columns -- every element of b a^T is the same commuting products in the same contraction order
    as the transposed element of a b^T, so both equal the stored forms (``row_topk(sim_matrix(a, b), k)[0].mean(1)``,
    ``col_topk_values(sim_matrix(a, b), k).mean(1)``) bit for bit.  1 <= csls_k <= 64.
    ``metric="manhattan"``: the same terms of S = 1 - l1_scores(a, b) from two fused L1 top-k passes; |x - y| == |y - x| and the
    sum runs over k in the same order from either side, so the transposed pass has the stored matrix's bits as well.
    ``screen="bf16"``: both products through ``sim_topk``'s screened form -- the same terms bit for bit."""
    _check_screen("csls_terms", screen, metric)
    csls_k = int(csls_k)
    if not 1 <= csls_k <= CSLS_KMAX or csls_k > min(a.shape[0], b.shape[0]):
        raise ValueError("csls_terms: csls_k must lie in [1, min(%d, n1, n2)] (got %d)" % (CSLS_KMAX, csls_k))
    if _l1_metric(metric):
        require_device(a, b)
        a, b = _rows16(a.detach()), _rows16(b.detach())
        return _csls_topk(a, b, csls_k, metric=metric)[1].mean(1), _csls_topk(b, a, csls_k, metric=metric)[1].mean(1)
    r1 = sim_topk(a, b, csls_k, return_values=True, screen=screen)[1].mean(1)
    r2 = sim_topk(b, a, csls_k, return_values=True, screen=screen)[1].mean(1)
    return r1, r2


def sinkhorn_potentials(emb1: torch.Tensor, emb2: torch.Tensor, scale: float = 50.0, iters: int = 10, metric: str = "cosine",
                        normalize: bool = False, tol: Optional[float] = None):
    """``(f fp32 [n1], g fp32 [n2], stats)``: the potentials of the log-domain Sinkhorn plan with uniform marginals,
    ``log P[i, j] = scale S[i, j] + f[i] + g[j]`` for S = the similarity of ``alignment_sim`` ('cosine', 'inner'), without the
    n1 x n2 matrix.  From f = g = 0, ``iters`` times  f <- -log n1 - LSE_j(scale S + g),  g <- -log n2 - LSE_i(scale S + f): every
    half-step is ONE jmac_sim_lse_f32 launch that writes f or g in place of the old one (the shifts carry the marginals), so an
    iteration is two full products and no element-wise launch.  The run ends on a g update: the column sums of P are 1 / n2 to
    rounding.  ``stats``: iters (done) and residual = max_i |f_new - f_old| of the last row step.  ``tol``: stop after the first
    iteration whose residual is <= tol (one host read per iteration; a default run has none)."""
    if _l1_metric(metric):
        raise NotImplementedError("sinkhorn_potentials: metric 'manhattan' is not built ('cosine' and 'inner' are)")
    iters = int(iters)
    if iters < 1:
        raise ValueError("sinkhorn_potentials: iters must be at least 1")
    if not scale > 0:
        raise ValueError("sinkhorn_potentials: scale must be positive")
    require_device(emb1, emb2)
    a, b = _alignment_operands(emb1, emb2, metric, normalize)
    a, b = _rows16(a.detach()), _rows16(b.detach())
    n1, n2 = a.shape[0], b.shape[0]
    if n1 == 0 or n2 == 0:
        raise ValueError("sinkhorn_potentials: empty operand")
    if a.shape[1] != b.shape[1]:
        raise ValueError("the two embedding tables disagree in width")
    dev = a.device
    f, f_old = torch.zeros(n1, dtype=torch.float32, device=dev), torch.zeros(n1, dtype=torch.float32, device=dev)
    g = torch.zeros(n2, dtype=torch.float32, device=dev)
    ws_bytes = int(lib().jmac_sim_lse_workspace_bytes(n1, n2))
    ws = workspace(ws_bytes, dev)
    row_shift, col_shift = -float(np.log(n1)), -float(np.log(n2))
    done, residual = 0, None
    for _ in range(iters):
        f, f_old = f_old, f                                            # the row step writes the buffer of two steps ago
        _sim_lse_call(a, b, scale, g, None, row_shift, 0.0, f, None, ws, ws_bytes)
        # g is read by nothing in its own launch (the column side adds f): written in place
        _sim_lse_call(a, b, scale, None, f, 0.0, col_shift, None, g, ws, ws_bytes)
        done += 1
        if tol is not None:
            residual = float((f - f_old).abs().max().item())
            if residual <= tol:
                break
    if residual is None:
        residual = float((f - f_old).abs().max().item())
    return f, g, {"iters": done, "residual": residual}


def sinkhorn_terms(emb1: torch.Tensor, emb2: torch.Tensor, scale: float = 50.0, iters: int = 10, metric: str = "cosine",
                   normalize: bool = False, tol: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(r1, r2) = (-(2 / scale) f, -(2 / scale) g)`` of ``sinkhorn_potentials``: with them the rescored value the alignment
    kernels decide on, ``c = 2 S - r1 - r2``, is ``(2 / scale) log P`` -- ranks, top-k and the stable matching under the Sinkhorn
    plan come from ``alignment_ranks`` / ``alignment_topk`` / ``stable_alignment(..., csls_k=<any positive>, terms=(r1, r2))``."""
    f, g, _ = sinkhorn_potentials(emb1, emb2, scale, iters, metric, normalize, tol)
    w = -2.0 / float(scale)
    return f * w, g * w


def _csls_operands(emb1, emb2, csls_k, metric, normalize, terms, screen=None):
    require_device(emb1, emb2)
    a, b = _alignment_operands(emb1, emb2, metric, normalize)
    a, b = _rows16(a.detach()), _rows16(b.detach())
    if a.shape[1] != b.shape[1]:
        raise ValueError("the two embedding tables disagree in width")
    r1 = r2 = None
    if int(csls_k) > 0:
        r1, r2 = terms if terms is not None else csls_terms(a, b, csls_k, metric, screen)
        r1, r2 = r1.contiguous(), r2.contiguous()
        if r1.shape != (a.shape[0],) or r2.shape != (b.shape[0],) or r1.dtype != torch.float32 or r2.dtype != torch.float32:
            raise ValueError("terms must be fp32 vectors of n1 and n2 entries")
        require_device(r1, r2)
    return a, b, r1, r2


def alignment_ranks(emb1: torch.Tensor, emb2: torch.Tensor, gold, csls_k: int = 10, metric: str = "cosine",
                    normalize: bool = False, terms=None, screen: Optional[str] = None, return_stats: bool = False):
    """int32 ranks [n1]: the 1-based rank of column gold[i] in row i of ``alignment_sim(emb1, emb2, metric, normalize, csls_k)``
    (descending, ties -> lower index first) == ``csls_rank(sim_matrix(..), csls_k, gold)`` (``csls_k = 0``:
    ``filtered_rank(sim_matrix(..), gold, descending=True)``) bit for bit, without the n1 x n2 matrix: the count runs in the
    product's epilogue (``metric="manhattan"``: in the L1 tile kernel's, against ``1 - l1_scores``).  ``terms``: ``csls_terms`` of the
    same operands and metric, if the caller has them already -- or ``sinkhorn_terms``: the ranks are then those under the
    Sinkhorn plan (any positive ``csls_k``).
    ``screen="bf16"``: the same ranks bit for bit from jmac_sim_csls_rank_screened_f32 (the CSLS terms' two products screened as
    well; not for 'manhattan'; row length <= 512).  The bf16 matrix cores decide every column whose bounds lie on one side of the
    row's gold value; the undecided ones are rescored with the fp32 product's own instructions.  A row with more than 512 undecided
    columns (its gold sits in the bulk of the row) comes back unranked and is finished here by the fp32 entry on the gathered
    rows: such rows cost what they cost without the screen, on top of the screen's pass, so the screen pays for golds near the top
    of their rows -- a trained model's -- and is NOT expected to win when most golds are random.  One host read
    (are there unranked rows).  ``return_stats`` (screened form only) appends ``sim_topk``'s statistics dict; overflow_rows is the
    number of rows finished dense."""
    _check_screen("alignment_ranks", screen, metric)
    if return_stats and screen is None:
        raise ValueError("alignment_ranks: return_stats needs screen='bf16'")
    a, b, r1, r2 = _csls_operands(emb1, emb2, csls_k, metric, normalize, terms, screen)
    n1, d = a.shape
    n2 = b.shape[0]
    check_index_range(gold, n2, "gold")
    gold = torch.as_tensor(gold, device=a.device).to(torch.int32).contiguous()
    if gold.numel() != n1:
        raise ValueError("gold must have one entry per row of emb1")
    rank = torch.empty(n1, dtype=torch.int32, device=a.device)
    L = lib()
    if screen is not None:
        nres = torch.empty(n1, dtype=torch.int32, device=a.device)
        ws_bytes = int(L.jmac_sim_csls_rank_screened_workspace_bytes(n1, n2, d))
        ws = workspace(ws_bytes, a.device)
        check(L.jmac_sim_csls_rank_screened_f32(ptr(a), d, ptr(b), d, n1, n2, d, ptr(r1), ptr(r2), ptr(gold), ptr(rank), ptr(nres), 0,
                                                ptr(ws), ws_bytes, stream()), "jmac_sim_csls_rank_screened_f32")
        rows = (rank == 0).nonzero().flatten()                         # the host read: the rows whose list overflowed
        if rows.numel():
            sub = torch.empty(rows.numel(), dtype=torch.int32, device=a.device)
            ws_bytes = int(L.jmac_sim_csls_rank_workspace_bytes(rows.numel(), n2))
            ws = workspace(ws_bytes, a.device)
            # (held in names: a temporary would be freed, and its memory reused, before the launch that reads it)
            a_s, gold_s = a.index_select(0, rows).contiguous(), gold.index_select(0, rows).contiguous()
            r1s = None if r1 is None else r1.index_select(0, rows).contiguous()
            check(L.jmac_sim_csls_rank_f32(ptr(a_s), d, ptr(b), d, rows.numel(), n2, d, ptr(r1s), ptr(r2), ptr(gold_s), ptr(sub), ptr(ws),
                                           ws_bytes, stream()), "jmac_sim_csls_rank_f32")
            rank[rows] = sub
        return (rank, _screen_stats(nres)) if return_stats else rank
    name = "jmac_l1_csls_rank" if _l1_metric(metric) else "jmac_sim_csls_rank"
    ws_bytes = int(getattr(L, name + "_workspace_bytes")(n1, n2))
    ws = workspace(ws_bytes, a.device)
    check(getattr(L, name + "_f32")(ptr(a), d, ptr(b), d, n1, n2, d, ptr(r1), ptr(r2), ptr(gold), ptr(rank), ptr(ws), ws_bytes,
                                    stream()), name + "_f32")
    return rank


def alignment_topk(emb1: torch.Tensor, emb2: torch.Tensor, k: int, csls_k: int = 10, metric: str = "cosine",
                   normalize: bool = False, terms=None, screen: Optional[str] = None, return_stats: bool = False):
    """The alignment itself: ``(idx int64 [n1, k], val fp32 [n1, k])``, per row of emb1 the k best matches among the rows of emb2
    under ``alignment_sim(.., csls_k)``, best first (ties -> lower index first) == ``row_topk(alignment_sim(..), k)`` bit for
    bit, without the n1 x n2 matrix (greedy_alignment's alignment_rest, alignment.py:10-112, is column 0).  1 <= k <= 64.
    ``screen="bf16"``: the same result bit for bit from jmac_sim_csls_topk_screened_f32 (the CSLS terms' two products screened as
    well): the bf16 matrix cores rule columns out, the survivors are rescored with the fp32 product's own instructions (not for
    'manhattan'; row length <= 512).  ``return_stats`` (screened form only) appends ``sim_topk``'s statistics dict."""
    _check_screen("alignment_topk", screen, metric)
    if return_stats and screen is None:
        raise ValueError("alignment_topk: return_stats needs screen='bf16'")
    a, b, r1, r2 = _csls_operands(emb1, emb2, csls_k, metric, normalize, terms, screen)
    nres = torch.empty(a.shape[0], dtype=torch.int32, device=a.device) if return_stats else None
    idx, val = _csls_topk(a, b, _check_k("alignment_topk", k, b.shape[0]), r1, r2, metric, screen=screen, n_rescored=nres)
    if return_stats:
        return idx.to(torch.int64), val, _screen_stats(nres)
    return idx.to(torch.int64), val


# ---- stable one-to-one alignment (galeshapley, modules/finding/alignment.py:115-168, run to convergence) ---------------------------
class _StableState:
    """The device state of one deferred-acceptance run (jmac_stable_match_f32): candidate lists, list positions, the reviewers'
    words and the outputs.  ``step()`` runs the lists to their fixpoint and returns (exhausted, proposals) -- its one host read."""

    def __init__(self, idx: torch.Tensor, val: torch.Tensor, n2: int):
        dev = idx.device
        self.idx, self.val, self.n2 = idx, val, int(n2)
        self.n1, self.k = idx.shape
        self.ptr = torch.zeros(self.n1, dtype=torch.int32, device=dev)
        self.best = torch.zeros(self.n2, dtype=torch.int64, device=dev)          # the 64-bit words; 0 = free
        self.match1 = torch.empty(self.n1, dtype=torch.int32, device=dev)
        self.match2 = torch.empty(self.n2, dtype=torch.int32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self.ws_bytes = int(lib().jmac_stable_match_workspace_bytes(self.n1, self.n2))
        self.ws = workspace(self.ws_bytes, dev)

    def step(self) -> Tuple[int, int]:
        check(lib().jmac_stable_match_f32(ptr(self.idx), ptr(self.val), self.k, self.n1, self.n2, self.k, ptr(self.ptr), ptr(self.best),
                                          ptr(self.match1), ptr(self.match2), ptr(self.counters), ptr(self.ws), self.ws_bytes, stream()),
              "jmac_stable_match_f32")
        exhausted, proposals = self.counters.tolist()
        return int(exhausted), int(proposals)

    def exhausted_ids(self, n: int) -> torch.Tensor:
        """int32 [n], ascending (the kernel lists them in no particular order)"""
        return self.ws[:4 * n].view(torch.int32).sort().values


def _candidate_lists(idx: torch.Tensor, val: torch.Tensor, n2: int, what: str):
    require_device(idx, val)
    if idx.dim() != 2 or idx.shape != val.shape or val.dtype != torch.float32:
        raise ValueError("%s: idx and val must be [n1, k] tensors, val fp32" % what)
    _check_k(what, idx.shape[1], int(n2))
    return idx.to(torch.int32).contiguous(), val.contiguous()


def stable_matching(idx: torch.Tensor, val: torch.Tensor, n2: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(match1 int64 [n1], match2 int64 [n2])``: the suitor-optimal stable matching of the instance with exactly these incomplete
    lists (no refill).  Row i of ``idx`` [n1, k] names suitor i's acceptable reviewers in [0, n2), best first, -1 ends the list;
    ``val[i, p]`` is c(i, idx[i, p]).  Both sides prefer the larger value and, on equal values, the lower index; -1 = unmatched /
    free.  Deferred acceptance with one 64-bit word per reviewer, run to its fixpoint on the device."""
    idx, val = _candidate_lists(idx, val, n2, "stable_matching")
    st = _StableState(idx, val, n2)
    st.step()
    return st.match1.to(torch.int64), st.match2.to(torch.int64)


def alignment_topk_viable(emb1: torch.Tensor, emb2: torch.Tensor, k: int, best: torch.Tensor, row_id=None, csls_k: int = 10,
                          metric: str = "cosine", normalize: bool = False, terms=None,
                          screen: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``alignment_topk`` over the reviewers a suitor can still win: column j counts for row m only if the word of
    (c(m, j), row_id[m]) -- larger c first, equal c -> lower id -- is above ``best[j]`` (int64 [n2], the reviewers' 64-bit words of
    a deferred-acceptance run, 0 = free).  ``row_id`` (default 0 .. n1-1) names the suitor each row stands for.  A row with fewer
    than k such columns ends in (idx -1, val -inf).  With ``best`` all zero this is ``alignment_topk`` bit for bit.
    ``screen="bf16"``: the same bits from jmac_sim_csls_topk_viable_screened_f32 (as in ``alignment_topk``)."""
    _check_screen("alignment_topk_viable", screen, metric)
    a, b, r1, r2 = _csls_operands(emb1, emb2, csls_k, metric, normalize, terms, screen)
    n1, n2 = a.shape[0], b.shape[0]
    k = _check_k("alignment_topk_viable", k, n2)
    require_device(best)
    if best.dtype != torch.int64 or best.shape != (n2,):
        raise ValueError("best must be an int64 vector of n2 words")
    rid = torch.arange(n1, dtype=torch.int32, device=a.device) if row_id is None else \
        torch.as_tensor(row_id, device=a.device).to(torch.int32).contiguous()
    if rid.shape != (n1,):
        raise ValueError("row_id must have one entry per row of emb1")
    idx, val = _csls_topk(a, b, k, r1, r2, metric, rid, best.contiguous(), screen=screen)
    return idx.to(torch.int64), val


# A refill gathers a handful of rows, and a screened call of any size pays the bf16 copy of the whole table: below this many rows the
# fp32 entry is faster (measured).  The viable entry applies the same count itself (SC_VIABLE_MIN_ROWS, screen.hip);
# the auction's refill runs through the plain entry, which screens whatever it is given, so that one is routed here.
SCREEN_REFILL_MIN_ROWS = 256


class _ScreenedCalls:
    """Counts, on the device, the refill calls of a matching run that took the screen: a call's ``n_rescored`` is -2 throughout when
    its shape ran the fp32 code (a narrow table; a viable refill of fewer rows than the library screens).  No host read per call."""

    def __init__(self, device):
        self.calls = torch.zeros(1, dtype=torch.int64, device=device)

    def buffer(self, rows: int) -> torch.Tensor:
        self.n = torch.empty(rows, dtype=torch.int32, device=self.calls.device)
        return self.n

    def count(self):
        self.calls += (self.n[:1] > -2)


def _run_screen_stats(n_rescored: torch.Tensor, refills: _ScreenedCalls) -> dict:
    """``stats["screen"]`` of a matching run: the initial call's list statistics and the refill calls that took the screen"""
    s = _screen_stats(n_rescored)
    return dict(rows=s["rows"], overflow_rows=s["overflow_rows"], rescored_mean=s["rescored_mean"],
                refill_calls_screened=int(refills.calls.item()))


def _refill_chunk_rows(metric: str, n1: int, n2: int, d: int, k: int, ws_bytes: int, screen: Optional[str] = None) -> int:
    """Most rows L whose top-k workspace AND gathered operand rows fit ``ws_bytes`` together (both grow linearly with L)."""
    need = lambda rows: _topk_bytes(metric, rows, n2, d, k, screen) + rows * d * 4 + 256      # noqa: E731
    rows = n1
    while rows > 1 and need(rows) > ws_bytes:
        rows = max(1, min(rows - 1, rows * ws_bytes // need(rows)))
    return rows


def stable_alignment(emb1: torch.Tensor, emb2: torch.Tensor, k: int = 16, csls_k: int = 10, metric: str = "cosine",
                     normalize: bool = False, terms=None, max_refills: Optional[int] = None, screen: Optional[str] = None):
    """A one-to-one alignment: ``(match1 int64 [n1], val1 fp32 [n1], stats)``, the suitor-optimal stable matching of the full
    n1 x n2 instance under c = ``alignment_sim(emb1, emb2, metric, normalize, csls_k)`` (suitors: rows of emb1; both sides prefer the
    larger c, ties -> lower index), without the matrix.  ``match1[i]`` is suitor i's reviewer or -1 (exactly max(0, n1 - n2)
    suitors when the run is complete), ``val1[i] = c(i, match1[i])`` or -inf.

    Every suitor starts on ``alignment_topk``'s k candidates; deferred acceptance runs on the lists; a suitor all of whose
    candidates have rejected it gets the k best of the reviewers it could still win (the viable top-k), and so on until nobody is
    left without candidates.  A reviewer only trades up, so a reviewer left out of a refill would have rejected the suitor anyway:
    the result is that of the full lists.  One host read per round.  ``stats``: refills (rounds of refill), proposals, unmatched,
    complete (False only when ``max_refills`` stopped the loop; suitors still open are -1 then).
    ``screen="bf16"``: the initial lists and every refill come from the screened top-k entries -- the same lists bit for bit, hence
    the same run; ``stats["screen"]`` then holds rows, overflow_rows and rescored_mean of the initial call and the number of
    refill calls that took the screen (refill_calls_screened: the library runs a viable refill of fewer than 256 rows on the fp32
    code, where the bf16 copy of the whole table costs more than it saves)."""
    _check_screen("stable_alignment", screen, metric)
    a, b, r1, r2 = _csls_operands(emb1, emb2, csls_k, metric, normalize, terms, screen)
    n1, d = a.shape
    n2 = b.shape[0]
    k = _check_k("stable_alignment", k, n2)
    # one workspace for every top-k of the run; a refill's gathered rows of `a` live in its tail
    ws_bytes = max(_topk_bytes(metric, n1, n2, d, k, screen), _topk_bytes(metric, 1, n2, d, k, screen) + d * 4 + 256)
    ws = workspace(ws_bytes, a.device)
    nres = torch.empty(n1, dtype=torch.int32, device=a.device) if screen is not None else None
    idx, val = _csls_topk(a, b, k, r1, r2, metric, ws=ws, screen=screen, n_rescored=nres)
    st = _StableState(idx, val, n2)
    refills = proposals = 0
    refill_calls = _ScreenedCalls(a.device) if screen is not None else None
    complete = True
    chunk = 0
    while n1 > 0:
        exhausted, made = st.step()
        proposals += made
        if exhausted == 0:
            break
        if max_refills is not None and refills >= int(max_refills):
            complete = False
            break
        ids = st.exhausted_ids(exhausted)
        chunk = chunk or _refill_chunk_rows(metric, n1, n2, d, k, ws_bytes, screen)
        for lo in range(0, exhausted, chunk):
            rid = ids[lo:lo + chunk].contiguous()
            rows = rid.numel()
            sel = rid.to(torch.int64)
            sub = ws[ws_bytes - rows * d * 4:].view(torch.float32).view(rows, d)       # (ws_bytes and the offset: multiples of 16)
            torch.index_select(a, 0, sel, out=sub)
            r1s = r1.index_select(0, sel) if r1 is not None else None
            nres_r = refill_calls.buffer(rows) if screen is not None else None
            idx[sel], val[sel] = _csls_topk(sub, b, k, r1s, r2, metric, rid, st.best, ws, screen=screen, n_rescored=nres_r)   # the workspace's head
            st.ptr[sel] = 0
            if screen is not None:
                refill_calls.count()
        refills += 1
    m1 = st.match1.to(torch.int64)
    held = (st.ptr & 0x7fffffff).to(torch.int64).clamp_(max=k - 1).unsqueeze(1)
    val1 = torch.where(m1 >= 0, val.gather(1, held).squeeze(1), torch.full_like(val[:, 0], float("-inf")))
    stats = {"refills": refills, "proposals": proposals, "unmatched": int((m1 < 0).sum().item()), "complete": complete}
    if screen is not None:
        stats["screen"] = _run_screen_stats(nres, refill_calls)
    return m1, val1, stats


# ---- optimal one-to-one alignment: the auction algorithm on candidate lists ("Hungarian" in the literature) -----------------------------
AUCTION_QUEUE_ROWS = 256                     # JMAC_AUCTION_QUEUE_ROWS: the open rows the one-workgroup form of the rounds kernel holds
AUCTION_BATCH = 64                           # rounds per call, whatever its form: a waiting row comes back when its batch ends


class _AuctionState:
    """The device state of one auction run (jmac_auction_rounds_f32): candidate lists (idx, val = c - price as of the refill, pref =
    the price then), prices, owners and the rows' states.  ``step(rounds, n_open)`` runs up to that many rounds and returns the
    counters (open, waiting, rounds, bids) -- its one host read."""

    def __init__(self, idx: torch.Tensor, val: torch.Tensor, n2: int, eps: float):
        dev = idx.device
        self.idx, self.val, self.n2, self.eps = idx, val, int(n2), float(eps)
        self.n1, self.k = idx.shape
        self.pref = torch.zeros_like(val)
        self.price = torch.zeros(self.n2, dtype=torch.float32, device=dev)
        self.owner = torch.full((self.n2,), -1, dtype=torch.int32, device=dev)
        self.match1 = torch.full((self.n1,), -1, dtype=torch.int32, device=dev)
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ws_bytes = int(lib().jmac_auction_rounds_workspace_bytes(self.n1, self.n2))
        self.ws = workspace(self.ws_bytes, dev)

    def step(self, rounds: int, n_open: int, form: int = 0) -> Tuple[int, int, int, int]:
        check(lib().jmac_auction_rounds_f32(ptr(self.idx), ptr(self.val), ptr(self.pref), self.k, self.n1, self.n2, self.k, ptr(self.price),
                                            ptr(self.owner), ptr(self.match1), self.eps, int(rounds), int(form), int(n_open),
                                            ptr(self.counters), ptr(self.ws), self.ws_bytes, stream()), "jmac_auction_rounds_f32")
        n_open, waiting, done, bids = self.counters.tolist()
        return int(n_open), int(waiting), int(done), int(bids)


def auction_alignment(emb1: torch.Tensor, emb2: torch.Tensor, k: int = 16, csls_k: int = 10, metric: str = "cosine",
                      normalize: bool = False, terms=None, eps: float = 1e-3, max_rounds: Optional[int] = None, form: int = 0,
                      screen: Optional[str] = None):
    """The OPTIMAL one-to-one alignment: ``(match1 int64 [n1], val1 fp32 [n1], price fp32, stats)``, the assignment that maximises
    the total of c = ``alignment_sim(emb1, emb2, metric, normalize, csls_k)`` over all one-to-one matchings of the smaller side (what
    the entity-alignment literature reports as "Hungarian"), to within min(n1, n2) * eps, without the n1 x n2 matrix.  ``match1[i]`` is
    row i's column or -1, ``val1[i]`` = c(i, match1[i]) to rounding or -inf, ``price`` the dual prices of the columns.

    Bertsekas' auction: an open row bids its best column up by (best - second best) + eps of c - price; the highest bidder takes the
    column and opens its previous owner.  A row only needs its two best values, so it runs on ``alignment_topk``'s k candidates
    (2 <= k <= min(64, n2)); prices only rise, so as long as its second best is no worse than the last listed value as of the refill
    no unlisted column can matter, and a row for which that fails gets its top-k under the current prices -- the rescoring term r2
    carries the prices through the same fused top-k (``csls_k = 0``: terms (0, 2 price), values halved: exact).  Rounds run in
    batches on the device (jmac_auction_rounds_f32; one host read per batch); columns never bid on keep price 0, so the final
    matching and prices satisfy eps-complementary slackness of the rectangular problem.  n1 > n2 runs the transposed instance:
    n1 - n2 rows are -1, ``price`` has n1 entries, ``stats["transposed"]`` is set.

    ``stats``: rounds, bids, batches (host reads), refills, refill_rows, unmatched, complete (False only when ``max_rounds`` stopped
    the run; rows still open are -1 then), eps, transposed.  ``form``: 0 lets the library pick the launch form of every batch from
    the open count, 1 holds it to the grid form (the same bits).  ``screen="bf16"``: the initial lists and every price-carrying
    refill of at least ``SCREEN_REFILL_MIN_ROWS`` rows (r2 + price is one more finite r2) come from the screened top-k entry, bit
    for bit the same; smaller refills stay on the fp32 entry, which is faster there.  ``stats["screen"]`` as in ``stable_alignment``."""
    _check_screen("auction_alignment", screen, metric)
    eps = float(eps)
    if not (eps > 0.0 and np.isfinite(eps)):
        raise ValueError("auction_alignment: eps must be finite and positive (got %r)" % eps)
    if emb1.dim() != 2 or emb2.dim() != 2 or emb1.shape[0] == 0 or emb2.shape[0] == 0:
        raise ValueError("auction_alignment: empty operand")
    a, b, r1, r2 = _csls_operands(emb1, emb2, csls_k, metric, normalize, terms, screen)
    transposed = a.shape[0] > b.shape[0]
    if transposed:                                                  # columns bid for rows: c^T, the terms change sides
        a, b, r1, r2 = b, a, r2, r1
    n1, d = a.shape
    n2 = b.shape[0]
    k = int(k)
    if not 2 <= k <= min(CSLS_KMAX, n2):
        raise ValueError("auction_alignment: k must lie in [2, min(64, n2)] (got %d, n2 = %d)" % (k, n2))
    dev = a.device
    ws_bytes = max(_topk_bytes(metric, n1, n2, d, k, screen), _topk_bytes(metric, 1, n2, d, k, screen) + d * 4 + 256)
    ws = workspace(ws_bytes, dev)
    nres = torch.empty(n1, dtype=torch.int32, device=dev) if screen is not None else None
    idx, val = _csls_topk(a, b, k, r1, r2, metric, ws=ws, screen=screen, n_rescored=nres)
    refill_calls = _ScreenedCalls(dev) if screen is not None else None
    st = _AuctionState(idx, val, n2, eps)
    stats = {"rounds": 0, "bids": 0, "batches": 0, "refills": 0, "refill_rows": 0}
    complete = True
    n_open, chunk = n1, 0
    while True:
        rounds = AUCTION_BATCH if max_rounds is None else min(AUCTION_BATCH, int(max_rounds) - stats["rounds"])
        n_open, waiting, done, bids = st.step(max(rounds, 0), n_open, form)
        stats["rounds"] += done
        stats["bids"] += bids
        stats["batches"] += 1
        if n_open == 0:
            break
        if max_rounds is not None and stats["rounds"] >= int(max_rounds):
            complete = False
            break
        if waiting == 0:
            continue
        # the rows at -2, ascending (a stable sort of "is not waiting" lists them first: no second host read)
        ids = torch.sort((st.match1 != -2).to(torch.uint8), stable=True).indices[:waiting]
        chunk = chunk or _refill_chunk_rows(metric, n1, n2, d, k, ws_bytes, screen)
        if r2 is not None:
            r2p = r2 + st.price
        else:
            r2p = 2.0 * st.price
        for lo in range(0, waiting, chunk):
            sel = ids[lo:lo + chunk]
            rows = sel.numel()
            sub = ws[ws_bytes - rows * d * 4:].view(torch.float32).view(rows, d)
            torch.index_select(a, 0, sel, out=sub)
            r1s = r1.index_select(0, sel) if r1 is not None else torch.zeros(rows, dtype=torch.float32, device=dev)
            if screen is not None and rows >= SCREEN_REFILL_MIN_ROWS:
                nidx, nval = _csls_topk(sub, b, k, r1s, r2p, metric, ws=ws, screen=screen, n_rescored=refill_calls.buffer(rows))
                refill_calls.count()
            else:
                nidx, nval = _csls_topk(sub, b, k, r1s, r2p, metric, ws=ws)
            if r2 is None:
                nval = nval * 0.5                                    # (2 S - 2 price) / 2: exact
            idx[sel], val[sel] = nidx, nval
            st.pref[sel] = st.price[nidx.to(torch.int64)]
            st.match1[sel] = -1
        stats["refills"] += 1
        stats["refill_rows"] += waiting
    m1 = st.match1.to(torch.int64).clamp_(min=-1)
    held = idx.to(torch.int64) == m1.unsqueeze(1)
    neg = torch.full_like(val[:, 0], float("-inf"))
    val1 = torch.where(m1 >= 0, torch.where(held, val + st.pref, torch.zeros_like(val)).sum(1), neg)
    price = st.price
    if transposed:                                                  # back to the caller's sides: its rows are the columns here
        rows_of = torch.full((n2,), -1, dtype=torch.int64, device=dev)
        vals_of = torch.full((n2,), float("-inf"), dtype=torch.float32, device=dev)
        got = m1 >= 0
        rows_of[m1[got]] = torch.nonzero(got).squeeze(1)
        vals_of[m1[got]] = val1[got]
        m1, val1 = rows_of, vals_of
    stats.update(unmatched=int((m1 < 0).sum().item()), complete=complete, eps=eps, transposed=transposed)
    if screen is not None:
        stats["screen"] = _run_screen_stats(nres, refill_calls)
    return m1, val1, price, stats


def _rank_summary(rank: torch.Tensor, top_k):
    rank = rank.to(torch.float64)
    hits = [float((rank <= k).double().mean().item() * 100.0) for k in top_k]
    return list(top_k), [round(h, 3) for h in hits], float(rank.mean().item()), float((1.0 / rank).mean().item())


def alignment_test(embeds1: torch.Tensor, embeds2: torch.Tensor, top_k=(1, 5, 10), metric: str = "cosine",
                   normalize: bool = False, csls_k: int = 10, matrix_free: bool = False, screen: Optional[str] = None):
    """test() / greedy_alignment() / calculate_rank(accurate=True), evaluation.py:20-28, alignment.py:10-112:
    row i of embeds1 is aligned with row i of embeds2.  Returns (top_k, hits [%], mr, mrr).  ``matrix_free``: the same ranks,
    hence the same tuple, from ``csls_terms`` + ``alignment_ranks`` -- three products, no n x n matrix.  ``screen``:
    ``alignment_ranks``'s, with ``matrix_free`` only (the stored matrix has no screened form)."""
    _check_screen("alignment_test", screen, metric)
    if screen is not None and not matrix_free:
        raise ValueError("alignment_test: screen needs matrix_free=True")
    if matrix_free:
        gold = torch.arange(embeds1.shape[0], device=embeds1.device, dtype=torch.int32)
        return _rank_summary(alignment_ranks(embeds1, embeds2, gold, csls_k, metric, normalize, screen=screen), top_k)
    s = alignment_sim(embeds1, embeds2, metric, normalize, 0)
    n = s.shape[0]
    gold = torch.arange(n, device=s.device, dtype=torch.int32)
    if csls_k > 0:                                                     # CSLS rescoring fused into the rank count
        rank = csls_rank(s, csls_k, gold)
    else:
        rank = filtered_rank(s, gold, descending=True)                 # 1-based position in the descending order
    return _rank_summary(rank, top_k)
