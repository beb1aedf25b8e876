"""Minimal training / evaluation harness that drives the hot path the way the reference's train.py does.

Not a re-implementation of train.py (argparse, Logger, DataLoader worker processes and the fastText name
embeddings are out of scope): just enough host code to run, on the HIP device,

    train_completion_component   train.py:328-364    batches sub.repeat(K+1) / rel.repeat(K+1) / cat(obj, neg)
    train_alignment_component    train.py:367-378    one full-batch alignment step
    CompletionEvaluator.test     src/validate.py:22-80   filtered ranking, Hits@1 / Hits@10 / MRR
    one epoch over the KG pairs  train.py:423-512    get_emb -> EnTr -> completion -> alignment

end to end, so the integration of data.py / graph.py / model.py / losses.py / scoring.py / entr.py is tested as a
whole (tests/test_gpu_harness.py).

Where the completion batches come from is ``args.neg_sampler``:

    "uniform" (default)   ``completion_batches``: a few torch calls per batch -- negatives drawn uniformly WITH replacement, a clash
                          with the gold tail redrawn once (it can clash again; the other true tails of (h, r) are not looked at).
                          An approximation of the reference's sampler, kept as it was.
    "filtered"            ``sampling.CompletionSampler``: the reference's sampler (modules/load/data_loader.py:36-47: distinct
                          negatives, uniform over the entities that are not a true tail of (h, r)) as one launch per batch into
                          persistent buffers, one sampler per KG of the pair, rebuilt at every refresh.
    "truncated"           the same sampler with BootEA's hard negatives in front (``--neg_sampling truncated``, modules/train/batch.py:
                          88-165): at every refresh each KG of the pair gets the ``args.neg_neighbors`` (default 64) nearest entities
                          of every entity under ``args.neg_metric`` (default "inner": ``find_neighbours``' product; ``args.sim_screen``
                          is honoured) in a ``sampling.NeighborTable`` refreshed in place, and the first ``args.neg_hard`` (default:
                          all ``num_negative``) negatives of a row come from its gold tail's row of that table.
    ``args.capture_completion`` (with "filtered" / "truncated" only): after three eager steps the step zero_grad -> next_batch ->
                          completion_loss -> backward -> step is captured in a hipGraph once per (pair, side, refresh) and replayed
                          for the remaining batches of every epoch until the next refresh; the per-step losses land in a device
                          vector that is read once per epoch.  Needs an optimizer whose step captures (``jmac_amd.optim.Adam``,
                          or ``torch.optim.Adam(capturable=True)``).
"""
from __future__ import annotations

import types
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import entr, scoring
from .sampling import CompletionSampler, NeighborTable, TrueTailIndex
from .data import KnowledgeGraph
from .model import JMAC


def make_args(dim=300, batch_size=1000, num_negative=25, device="cuda", entr_matrix_free=False, **kw):
    a = dict(dim=dim, dropout=0.4, leaky_relu_w=0.05, comp_op="sub", num_gcn_layer=2, num_negative=num_negative,
             margin_align=1.0, margin_completion=5.0, batch_size=batch_size, no_name_info=False, device=device,
             pair_sample_weight=0.2, lr=1e-3,                     # train.py:57-102 defaults for the fields used here
             eval_metric="cosine", eval_norm=False,              # the alignment evaluator's sim() (train.py:95-96, :112)
             neg_sampler="uniform", capture_completion=False,    # this harness' own: where the completion batches come from
             neg_neighbors=64, neg_hard=None, neg_metric="inner",  # "truncated": table width, hard negatives per row, metric
             entr_matrix_free=entr_matrix_free)                   # EnTr refresh from scoring.alignment_stats (no N1 x N2 matrix)
    a.update(kw)
    return types.SimpleNamespace(**a)


def process_input_data(kg: KnowledgeGraph, device):
    """train.py:214-228: first visit uses the loader's bidirectional graph, later visits the transferred triples."""
    if not len(kg.transferred_triples):
        triples = kg.train_data
        kg.triple_keys = entr.encode_triples(triples)
        ei, et = torch.from_numpy(kg.edge_index).to(device), torch.from_numpy(kg.edge_type).to(device)
    else:
        triples = kg.transferred_triples
        ei, et = entr.align_data_processing(triples, device)
    return ei, et, [kg.entity_id_base, kg.upper_entity_base], [kg.relation_id_base, kg.upper_relation_base], triples


def completion_batches(triples: np.ndarray, num_ent: int, batch_size: int, k: int, device, generator=None):
    """(triple [B,3], neg [B,k]) batches of full size only (train.py:343-346 skips ragged last batches)."""
    t = torch.from_numpy(np.asarray(triples, dtype=np.int64)).to(device)
    perm = torch.randperm(len(t), device=device, generator=generator)
    for s in range(0, len(t) - batch_size + 1, batch_size):
        tr = t[perm[s:s + batch_size]]
        neg = torch.randint(0, num_ent, (batch_size, k), device=device, generator=generator)
        clash = neg == tr[:, 2:3]
        neg = torch.where(clash, torch.randint(0, num_ent, neg.shape, device=device, generator=generator), neg)
        yield tr, neg


def train_completion_component(model: JMAC, opt, ei1, et1, ei2, et2, feeddict, triples1, triples2, n1, n2, args, generator=None,
                               state: dict = None):
    """One completion epoch on a KG pair (train.py:328-364): every full batch of KG 1, then of KG 2.  ``state`` (optional): a
    dict that lives as long as the triple lists and graphs do (train_epoch: until the next refresh); the "filtered" mode keeps
    its samplers and captured steps there and leaves the epoch's per-step losses (device, [steps]) under "step_losses".  The
    "truncated" mode reads ``state["neighbors"]``, one ``NeighborTable`` per KG, or builds them from ``state["embeddings"]``, the
    two KGs' entity embeddings ``[n1, d]`` / ``[n2, d]`` on the device (``neighbor_tables``)."""
    mode = getattr(args, "neg_sampler", "uniform")
    if mode in ("filtered", "truncated"):
        state = {} if state is None else state
        if mode == "truncated" and "neighbors" not in state:
            if state.get("embeddings") is None:
                raise ValueError("args.neg_sampler == 'truncated' needs the neighbour tables: pass state={'neighbors': (NeighborTable of "
                                 "KG 1, NeighborTable of KG 2)} or state={'embeddings': (emb1 [n1, d], emb2 [n2, d])} (device tensors)")
            state["neighbors"] = neighbor_tables(state["embeddings"], (n1, n2), args)
        return _train_completion_filtered(model, opt, ei1, et1, ei2, et2, feeddict, triples1, triples2, n1, n2, args, generator, state)
    if mode != "uniform":
        raise ValueError("args.neg_sampler must be 'uniform', 'filtered' or 'truncated' (got %r)" % (mode,))
    if getattr(args, "capture_completion", False):
        raise ValueError("args.capture_completion needs args.neg_sampler == 'filtered' or 'truncated' (the uniform batches are new "
                         "tensors every step)")
    losses = []
    for triples, n_ent, source in ((triples1, n1, True), (triples2, n2, False)):
        for tr, neg in completion_batches(triples, n_ent, args.batch_size, args.num_negative, ei1.device, generator):
            opt.zero_grad(set_to_none=True)
            sub, rel, obj = tr[:, 0], tr[:, 1], tr[:, 2]
            k = args.num_negative
            data = {"batch_h": sub.repeat(k + 1), "batch_r": rel.repeat(k + 1), "batch_t": torch.cat((obj, neg.view(-1)))}
            loss = model.completion_loss(data, ei1, et1, ei2, et2, feeddict, source)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
    return float(torch.stack(losses).mean()) if losses else float("nan")


def neighbor_tables(embeddings, num_ents, args, tables=None):
    """One ``NeighborTable`` per KG for the "truncated" sampler, filled from the KG's entity embeddings (``generate_neighbours``);
    ``tables``: an earlier call's result, refreshed in place (their buffers keep their addresses)."""
    if tables is None:
        tables = tuple(NeighborTable(n, getattr(args, "neg_neighbors", 64), e.device) for e, n in zip(embeddings, num_ents))
    for t, e in zip(tables, embeddings):
        t.refresh(e, getattr(args, "neg_metric", "inner"), getattr(args, "sim_screen", None))
    return tables


_CAPTURE_WARMUP = 3      # eager steps in front of a capture (bench.py:try_capture): real training steps of the epoch


def _train_completion_filtered(model, opt, ei1, et1, ei2, et2, feeddict, triples1, triples2, n1, n2, args, generator, state):
    dev = ei1.device
    capture = bool(getattr(args, "capture_completion", False))
    sides = state.get("completion_sides")
    if sides is None:                                      # once per (pair, refresh): the CSR of the true tails, the batch buffers
        hard = [{}, {}]
        if getattr(args, "neg_sampler", "uniform") == "truncated":
            hard = [{"neighbors": t, "n_hard": getattr(args, "neg_hard", None)} for t in state["neighbors"]]
        sides = state["completion_sides"] = [
            {"sampler": CompletionSampler(tr, n, args.batch_size, args.num_negative, dev, **kw), "source": src, "graph": None}
            for tr, n, src, kw in ((triples1, n1, True, hard[0]), (triples2, n2, False, hard[1])) if len(tr) >= args.batch_size]
    links = feeddict["links"]
    if len(links) and not (isinstance(links, torch.Tensor) and links.device == dev):
        # host seed links (train.py:190-193 hands out numpy arrays) would be uploaded by every step, which a stream capture
        # refuses: upload them once per refresh -- completion_loss cuts and checks the columns of a device tensor once
        if "links" not in state:
            state["links"] = torch.as_tensor(np.asarray(links.cpu() if isinstance(links, torch.Tensor) else links).astype(np.int64)).to(dev)
        feeddict = dict(feeddict, links=state["links"])
    per_side = []
    for side in sides:
        sampler, source = side["sampler"], side["source"]
        steps = len(sampler)
        out = side.setdefault("losses", torch.zeros(steps, dtype=torch.float32, device=dev))
        slot = side.setdefault("slot", torch.zeros(1, dtype=torch.int64, device=dev))
        sampler.new_epoch(generator)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = model.completion_loss(sampler.next_batch(), ei1, et1, ei2, et2, feeddict, source)
            loss.backward()
            opt.step()
            out.index_copy_(0, slot, loss.detach().reshape(1))          # device-side slot: a replay writes the next one
            slot.add_(1)

        slot.zero_()
        done = 0
        if not capture:
            for _ in range(steps):
                step()
        else:
            if side["graph"] is None and steps > _CAPTURE_WARMUP:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(_CAPTURE_WARMUP):
                        step()
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                done = _CAPTURE_WARMUP
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    step()
                side["graph"] = g
            if side["graph"] is None:                      # an epoch no longer than the warm-up: nothing left to replay
                for _ in range(steps):
                    step()
            else:
                for _ in range(steps - done):
                    side["graph"].replay()
                sampler.skip(steps - done)
        per_side.append(out.clone())
    if not per_side:
        state["step_losses"] = torch.zeros(0, dtype=torch.float32, device=dev)
        return float("nan")
    state["step_losses"] = torch.cat(per_side)
    return float(state["step_losses"].mean())


def train_alignment_component(model: JMAC, opt, ei1, et1, ei2, et2, feeddict):
    if not len(feeddict["links"]):
        return 0.0
    opt.zero_grad(set_to_none=True)
    loss = model.alignment_loss(feeddict, ei1, et1, ei2, et2)
    loss.backward()
    opt.step()
    return float(loss.detach())


def _true_tail_index(kg: KnowledgeGraph, device):
    """``kg.true_tail`` as a device index, built once and kept on the KG object; rebuilt when the dictionary object or the
    device changes."""
    if not kg.true_tail:                                   # nothing known: every query ranks raw
        return None
    device = torch.device(device)
    hit = getattr(kg, "_true_tail_index", None)
    if hit is None or hit[0] is not kg.true_tail or hit[1] != device:
        hit = (kg.true_tail, device, TrueTailIndex.from_dict(kg.true_tail, device))
        kg._true_tail_index = hit
    return hit[2]


@torch.no_grad()
def evaluate_completion(model: JMAC, kg: KnowledgeGraph, ei, et, args, split="val", filtered=True, fused=True, eval_batch=None):
    """CompletionEvaluator.test (src/validate.py:22-80) with the encoder run once instead of once per batch.
    The reference scores 1 000 queries at a time (``args.batch_size``) because it materialises their [B, N] distance matrix.  The
    fused path has no matrix and a query's rank does not depend on what else is in its call, so it takes ``eval_batch`` queries
    per call -- default: up to 16 384, i.e. a whole DBP-5L split at once (the per-call query preparation and the last partial
    round of tiles are paid once); the materialised path keeps the reference's batches.  The fused path's filter is the KG's
    ``TrueTailIndex`` on the device (no per-query host work); the materialised path packs the reference's per-batch lists."""
    model.eval()
    data = {"val": kg.val_data, "test": kg.test_data, "train": kg.train_data}[split]
    eb, rb = [kg.entity_id_base, kg.upper_entity_base], [kg.relation_id_base, kg.upper_relation_base]
    cached = model.forward_base(ei, et, eb, rb)
    ranks = []
    step = int(eval_batch or (16384 if fused else args.batch_size))
    for s in range(0, len(data), step):
        b = data[s:s + step]
        if fused:       # ranks without the [B, N] matrix; the filter is looked up in the KG's known-tail index on the device
            index = _true_tail_index(kg, ei.device) if filtered else None
            ranks.append(model.linkpred_ranks(b[:, 0], b[:, 1], b[:, 2], ei, et, eb, rb, cached=cached, index=index))
        else:           # the reference's two steps: forward_linkpred, then the ranking loop
            h, r, t = b[:, 0].tolist(), b[:, 1].tolist(), b[:, 2].tolist()
            fp = fi = None
            if filtered:
                fp, fi = scoring.build_filter_csr(h, r, kg.true_tail, ei.device)
            dist = model.forward_linkpred(h, r, ei, et, range(kg.num_entity), eb, rb, cached=cached)
            ranks.append(scoring.filtered_rank(dist, torch.as_tensor(t, dtype=torch.int32, device=dist.device), fp, fi))
    rk = torch.cat(ranks).double()
    model.train()
    return float((rk <= 1).double().mean()), float((rk <= 10).double().mean()), float((1.0 / rk).mean())


def calibration_error(confidence: torch.Tensor, correct: torch.Tensor, bins: int = 10) -> torch.Tensor:
    """Expected calibration error of top-1 predictions: over ``bins`` equal-width confidence bins [j / bins, (j + 1) / bins)
    (the last one closed), sum of (share of the queries in the bin) * |accuracy in the bin - mean confidence in the bin|.
    A 0-d float64 tensor on the inputs' device (no host read)."""
    conf = confidence.double().reshape(-1)
    hit = correct.double().reshape(-1)
    which = (conf * bins).long().clamp_(0, bins - 1)
    zero = torch.zeros(bins, dtype=torch.float64, device=conf.device)
    n = zero.index_add(0, which, torch.ones_like(conf))
    gap = (zero.index_add(0, which, hit) - zero.index_add(0, which, conf)).abs()      # n_j |acc_j - conf_j|
    return gap.sum() / n.sum().clamp_min(1.0)


def _completion_stats(model: JMAC, kg: KnowledgeGraph, ei, et, split, eval_batch):
    """(triples of the split, call(scale) -> scoring.LinkStats of the whole split in evaluation mode, filtered): the encoder runs
    once, every call scores on its cached tables."""
    data = {"val": kg.val_data, "test": kg.test_data, "train": kg.train_data}[split]
    eb, rb = [kg.entity_id_base, kg.upper_entity_base], [kg.relation_id_base, kg.upper_relation_base]
    cached = model.forward_base(ei, et, eb, rb)
    index = _true_tail_index(kg, ei.device)
    step = int(eval_batch or 16384)

    def call(scale):
        parts = [model.linkpred_stats(data[s:s + step, 0], data[s:s + step, 1], scale, ei, et, eb, rb, gold=data[s:s + step, 2],
                                      index=index, cached=cached) for s in range(0, len(data), step)]
        if len(parts) == 1:
            return parts[0]
        return scoring.LinkStats(*[torch.cat([getattr(p, f) for p in parts]) for f in scoring.LinkStats._fields[:-1]], parts[0].scale)

    return data, call


@torch.no_grad()
def evaluate_completion_confidence(model: JMAC, kg: KnowledgeGraph, ei, et, args, scale, split="val", eval_batch=None):
    """How well calibrated the completion model is on a split, under ``softmax(-scale * dist)`` over the filtered candidates
    (scoring.linkpred_stats in evaluation mode): ``{"nll": mean -log p(gold), "entropy": mean entropy in nats, "confidence": mean
    top-1 probability, "hits1": share of queries whose nearest candidate is the gold, "ece": calibration_error of the top-1
    prediction over ten bins}``.  The encoder runs once, the whole split goes through one call (``eval_batch`` as in
    evaluate_completion's fused path), the reductions run on the device and ONE host read ends it."""
    model.eval()
    data, call = _completion_stats(model, kg, ei, et, split, eval_batch)
    st = call(scale)
    gold = torch.as_tensor(np.ascontiguousarray(data[:, 2]), dtype=torch.int64, device=st.nearest.device)
    hit = st.nearest == gold
    conf = st.confidence
    out = torch.stack([-st.logp_gold.double().mean(), st.entropy.double().mean(), conf.double().mean(), hit.double().mean(),
                       calibration_error(conf, hit)]).tolist()
    model.train()
    return dict(zip(("nll", "entropy", "confidence", "hits1", "ece"), out))


@torch.no_grad()
def calibrate_link_scale(model: JMAC, kg: KnowledgeGraph, ei, et, args, scales, split="val"):
    """Temperature scaling by grid: ``(best_scale, {scale: nll})``, the ``scale`` of ``scales`` with the smallest mean negative
    log-likelihood of the split's gold tails (the first on ties).  One encoder pass, one statistics call per scale, one host read."""
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError("calibrate_link_scale: no scales given")
    model.eval()
    _, call = _completion_stats(model, kg, ei, et, split, None)
    nll = torch.stack([-call(s).logp_gold.double().mean() for s in scales]).tolist()
    model.train()
    table = dict(zip(scales, nll))
    return min(scales, key=lambda s: table[s]), table


def alignment_links(kg_t: KnowledgeGraph, kg_s: KnowledgeGraph, seed_pairs, predicted=None, device=None):
    """The link map of supporting KG ``kg_s`` for target ``kg_t`` (scoring.link_map: int32 [kg_t.num_entity], -1 = unaligned)
    from ``seed_pairs`` [L, 2] of (target row, support row), ids local to their KG.  ``predicted``: a ``match`` vector indexed by
    target row (scoring.stable_alignment / auction_alignment: the matched support row or -1) that fills the rows no seed
    names -- seeds win."""
    link = scoring.link_map(seed_pairs, kg_t.num_entity, kg_s.num_entity)
    if predicted is not None:
        p = torch.as_tensor(predicted).detach().cpu().to(torch.int64).reshape(-1)
        if p.numel() != kg_t.num_entity:
            raise ValueError("predicted must hold one entry per target entity (%d)" % kg_t.num_entity)
        if p.numel() and (int(p.min()) < -1 or int(p.max()) >= kg_s.num_entity):
            raise ValueError("predicted holds ids outside [-1, %d)" % kg_s.num_entity)
        link = torch.where(link >= 0, link, p.to(torch.int32))
    return link.to(device) if device is not None else link


@torch.no_grad()
def evaluate_completion_ensemble(model: JMAC, kgs: Dict[str, KnowledgeGraph], target: str, supports, graphs, links, weights, args,
                                 split="val", filtered=True, eval_batch=None):
    """evaluate_completion(fused=True) of KG ``target`` on the cross-KG ensemble distance (scoring.linkpred_ranks_ensemble):
    ``supports`` names the supporting KGs, ``graphs`` = [(ei, et) of the target, then of every support], ``links`` one link map
    per support (alignment_links), ``weights`` one per KG.  Every KG is encoded ONCE, a whole split goes through one call, the
    filter is the target's TrueTailIndex.  Returns (hits@1, hits@10, mrr).
    The KGs are encoded by forward_base, one call each, as evaluate_completion encodes its KG -- not as one stacked launch set
    (forward_blocks), whose rows agree with forward_base's to rounding only: with the target's tables bit for bit the same,
    weights (1, 0, ..) return evaluate_completion(fused=True)'s numbers exactly."""
    model.eval()
    kg = kgs[target]
    data = {"val": kg.val_data, "test": kg.test_data, "train": kg.train_data}[split]
    blocks = [(ei, et, [k.entity_id_base, k.upper_entity_base], [k.relation_id_base, k.upper_relation_base])
              for k, (ei, et) in zip([kg] + [kgs[s] for s in supports], graphs)]
    dev = graphs[0][0].device
    links = [l.to(dev) for l in links]
    cached = [model.forward_base(*b) for b in blocks]
    index = _true_tail_index(kg, dev) if filtered else None
    ranks = []
    step = int(eval_batch or 16384)
    for s in range(0, len(data), step):
        b = data[s:s + step]
        ranks.append(model.linkpred_ranks_ensemble(b[:, 0], b[:, 1], b[:, 2], blocks, links, weights, index=index, cached=cached))
    rk = torch.cat(ranks).double()
    model.train()
    return float((rk <= 1).double().mean()), float((rk <= 10).double().mean()), float((1.0 / rk).mean())


@torch.no_grad()
def evaluate_alignment(model: JMAC, kg1: KnowledgeGraph, kg2: KnowledgeGraph, pairs, graphs, args, csls_k=10, top_k=(1, 5, 10),
                       matrix_free=True, screen=None):
    """test_alignment_ (train.py:105-113) on the test pairs of a KG pair: row i of ``pairs`` aligns entity pairs[i, 0] of kg1
    with pairs[i, 1] of kg2 (ids local to their KG).  ``graphs``: ((ei1, et1), (ei2, et2)).  One encoder pass in eval mode, the
    alignment embeddings of the listed entities gathered on the device, then scoring.alignment_test -- by default its
    matrix-free form (no len(pairs)^2 matrix) -- under ``args.eval_metric`` ('cosine', 'inner', 'manhattan') and ``args.eval_norm``
    (train.py:95-96; absent: 'cosine', False).  Returns (top_k, hits [%], mr, mrr).  ``screen``: scoring.alignment_test's."""
    (ei1, et1), (ei2, et2) = graphs
    b1 = (ei1, et1, [kg1.entity_id_base, kg1.upper_entity_base], [kg1.relation_id_base, kg1.upper_relation_base])
    b2 = (ei2, et2, [kg2.entity_id_base, kg2.upper_entity_base], [kg2.relation_id_base, kg2.upper_relation_base])
    was_training = model.training
    model.eval()
    (a1, _), (a2, _) = model.get_emb_blocks([b1, b2], on_device=True)
    model.train(was_training)
    pairs = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64).reshape(-1, 2)
    scoring.check_index_range(pairs[:, 0], a1.shape[0], "pairs[:, 0]")
    scoring.check_index_range(pairs[:, 1], a2.shape[0], "pairs[:, 1]")
    p = torch.from_numpy(pairs).to(a1.device)
    return scoring.alignment_test(a1.index_select(0, p[:, 0]), a2.index_select(0, p[:, 1]), top_k, getattr(args, "eval_metric", "cosine"),
                                  bool(getattr(args, "eval_norm", False)), csls_k, matrix_free=matrix_free, screen=screen)


@torch.no_grad()
def evaluate_stable_alignment(model: JMAC, kg1: KnowledgeGraph, kg2: KnowledgeGraph, pairs, graphs, args, csls_k=10, k=16, screen=None):
    """stable_alignment (JMAC_DBPv1/modules/finding/alignment.py:90-134) on the test pairs of a KG pair, run to convergence: the
    pairs' embeddings are selected as in ``evaluate_alignment``, the one-to-one matching comes from scoring.stable_alignment (no
    len(pairs)^2 matrix).  Returns (precision [%], stats): "stable alignment precision" (:128-133), the share of matched suitors
    i with match1[i] == i, and the run's refills / proposals / unmatched / complete.  ``screen``: scoring.stable_alignment's."""
    (ei1, et1), (ei2, et2) = graphs
    b1 = (ei1, et1, [kg1.entity_id_base, kg1.upper_entity_base], [kg1.relation_id_base, kg1.upper_relation_base])
    b2 = (ei2, et2, [kg2.entity_id_base, kg2.upper_entity_base], [kg2.relation_id_base, kg2.upper_relation_base])
    was_training = model.training
    model.eval()
    (a1, _), (a2, _) = model.get_emb_blocks([b1, b2], on_device=True)
    model.train(was_training)
    pairs = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64).reshape(-1, 2)
    scoring.check_index_range(pairs[:, 0], a1.shape[0], "pairs[:, 0]")
    scoring.check_index_range(pairs[:, 1], a2.shape[0], "pairs[:, 1]")
    p = torch.from_numpy(pairs).to(a1.device)
    k = min(int(k), len(pairs))
    match1, _, stats = scoring.stable_alignment(a1.index_select(0, p[:, 0]), a2.index_select(0, p[:, 1]), k, csls_k,
                                                getattr(args, "eval_metric", "cosine"), bool(getattr(args, "eval_norm", False)),
                                                screen=screen)
    matched = match1 >= 0
    hits = (match1 == torch.arange(match1.numel(), device=match1.device)) & matched
    precision = 100.0 * float(hits.sum().item()) / max(1, int(matched.sum().item()))
    return precision, stats


@torch.no_grad()
def evaluate_auction_alignment(model: JMAC, kg1: KnowledgeGraph, kg2: KnowledgeGraph, pairs, graphs, args, csls_k=10, k=16, eps=1e-3,
                               screen=None):
    """The optimal one-to-one alignment of the test pairs of a KG pair (what the literature reports as "Hungarian"; no counterpart
    in the reference): the pairs' embeddings are selected as in ``evaluate_alignment``, the assignment comes from
    scoring.auction_alignment (no len(pairs)^2 matrix).  Returns (precision [%], stats), counted as ``evaluate_stable_alignment``
    counts it: the share of matched rows i with match1[i] == i.  ``screen``: scoring.auction_alignment's."""
    (ei1, et1), (ei2, et2) = graphs
    b1 = (ei1, et1, [kg1.entity_id_base, kg1.upper_entity_base], [kg1.relation_id_base, kg1.upper_relation_base])
    b2 = (ei2, et2, [kg2.entity_id_base, kg2.upper_entity_base], [kg2.relation_id_base, kg2.upper_relation_base])
    was_training = model.training
    model.eval()
    (a1, _), (a2, _) = model.get_emb_blocks([b1, b2], on_device=True)
    model.train(was_training)
    pairs = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64).reshape(-1, 2)
    scoring.check_index_range(pairs[:, 0], a1.shape[0], "pairs[:, 0]")
    scoring.check_index_range(pairs[:, 1], a2.shape[0], "pairs[:, 1]")
    p = torch.from_numpy(pairs).to(a1.device)
    k = min(int(k), len(pairs))
    match1, _, _, stats = scoring.auction_alignment(a1.index_select(0, p[:, 0]), a2.index_select(0, p[:, 1]), k, csls_k,
                                                    getattr(args, "eval_metric", "cosine"), bool(getattr(args, "eval_norm", False)),
                                                    eps=eps, screen=screen)
    matched = match1 >= 0
    hits = (match1 == torch.arange(match1.numel(), device=match1.device)) & matched
    precision = 100.0 * float(hits.sum().item()) / max(1, int(matched.sum().item()))
    return precision, stats


@torch.no_grad()
def evaluate_sinkhorn_alignment(model: JMAC, kg1: KnowledgeGraph, kg2: KnowledgeGraph, pairs, graphs, args, scale=50.0, iters=10,
                                top_k=(1, 5, 10), stable_k=None, screen=None):
    """``evaluate_alignment`` under the Sinkhorn plan of the test pairs instead of CSLS (no counterpart in the reference): the
    pairs' embeddings are selected as there, scoring.sinkhorn_terms gives the rescoring terms (2 ``iters`` products, no
    len(pairs)^2 matrix) and scoring.alignment_ranks the ranks.  ``args.eval_metric`` ('cosine', 'inner'; 'manhattan' is not
    built) and ``args.eval_norm`` as there.  Returns (top_k, hits [%], mr, mrr); with ``stable_k`` a fifth entry, the one-to-one
    precision [%] of scoring.stable_alignment (k = ``stable_k``) under the same terms, as ``evaluate_stable_alignment`` counts it.
    ``screen``: scoring.alignment_ranks's and scoring.stable_alignment's (the Sinkhorn iterations themselves are not screened)."""
    (ei1, et1), (ei2, et2) = graphs
    b1 = (ei1, et1, [kg1.entity_id_base, kg1.upper_entity_base], [kg1.relation_id_base, kg1.upper_relation_base])
    b2 = (ei2, et2, [kg2.entity_id_base, kg2.upper_entity_base], [kg2.relation_id_base, kg2.upper_relation_base])
    metric, norm = getattr(args, "eval_metric", "cosine"), bool(getattr(args, "eval_norm", False))
    if metric == "manhattan":
        raise NotImplementedError("evaluate_sinkhorn_alignment: metric 'manhattan' is not built ('cosine' and 'inner' are)")
    was_training = model.training
    model.eval()
    (a1, _), (a2, _) = model.get_emb_blocks([b1, b2], on_device=True)
    model.train(was_training)
    pairs = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64).reshape(-1, 2)
    scoring.check_index_range(pairs[:, 0], a1.shape[0], "pairs[:, 0]")
    scoring.check_index_range(pairs[:, 1], a2.shape[0], "pairs[:, 1]")
    p = torch.from_numpy(pairs).to(a1.device)
    e1, e2 = a1.index_select(0, p[:, 0]), a2.index_select(0, p[:, 1])
    terms = scoring.sinkhorn_terms(e1, e2, scale, iters, metric, norm)
    gold = torch.arange(e1.shape[0], device=e1.device, dtype=torch.int32)
    out = scoring._rank_summary(scoring.alignment_ranks(e1, e2, gold, 1, metric, norm, terms=terms, screen=screen), top_k)
    if stable_k is None:
        return out
    match1, _, _ = scoring.stable_alignment(e1, e2, min(int(stable_k), len(pairs)), 1, metric, norm, terms=terms, screen=screen)
    matched = match1 >= 0
    hits = (match1 == torch.arange(match1.numel(), device=match1.device)) & matched
    return (*out, 100.0 * float(hits.sum().item()) / max(1, int(matched.sum().item())))


def train_epoch(model: JMAC, kgs: Dict[str, KnowledgeGraph], seeds_train: Dict[Tuple[str, str], np.ndarray],
                seeds_test: Dict[Tuple[str, str], np.ndarray], opt_c, opt_a, args, state: dict, refresh: bool,
                generator=None) -> List[dict]:
    """One pass over the KG pairs (train.py:426-496).  ``state`` keeps the per-pair feeddicts / graphs / entropies."""
    dev = torch.device(args.device)
    log = []
    for idx, ((l1, l2), links) in enumerate(sorted(seeds_train.items())):
        kg1, kg2 = kgs[l1], kgs[l2]
        ei1, et1, eb1, rb1, tr1 = process_input_data(kg1, dev)
        ei2, et2, eb2, rb2, tr2 = process_input_data(kg2, dev)
        st = state.setdefault(idx, {"entropy": [-1], "seeds": [links]})
        if refresh or "feeddict" not in st:
            model.eval()
            with torch.no_grad():                      # train.py:450-451: get_emb once per KG of the pair -- one encoder pass here
                (a1, c1), (a2, c2) = model.get_emb_blocks([(ei1, et1, eb1, rb1), (ei2, et2, eb2, rb2)])
                o1, o2 = torch.from_numpy(a1).to(dev), torch.from_numpy(a2).to(dev)
            model.train()
            test_pairs = seeds_test.get((l1, l2), links)
            new1, new2, k1, k2, feed, _ = entr.seed_enlargement_triple_transferring(
                o1, o2, test_pairs[:, 0].tolist(), test_pairs[:, 1].tolist(), st["entropy"], 0, st["seeds"][0], tr1, tr2,
                st["seeds"], eb1, rb1, eb2, rb2, kg1, kg2, args, generator=generator,
                matrix_free=getattr(args, "entr_matrix_free", False))
            kg1.triple_keys, kg2.triple_keys = k1, k2
            kg1.transferred_triples, kg2.transferred_triples = new1, new2
            st["feeddict"] = feed
            st["g1"] = entr.align_data_processing(new1, dev)           # train-mode graph: head <- tail, one direction
            st["g2"] = entr.align_data_processing(new2, dev)
            st["tr"] = (new1, new2)
            tables = st.get("completion", {}).get("neighbors")
            st["completion"] = {}                                      # "filtered": samplers and captured steps of this refresh
            if getattr(args, "neg_sampler", "uniform") == "truncated":  # the tables outlive it: refreshed in place, from the
                comp = (torch.from_numpy(c1).to(dev), torch.from_numpy(c2).to(dev))      # normalised completion embeddings
                st["completion"]["neighbors"] = neighbor_tables(comp, (kg1.num_entity, kg2.num_entity), args, tables)
        (ei1, et1), (ei2, et2) = st["g1"], st["g2"]
        closs = train_completion_component(model, opt_c, ei1, et1, ei2, et2, st["feeddict"], st["tr"][0], st["tr"][1],
                                           kg1.num_entity, kg2.num_entity, args, generator, state=st["completion"])
        aloss = train_alignment_component(model, opt_a, ei1, et1, ei2, et2, st["feeddict"])
        log.append({"pair": (l1, l2), "completion_loss": closs, "align_loss": aloss, "links": len(st["feeddict"]["links"]),
                    "triples": (len(st["tr"][0]), len(st["tr"][1])), "entropy": st["entropy"][0]})
    return log
