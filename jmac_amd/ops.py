"""torch.autograd.Function wrappers over the C ABI (include/jmac_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic step of the hot path
runs in libjmac_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from ._lib import check, lib, ptr, require_device, stream, testing_lib, workspace
from .graph import RelGraph

BWD_MODE_ATOMIC = 0            # testing build only (libjmac_hip_testing.so): float atomics, a second implementation for the tests
BWD_MODE_DETERMINISTIC = 1

# bench.py sets this to a list to collect (name, start_event, end_event) around the aggregation launches;
# events are recorded on the stream the kernels are launched on (torch's current stream).
PROFILE = None


def _ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _launch(fn, args, name: str) -> None:
    """check(fn(*args)), between two PROFILE events recorded as ``name`` while PROFILE is a list."""
    if PROFILE is None:
        check(fn(*args), fn.__name__)
        return
    ev0 = _ev()
    check(fn(*args), fn.__name__)
    PROFILE.append((name, ev0, _ev()))


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError("jmac_amd ops compute in fp32 (got %s)" % t.dtype)
    return t


def _table(t: torch.Tensor) -> torch.Tensor:
    """Gathered tables: fp32, or bf16 for the inference form (arithmetic and outputs stay fp32)."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("jmac_amd tables are fp32 or bf16 (got %s)" % t.dtype)
    return t


def bf16_pad(d: int) -> int:
    """Half pitch of the PADDED bf16 tables the half-wave aggregation kernel reads (16-byte aligned halves: a multiple of
    8 elements): d = 300 -> 304; d itself where no padded form exists."""
    return 304 if d == 300 else d


def pad_table_weight(w: torch.Tensor, d: int, parts: int) -> torch.Tensor:
    """[k, parts*d] projection weight -> [k, parts*bf16_pad(d)] with zero pad columns behind every d-wide part: the GEMM then
    writes [P|Q|Z] / [Rq|Rz] rows in the padded layout, pad columns zero."""
    dh = bf16_pad(d)
    if dh == d:
        return w
    out = w.new_zeros((w.shape[0], parts * dh))
    for p_ in range(parts):
        out[:, p_ * dh:p_ * dh + d] = w[:, p_ * d:(p_ + 1) * d]
    return out


def pad_table(t: torch.Tensor, d: int, parts: int) -> torch.Tensor:
    """[n, parts*d] table -> the padded layout [n, parts*bf16_pad(d)] (zero pad columns); benchmarks and tests that build
    their tables directly use it -- the layers get the layout from the GEMM (pad_table_weight)."""
    return pad_table_weight(t, d, parts)


def pqz_views(PQZ: torch.Tensor):
    """P and [Q|Z]: column views of a [P|Q|Z] table (half pitch PQZ.shape[1] // 3), as the raw forms below take them."""
    dh = PQZ.shape[1] // 3
    return PQZ[:, :dh], PQZ[:, dh:]


class _RelAttnAggregate(torch.autograd.Function):
    """out = out_scale * ( sqrt(deg) * softmax-weighted sum over in-edges of (Z[j]-Rz[t]) + [Z[i]-Rz[loop]] ).

    PQZ: [N, 3d] = P | Q | Z (one GEMM output), RR: [nrel, 2d] = Rq | Rz, a: [d].
    """

    @staticmethod
    def forward(ctx, PQZ, RR, a, graph: RelGraph, slope: float, loop_rel: int, out_scale: float, bwd_mode: int):
        require_device(PQZ, RR, a)
        PQZ, RR, a = _table(PQZ).contiguous(), _table(RR).contiguous(), _f32c(a).contiguous()
        out, seg_max, seg_den = rel_attn_split_fwd_raw(*pqz_views(PQZ), RR, a, graph, slope, out_scale, loop_rel, 0)
        if PQZ.dtype == torch.bfloat16:
            ctx.mark_non_differentiable(out)
            return out
        ctx.save_for_backward(PQZ, RR, a, out, seg_max, seg_den)
        ctx.graph, ctx.slope, ctx.loop_rel, ctx.out_scale, ctx.bwd_mode = graph, slope, loop_rel, out_scale, bwd_mode
        return out

    @staticmethod
    def backward(ctx, G):
        PQZ, RR, a, out, seg_max, seg_den = ctx.saved_tensors
        dPQZ = torch.empty_like(PQZ)
        _, _, dRR, da = rel_attn_split_bwd_raw(*pqz_views(PQZ), RR, a, ctx.graph, ctx.slope, ctx.out_scale, ctx.loop_rel, 0, out,
                                               seg_max, seg_den, G, mode=int(ctx.bwd_mode), dPQZ=dPQZ)
        return dPQZ, dRR, da, None, None, None, None, None


def rel_attn_aggregate(PQZ: torch.Tensor, RR: torch.Tensor, a: torch.Tensor, graph: RelGraph, slope: float,
                       loop_rel: int = -1, out_scale: float = 1.0,
                       bwd_mode: int = BWD_MODE_DETERMINISTIC) -> torch.Tensor:
    if PQZ.dtype == torch.bfloat16 and torch.is_grad_enabled() and (PQZ.requires_grad or RR.requires_grad or a.requires_grad):
        raise RuntimeError("bf16 tables are the inference form of the op (no backward): run under torch.no_grad()")
    return _RelAttnAggregate.apply(PQZ, RR, a, graph, float(slope), int(loop_rel), float(out_scale), int(bwd_mode))


def _fwd_call(P, QZ, RR, a, graph: RelGraph, slope: float, out_scale: float, loop_rel: int, self_off: int, compact: bool,
              lanes64: bool = False):
    """(entry point, arguments, (out, seg_max, seg_den), workspace) of one forward aggregation.  The arguments of the fp32 form
    without the stream are the fields of an AggFwdJob (jmac_rel_attn_aggregate_fwd_jobs_f32).  ``lanes64``: the testing
    build's entry point of the same signature (rel_attn_split_fwd_raw)."""
    if QZ.dtype != P.dtype or RR.dtype != P.dtype:
        raise TypeError("P, QZ and RR must share a dtype")
    N, dh, d = P.shape[0], P.shape[1], int(a.numel())      # dh: half pitch of the table rows; > d for padded bf16 tables
    bf16 = P.dtype == torch.bfloat16
    if dh != d and not (bf16 and dh == bf16_pad(d) and RR.shape[1] == 2 * dh):
        raise ValueError("tables of half pitch %d do not go with a_att of %d elements" % (dh, d))
    if graph.N != N or graph.num_src != QZ.shape[0] or QZ.shape[1] != 2 * dh:
        raise ValueError("graph / table shapes disagree")
    L = lib()
    dev = P.device
    out = torch.empty((N, d), dtype=torch.float32, device=dev)
    seg_max = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
    seg_den = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
    s = graph.by_dst
    ws_bytes = int(L.jmac_rel_attn_fwd_workspace_bytes(s.n_parts_max, d))
    ws = workspace(ws_bytes, dev)
    # compact: RR holds the rows of graph.rel_used + the loop row (RelGraph.ensure_rel_compact)
    etype, view = (graph.etype_c, s.view_compact(graph.col, graph.etype_c)) if compact else (graph.etype, s.view())
    if lanes64:                                         # fp32 tables, or bf16 tables in the padded layout (pitch = d where no pad)
        T = testing_lib()
        fn, pitch = (T.jmac_rel_attn_aggregate_fwd_lanes64_bf16_padded, (dh,)) if bf16 else (T.jmac_rel_attn_aggregate_fwd_lanes64_f32, ())
    elif dh != d:                                       # the padded form takes the half pitch after ldrr
        fn, pitch = L.jmac_rel_attn_aggregate_fwd_bf16_padded, (dh,)
    else:
        fn, pitch = (L.jmac_rel_attn_aggregate_fwd_bf16 if bf16 else L.jmac_rel_attn_aggregate_fwd_f32), ()
    args = (ptr(P), P.stride(0), ptr(QZ), QZ.stride(0), ptr(RR), RR.stride(0), *pitch, ptr(a), ptr(graph.col), ptr(etype),
            C.pointer(view), N, d, float(slope), int(loop_rel), int(self_off), float(out_scale), ptr(out), d, ptr(seg_max),
            ptr(seg_den), ptr(ws), ws_bytes, stream())
    return fn, args, (out, seg_max, seg_den), ws


def rel_attn_split_fwd_raw(P, QZ, RR, a, graph: RelGraph, slope: float, out_scale: float, loop_rel: int, self_off: int, *,
                           compact: bool = False, lanes64: bool = False):
    """The forward aggregation without autograd on P [N_dst, dh] and QZ [N_src, 2dh] -- separate tables, or the column views
    of one [P|Q|Z] table (pqz_views): out [N, d] and the per-destination softmax (max, denominator).  d = a.numel(); the half
    pitch dh is d, or bf16_pad(d) for padded bf16 tables.  ``compact``: the edge types and RR's rows are in the compact
    relation numbering (RelGraph.ensure_rel_compact).  ``lanes64`` (parity tests): the testing build's entry point, which keeps
    the 64-lane kernels where the product takes the half-wave kernel."""
    fn, args, res, ws = _fwd_call(P, QZ, RR, a, graph, slope, out_scale, loop_rel, self_off, compact, lanes64)
    _launch(fn, args, "rel_attn_fwd_bf16" if P.dtype == torch.bfloat16 else "rel_attn_fwd")
    return res


class _AggBackward:
    """Outputs, views and workspace of one backward aggregation, and the argument tuple that jmac_rel_attn_aggregate_bwd_f32
    and jmac_rel_attn_aggregate_bwd_phases_f32 both take (the int before ws: ``mode`` in the first, ``phases`` in the
    second).  ``dPQZ``: an [N, 3d] buffer whose column views receive dP and d[Q|Z] (callers that hold one [P|Q|Z] table)."""

    def __init__(self, P, QZ, RR, a, graph: RelGraph, slope: float, out_scale: float, loop_rel: int, self_off: int, out, seg_max,
                 seg_den, G, compact: bool = False, mode: int = BWD_MODE_DETERMINISTIC, dPQZ=None):
        self.L = lib() if mode == BWD_MODE_DETERMINISTIC else testing_lib()      # mode 0 exists in the testing build only
        self.P, self.QZ, self.RR, self.a, self.graph = P, QZ, RR, a, graph
        self.slope, self.out_scale, self.loop_rel, self.self_off = float(slope), float(out_scale), int(loop_rel), int(self_off)
        self.out, self.seg_max, self.seg_den, self.G = out, seg_max, seg_den, _f32c(G).contiguous()
        self.N, self.d, self.nsrc, self.nrel = P.shape[0], int(a.numel()), QZ.shape[0], RR.shape[0]
        if mode:                          # mode 0 reads the by-destination view only
            if compact:
                graph.ensure_backward_views_compact()
            else:
                graph.ensure_backward_views()
        by_rel = graph.by_rel_c if compact else graph.by_rel
        self.etype = graph.etype_c if compact else graph.etype
        self.dst_of_slot = graph.dst_of_slot if mode else None
        self.vd = graph.by_dst_bwd.view_compact(graph.col, graph.etype_c) if compact else graph.by_dst_bwd.view()
        self.vs = graph.by_src.view() if mode else None
        self.vr = by_rel.view() if mode else None
        self.dP, self.dQZ = pqz_views(dPQZ) if dPQZ is not None else (torch.empty_like(P), torch.empty_like(QZ))
        self.dRR, self.da = torch.empty_like(RR), torch.empty_like(a)
        self.ws_bytes = int(self.L.jmac_rel_attn_bwd_workspace_bytes(
            self.N, graph.E, self.nrel, self.d, graph.by_dst_bwd.n_parts_max, graph.by_src.n_parts_max if mode else 0,
            by_rel.n_parts_max if mode else 0, mode))
        self.ws = workspace(self.ws_bytes, P.device)

    def args(self, flag: int, src_view, row0: int, rows: int) -> tuple:
        """Arguments of a call whose pass B covers source rows [row0, row0 + rows) of d[Q|Z] through ``src_view``."""
        g, dQZ = self.graph, self.dQZ
        return (ptr(self.P), self.P.stride(0), ptr(self.QZ), self.QZ.stride(0), ptr(self.RR), self.RR.stride(0), ptr(self.a),
                ptr(g.col), ptr(self.etype), ptr(self.dst_of_slot), C.byref(self.vd),
                C.byref(src_view) if src_view is not None else None, C.byref(self.vr) if self.vr is not None else None,
                self.N, rows, g.E, self.nrel, self.d, self.slope, self.loop_rel, self.self_off - row0, self.out_scale,
                ptr(self.out), self.out.stride(0), ptr(self.seg_max), ptr(self.seg_den), ptr(self.G), self.G.stride(0),
                ptr(self.dP), self.dP.stride(0), dQZ.data_ptr() + row0 * dQZ.stride(0) * dQZ.element_size(), dQZ.stride(0),
                ptr(self.dRR), self.dRR.stride(0), ptr(self.da), int(flag), ptr(self.ws), self.ws_bytes, stream())


def rel_attn_split_bwd_raw(P, QZ, RR, a, graph: RelGraph, slope: float, out_scale: float, loop_rel: int, self_off: int,
                           out, seg_max, seg_den, G, *, compact: bool = False, mode: int = BWD_MODE_DETERMINISTIC, dPQZ=None):
    """jmac_rel_attn_aggregate_bwd_f32 on the tables of rel_attn_split_fwd_raw: dP, dQZ, dRR, da (``dPQZ``: see _AggBackward).
    ``mode``: BWD_MODE_DETERMINISTIC, or BWD_MODE_ATOMIC (testing build)."""
    b = _AggBackward(P, QZ, RR, a, graph, slope, out_scale, loop_rel, self_off, out, seg_max, seg_den, G, compact, mode, dPQZ)
    _launch(b.L.jmac_rel_attn_aggregate_bwd_f32, b.args(mode, b.vs, 0, b.nsrc), "rel_attn_bwd")
    return b.dP, b.dQZ, b.dRR, b.da


PHASE_A, PHASE_B, PHASE_C, PHASE_M, PHASE_ALL = 1, 2, 4, 8, 15


class SplitBackwardPhases(_AggBackward):
    """jmac_rel_attn_aggregate_bwd_phases_f32 on the split tables: the deterministic backward as separately launched phases --
    pass A (+ pass C and the merges that hang on them) first, then pass B over SLABS of the source rows, each slab's d[Q|Z] rows
    complete when its call returns to the stream (the caller queues that slab's reduce-scatter and goes on with the next slab).
    ``slab_bounds``: ascending source-row bounds from 0 to the table's rows.  Results equal rel_attn_split_bwd_raw's bit for bit
    (the same kernels on the same items in the same order per output row)."""

    def __init__(self, P, QZ, RR, a, graph: RelGraph, slope: float, out_scale: float, loop_rel: int, self_off: int, out, seg_max,
                 seg_den, G, slab_bounds):
        super().__init__(P, QZ, RR, a, graph, slope, out_scale, loop_rel, self_off, out, seg_max, seg_den, G)
        self.bounds = [int(b) for b in slab_bounds]
        self.slabs = graph.src_slab_views(self.bounds)

    def _call(self, phases: int, src_view, row0: int, rows: int) -> None:
        _launch(self.L.jmac_rel_attn_aggregate_bwd_phases_f32, self.args(phases, src_view, row0, rows),
                "rel_attn_bwd_phase%d" % phases)

    def begin(self) -> None:
        """Pass A, pass C and every merge but the by-source one: dP, dRR, da are final afterwards."""
        self._call(PHASE_A | PHASE_C | PHASE_M, self.vs, 0, self.nsrc)

    def slab(self, c: int) -> torch.Tensor:
        """Pass B on source rows [bounds[c], bounds[c+1]): returns that slice of d[Q|Z] (final once the stream reaches here)."""
        r0, r1 = self.bounds[c], self.bounds[c + 1]
        if r1 > r0:
            self._call(PHASE_B, self.slabs[c].view(), r0, r1 - r0)
        return self.dQZ[r0:r1]


def softmax_parts_merge(parts, N: int, d: int, device, zself=None, rz_loop=None, out_scale: float = 1.0):
    """jmac_softmax_parts_merge_f32: parts = [(out_c [N,d], seg_max_c [N], seg_den_c [N], rowptr_c [N+1] int32), ...] of the
    same destinations over disjoint edge sets -> (out [N,d], seg_max [N], seg_den [N]) of their union; out = out_scale * (nb +
    zself[i] - rz_loop) with a self table (zself: [N, d] rows with any 4-aligned stride, rz_loop [d]), else out_scale * nb."""
    L = lib()
    n = len(parts)
    out = torch.empty((N, d), dtype=torch.float32, device=device)
    seg_max = torch.empty(max(N, 1), dtype=torch.float32, device=device)
    seg_den = torch.empty(max(N, 1), dtype=torch.float32, device=device)
    arr = lambda k: (C.c_void_p * max(n, 1))(*[ptr(p[k]) for p in parts])
    for o, m, l, rp in parts:
        require_device(o, m, l, rp)
        if o.shape != (N, d) or not o.is_contiguous() or rp.dtype != torch.int32 or rp.numel() != N + 1:
            raise ValueError("softmax_parts_merge: part shapes disagree")
    if zself is not None:
        require_device(zself, rz_loop)
        if zself.shape != (N, d) or zself.stride(1) != 1 or rz_loop.numel() != d or not rz_loop.is_contiguous():
            raise ValueError("softmax_parts_merge: self table shapes disagree")
    if n == 0:                       # no edges at all: the kernel is not given anything to read
        seg_max.fill_(float("-inf"))
        seg_den.zero_()
        if zself is None or N == 0:
            out.zero_()
            return out, seg_max, seg_den
    check(L.jmac_softmax_parts_merge_f32(arr(0), d, arr(1), arr(2), arr(3), n, N, d,
                                         ptr(zself) if zself is not None else None, zself.stride(0) if zself is not None else 0,
                                         ptr(rz_loop) if zself is not None else None, float(out_scale), ptr(out), d, ptr(seg_max),
                                         ptr(seg_den), stream()), "jmac_softmax_parts_merge_f32")
    return out, seg_max, seg_den


class _RelAttnAggregateSplit(torch.autograd.Function):
    """Same op with P [N_dst, d] and QZ [N_src, 2d] as separate tables (destination-sharded multi-GPU: P holds
    the rank's rows, QZ the all-gathered table).  The fused self term reads QZ[self_off + i] (loop_rel < 0: none)."""

    @staticmethod
    def forward(ctx, P, QZ, RR, a, graph: RelGraph, slope: float, out_scale: float, loop_rel: int, self_off: int):
        require_device(P, QZ, RR, a)
        P, QZ, RR, a = _f32c(P).contiguous(), _f32c(QZ).contiguous(), _f32c(RR).contiguous(), _f32c(a).contiguous()
        out, seg_max, seg_den = rel_attn_split_fwd_raw(P, QZ, RR, a, graph, slope, out_scale, loop_rel, self_off)
        ctx.save_for_backward(P, QZ, RR, a, out, seg_max, seg_den)
        ctx.graph, ctx.slope, ctx.out_scale, ctx.loop_rel, ctx.self_off = graph, slope, out_scale, int(loop_rel), int(self_off)
        return out

    @staticmethod
    def backward(ctx, G):
        P, QZ, RR, a, out, seg_max, seg_den = ctx.saved_tensors
        dP, dQZ, dRR, da = rel_attn_split_bwd_raw(P, QZ, RR, a, ctx.graph, ctx.slope, ctx.out_scale, ctx.loop_rel, ctx.self_off,
                                                  out, seg_max, seg_den, G)
        return dP, dQZ, dRR, da, None, None, None, None, None


def rel_attn_aggregate_split(P, QZ, RR, a, graph: RelGraph, slope: float, out_scale: float = 1.0, loop_rel: int = -1,
                             self_off: int = 0) -> torch.Tensor:
    return _RelAttnAggregateSplit.apply(P, QZ, RR, a, graph, float(slope), float(out_scale), int(loop_rel), int(self_off))


class EdgeAttention(NamedTuple):
    """What rel_attn_edge_weights returns; a field that was not asked for is None."""
    alpha: torch.Tensor                      # [E] fp32, the caller's edge order
    logit: Optional[torch.Tensor]            # [E] fp32
    entropy: Optional[torch.Tensor]          # [N] fp32, of the unscaled alpha; 0 for a destination without in-edges
    argmax: Optional[torch.Tensor]           # [N] int64, original edge id of the largest alpha; -1 without in-edges


def rel_attn_edge_weights(P, QZ, RR, a, graph: RelGraph, slope: float, scale_by_degree: bool = False, logits: bool = False,
                          stats: bool = False, dh: Optional[int] = None, slot_order: bool = False) -> EdgeAttention:
    """jmac_rel_attn_edge_weights_*: alpha = softmax over the in-edges of every destination of s_e = a . LeakyReLU(P[i] + Q[j] -
    Rq[t]) -- the weights the forward aggregation applies and never writes -- on the tables rel_attn_split_fwd_raw takes (P
    [N, dh], QZ [Nsrc, >= dh] with Q in front, RR likewise; fp32, or bf16 in the padded layout with half pitch ``dh``, default
    P.shape[1]).  ``scale_by_degree``: alpha * sqrt(deg), the factor on the layer's messages.  ``logits``: also s; ``stats``: also
    the entropy and the argmax edge of every destination.  Outputs indexed by edge follow ``graph``'s input edge order
    (``slot_order``: the CSR slot order instead, argmax then names slots).  No autograd: a read-out."""
    require_device(P, QZ, RR, a)
    if QZ.dtype != P.dtype or RR.dtype != P.dtype:
        raise TypeError("P, QZ and RR must share a dtype")
    _table(P), _f32c(a)
    a = a.contiguous()
    N, d = P.shape[0], int(a.numel())
    dh = int(P.shape[1] if dh is None else dh)
    bf16 = P.dtype == torch.bfloat16
    if dh != d and not (bf16 and dh == bf16_pad(d)):
        raise ValueError("tables of half pitch %d do not go with a_att of %d elements" % (dh, d))
    if P.shape[1] < dh or QZ.shape[1] < dh or RR.shape[1] < dh or min(P.stride(1), QZ.stride(1), RR.stride(1)) != 1:
        raise ValueError("table rows are shorter than the half pitch %d, or not row-major" % dh)
    if graph.N != N or graph.num_src > QZ.shape[0] or graph.num_rel > RR.shape[0]:
        raise ValueError("graph / table shapes disagree")
    L = lib()
    dev, E = P.device, graph.E
    alpha = torch.empty(E, dtype=torch.float32, device=dev)
    logit = torch.empty(E, dtype=torch.float32, device=dev) if logits else None
    entropy = torch.empty(N, dtype=torch.float32, device=dev) if stats else None
    argmax = torch.empty(N, dtype=torch.int32, device=dev) if stats else None
    ws_bytes = int(L.jmac_rel_attn_edge_weights_workspace_bytes(N, E))
    ws = workspace(ws_bytes, dev)
    fn, pitch = (L.jmac_rel_attn_edge_weights_bf16, (dh,)) if bf16 else (L.jmac_rel_attn_edge_weights_f32, ())
    args = (ptr(P), P.stride(0), ptr(QZ), QZ.stride(0), ptr(RR), RR.stride(0), *pitch, ptr(a), ptr(graph.col), ptr(graph.etype),
            None if slot_order else ptr(graph.perm), C.pointer(graph.by_dst.view()), N, E, d, float(slope),
            1 if scale_by_degree else 0, ptr(alpha) if E > 0 else None, ptr(logit) if E > 0 else None, ptr(entropy), ptr(argmax),
            ptr(ws), ws_bytes, stream())
    _launch(fn, args, "rel_attn_edge_weights_bf16" if bf16 else "rel_attn_edge_weights")
    return EdgeAttention(alpha, logit, entropy, argmax.long() if stats else None)


def bn_tanh_fwd_raw(x, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float, y, y2=None,
                    seg=None):
    """tanh(BatchNorm1d(x)) into y (and y2, may be None) with nn.BatchNorm1d's running-estimate update (src/jmac_model.py:52;
    num_batches_tracked is the caller's): jmac_bn_tanh_fwd2_f32, or jmac_bn_tanh_seg_fwd2_f32 for batch statistics over the
    row blocks of ``seg`` (encoder.RowBlocks, more than one block): every block is normalised with ITS statistics and the
    running estimates move once per block.  -> (save_mean, save_invstd): [d], or [blocks, d] from the segmented form."""
    L = lib()
    N, d = x.shape
    dev = x.device
    ldy2 = y2.stride(0) if y2 is not None else 0
    if training and seg is not None and seg.nb > 1:
        if seg.offsets[-1] != N:
            raise ValueError("RowBlocks cover %d rows, the layer has %d" % (seg.offsets[-1], N))
        mean = torch.empty((seg.nb, d), dtype=torch.float32, device=dev)
        invstd = torch.empty((seg.nb, d), dtype=torch.float32, device=dev)
        ws_bytes = int(L.jmac_bn_tanh_seg_workspace_bytes(seg.nb, d))
        ws = workspace(ws_bytes, dev)
        check(L.jmac_bn_tanh_seg_fwd2_f32(ptr(x), x.stride(0), d, seg.nb, seg.c_ptr, seg.c_order, ptr(weight), ptr(bias),
                                          ptr(running_mean), ptr(running_var), float(momentum), float(eps), ptr(y), y.stride(0),
                                          ptr(y2), ldy2, ptr(mean), ptr(invstd), ptr(ws), ws_bytes, stream()),
              "jmac_bn_tanh_seg_fwd2_f32")
        return mean, invstd
    mean = torch.empty(d, dtype=torch.float32, device=dev)
    invstd = torch.empty(d, dtype=torch.float32, device=dev)
    ws_bytes = int(L.jmac_bn_tanh_workspace_bytes(N, d))
    ws = workspace(ws_bytes, dev)
    check(L.jmac_bn_tanh_fwd2_f32(ptr(x), x.stride(0), N, d, ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var),
                                  1 if training else 0, float(momentum), float(eps), ptr(y), y.stride(0), ptr(y2), ldy2, ptr(mean),
                                  ptr(invstd), ptr(ws), ws_bytes, stream()), "jmac_bn_tanh_fwd2_f32")
    return mean, invstd


def bn_tanh_bwd_raw(x, y, gy, gy2, weight, mean, invstd, training: bool, seg=None):
    """Backward of bn_tanh_fwd_raw, the incoming gradients gy + gy2 (gy2 may be None) summed as the kernel reads them: gx [N, d]
    and [grad bias | grad weight] [2d] (one reduction writes both).  ``seg``: the forward's RowBlocks where its statistics are
    per block (mean / invstd [blocks, d])."""
    L = lib()
    N, d = x.shape
    dev = x.device
    gx = torch.empty((N, d), dtype=torch.float32, device=dev)
    gbw = torch.empty(2 * d, dtype=torch.float32, device=dev)
    ldgy2 = gy2.stride(0) if gy2 is not None else 0
    if mean.dim() == 2:                                        # per-block statistics (segmented forward)
        ws_bytes = int(L.jmac_bn_tanh_seg_workspace_bytes(seg.nb, d))
        ws = workspace(ws_bytes, dev)
        check(L.jmac_bn_tanh_seg_bwd2_f32(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(gy), gy.stride(0), ptr(gy2), ldgy2, d,
                                          seg.nb, seg.c_ptr, ptr(weight), ptr(mean), ptr(invstd), ptr(gx), d,
                                          gbw.data_ptr() + d * 4, ptr(gbw), ptr(ws), ws_bytes, stream()),
              "jmac_bn_tanh_seg_bwd2_f32")
        return gx, gbw
    ws_bytes = int(L.jmac_bn_tanh_workspace_bytes(N, d))
    ws = workspace(ws_bytes, dev)
    check(L.jmac_bn_tanh_bwd2_f32(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(gy), gy.stride(0), ptr(gy2), ldgy2, N, d,
                                  ptr(weight), ptr(mean), ptr(invstd), 1 if training else 0, ptr(gx), d, gbw.data_ptr() + d * 4,
                                  ptr(gbw), ptr(ws), ws_bytes, stream()), "jmac_bn_tanh_bwd2_f32")
    return gx, gbw


def _seed_args(drop):
    """(seed pointer, p_drop) of a SEED-form dropout state ``("seed", tensor, p_drop)`` or None (no dropout)."""
    if drop is None:
        return None, 0.0
    if drop[0] != "seed":
        raise ValueError("the fused row passes draw from a device seed (mask-form dropout keeps the separate launches)")
    return ptr(drop[1]), float(drop[2])


def bn_tanh_norm_fwd_raw(x, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float, y, yn, drop,
                         row_map=None, y_rows=None):
    """bn_tanh_fwd_raw whose apply pass also writes F.normalize + dropout of the output rows into ``yn`` (a cat operand) and, with a
    ``row_map`` (int64 [N]), row r to ``y_rows[row_map[r]]``: jmac_bn_tanh_normalize_dropseed_fwd_f32 -> (save_mean, save_invstd,
    inv).  ``drop``: ("seed", tensor, p_drop) or None."""
    L = lib()
    N, d = x.shape
    dev = x.device
    mean = torch.empty(d, dtype=torch.float32, device=dev)
    invstd = torch.empty(d, dtype=torch.float32, device=dev)
    inv = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
    seed, p_drop = _seed_args(drop)
    ws_bytes = int(L.jmac_bn_tanh_workspace_bytes(N, d))
    ws = workspace(ws_bytes, dev)
    check(L.jmac_bn_tanh_normalize_dropseed_fwd_f32(ptr(x), x.stride(0), N, d, ptr(weight), ptr(bias), ptr(running_mean),
                                                    ptr(running_var), 1 if training else 0, float(momentum), float(eps), ptr(y),
                                                    y.stride(0), ptr(row_map), ptr(y_rows), y_rows.stride(0) if y_rows is not None else 0,
                                                    1e-12, seed, p_drop, ptr(yn), yn.stride(0), ptr(inv), ptr(mean), ptr(invstd),
                                                    ptr(ws), ws_bytes, stream()), "jmac_bn_tanh_normalize_dropseed_fwd_f32")
    return mean, invstd, inv


def bn_tanh_bwd_normadj_raw(x, y, inv, drop, g, gy2, row_map, weight, mean, invstd, training: bool):
    """bn_tanh_bwd_raw whose first incoming gradient is the normalise + dropout adjoint of ``g`` (rows of a cat adjoint; the
    adjoint's x is ``y``), formed per row inside both passes instead of being written as a table; ``gy2`` (may be None) is read
    through ``row_map`` (may be None): jmac_bn_tanh_bwd_normadj_f32 -> gx [N, d], [grad bias | grad weight] [2d]."""
    L = lib()
    N, d = x.shape
    dev = x.device
    gx = torch.empty((N, d), dtype=torch.float32, device=dev)
    gbw = torch.empty(2 * d, dtype=torch.float32, device=dev)
    seed, p_drop = _seed_args(drop)
    ws_bytes = int(L.jmac_bn_tanh_workspace_bytes(N, d))
    ws = workspace(ws_bytes, dev)
    check(L.jmac_bn_tanh_bwd_normadj_f32(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(inv), ptr(g), g.stride(0), 1e-12, seed, p_drop,
                                         ptr(gy2), gy2.stride(0) if gy2 is not None else 0, ptr(row_map), N, d, ptr(weight), ptr(mean),
                                         ptr(invstd), 1 if training else 0, ptr(gx), d, gbw.data_ptr() + d * 4, ptr(gbw), ptr(ws),
                                         ws_bytes, stream()), "jmac_bn_tanh_bwd_normadj_f32")
    return gx, gbw


class _BnTanh(torch.autograd.Function):
    """tanh(BatchNorm1d(x)) with nn.BatchNorm1d semantics (src/jmac_model.py:52)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float):
        require_device(x, weight, bias)
        x = _f32c(x).contiguous()
        y = torch.empty_like(x)
        save_mean, save_invstd = bn_tanh_fwd_raw(x, weight, bias, running_mean, running_var, training, momentum, eps, y)
        ctx.save_for_backward(x, y, weight, save_mean, save_invstd)
        ctx.training = training
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, weight, save_mean, save_invstd = ctx.saved_tensors
        d = x.shape[1]
        gx, gbw = bn_tanh_bwd_raw(x, y, _f32c(gy).contiguous(), None, weight, save_mean, save_invstd, ctx.training)
        return gx, gbw[d:], gbw[:d], None, None, None, None, None


def bn_tanh(x, weight, bias, running_mean, running_var, training: bool, momentum: float = 0.1, eps: float = 1e-5):
    if x.shape[1] % 4 != 0:
        raise ValueError("bn_tanh needs d % 4 == 0 (pad on the host)")
    return _BnTanh.apply(x, weight, bias, running_mean, running_var, bool(training), float(momentum), float(eps))


# ---- small fp32 GEMM (relation-side projections) -----------------------------------------------------------------
def _gemm(A, ta, B, tb, M, N, K):
    C_ = torch.empty((M, N), dtype=torch.float32, device=A.device)
    check(lib().jmac_gemm_f32(ptr(A), A.stride(0), 1 if ta else 0, ptr(B), B.stride(0), 1 if tb else 0, M, N, K, ptr(C_), N,
                              stream()), "jmac_gemm_f32")
    return C_


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    return t if (t.dim() == 2 and t.stride(1) == 1) else t.contiguous()


class _SmallMM(torch.autograd.Function):
    """C = A @ B on jmac_gemm_f32 with its two backward forms (dA = G B^T, dB = A^T G)."""

    @staticmethod
    def forward(ctx, A, B):
        require_device(A, B)
        A, B = _rowmajor(_f32c(A)), _rowmajor(_f32c(B))
        if A.shape[1] != B.shape[0]:
            raise ValueError("small_mm: %s @ %s" % (tuple(A.shape), tuple(B.shape)))
        ctx.save_for_backward(A, B)
        return _gemm(A, False, B, False, A.shape[0], B.shape[1], A.shape[1])

    @staticmethod
    def backward(ctx, G):
        A, B = ctx.saved_tensors
        G = _rowmajor(_f32c(G))
        M, K = A.shape
        N = B.shape[1]
        dA = _gemm(G, False, B, True, M, K, N) if ctx.needs_input_grad[0] else None      # [M,N] x [K,N]^T
        dB = _gemm(A, True, G, False, K, N, M) if ctx.needs_input_grad[1] else None      # [M,K]^T x [M,N]
        return dA, dB


def _gemm_any(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """A @ B on jmac_gemm_f32 for operands that may be transposed views (``x.t()`` is passed as a transposed operand,
    not copied)."""
    def operand(t):
        if t.stride(1) == 1:
            return t, False
        if t.stride(0) == 1:
            return t.t(), True                                   # stored [cols, rows] row-major
        return t.contiguous(), False
    (a, ta), (b, tb) = operand(A), operand(B)
    return _gemm(a, ta, b, tb, A.shape[0], B.shape[1], A.shape[1])


# Row bound below which the layer routes its relation-side products (962 rows per DBP-5L KG) through small_mm.
# 0 = off (default): measured inside the training step the kernel takes 10.5-15 us per product against the library's
# 17 us untuned -- and 8-9 us once torch's TunableOp has picked the library kernel for the shape (bench.py turns it
# on), so the library keeps these.  The op stays available (deterministic summation order, any strides / transposes).
SMALL_MM_MAX_ROWS = 0


def small_mm(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """``torch.mm`` for the relation-side products ([~10^3, d] x [d, d..2d]): one 32x32 tile per 4-wave block, K split
    over the waves, fragments straight from L2 -- ~4 us where the library GEMM takes ~17 us."""
    return _SmallMM.apply(A, B)


# ---- row L2 normalisation (F.normalize(x, 2, -1)) ------------------------------------------------------------------
class _RowNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        require_device(x)
        x = _rowmajor(_f32c(x))
        N, d = x.shape
        y = torch.empty((N, d), dtype=torch.float32, device=x.device)
        inv = torch.empty(max(N, 1), dtype=torch.float32, device=x.device)
        check(lib().jmac_row_normalize_fwd_f32(ptr(x), x.stride(0), N, d, float(eps), ptr(y), d, ptr(inv), stream()),
              "jmac_row_normalize_fwd_f32")
        ctx.save_for_backward(y, inv)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, g):
        y, inv = ctx.saved_tensors
        g = _rowmajor(_f32c(g))
        N, d = y.shape
        gx = torch.empty((N, d), dtype=torch.float32, device=y.device)
        check(lib().jmac_row_normalize_bwd_f32(ptr(y), d, ptr(g), g.stride(0), ptr(inv), N, d, ctx.eps, ptr(gx), d, stream()),
              "jmac_row_normalize_bwd_f32")
        return gx, None


def row_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """``F.normalize(x, 2, -1)`` for a 2-D fp32 tensor: one kernel each way instead of norm / clamp / div and their
    six-kernel backward."""
    return _RowNormalize.apply(x, float(eps))


# ---- fp32 GEMM on the bf16 matrix cores (split-bf16, fp32-level accuracy) -------------------------------------------
def gemm_nt_x3(A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``A @ B.t()`` for fp32 row-major A [M,K], B [N,K] on jmac_gemm_nt_x3_f32 (three-term bf16 split, six products,
    fp32 accumulation).  K % 4 == 0; rows 16-byte aligned."""
    require_device(A, B)
    A, B = _rowmajor(_f32c(A)), _rowmajor(_f32c(B))
    M, K = A.shape
    N = B.shape[0]
    if B.shape[1] != K:
        raise ValueError("gemm_nt_x3: %s x %s^T" % (tuple(A.shape), tuple(B.shape)))
    C_ = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=A.device)
    # the testing library only (measured, rejected: DESIGN.md section 5): never the product library
    check(testing_lib().jmac_gemm_nt_x3_f32(ptr(A), A.stride(0), ptr(B), B.stride(0), M, N, K, ptr(C_), C_.stride(0), stream()),
          "jmac_gemm_nt_x3_f32")
    return C_


class _MMx3(torch.autograd.Function):
    """``A @ W`` for an N-row activation A [M,K] and a weight W [K,N]: forward and dA on the split-bf16 matrix-core GEMM
    (both are "NT" products with a k-contiguous weight operand: W^T for the forward, W itself for dA = G W^T); dW = A^T G
    contracts over the M rows (both operands k-strided) and stays on the library GEMM."""

    @staticmethod
    def forward(ctx, A, W):
        ctx.save_for_backward(A, W)
        return gemm_nt_x3(A, W.t().contiguous())

    @staticmethod
    def backward(ctx, G):
        A, W = ctx.saved_tensors
        G = _rowmajor(G)
        dA = gemm_nt_x3(G, W) if ctx.needs_input_grad[0] else None
        dW = torch.mm(A.t(), G) if ctx.needs_input_grad[1] else None
        return dA, dW


def mm_x3(A: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """``torch.mm(A, W)`` on the split-bf16 GEMM (with its backward).  EXPERIMENTAL, not used by the layer or the encoder:
    per product it is as accurate as an fp32 GEMM (3e-7 of sum |a||b|) and as fast as the tuned library kernel (~100
    TFLOP/s at DBP-5L size, 128 vs 101 at 10^6 rows), but v_mfma_f32_32x32x16_bf16 accumulates with a small NEGATIVE BIAS
    (mean signed error -1.3e-8 .. -2.2e-8 of the result on positive data against 2e-10 for the fp32 GEMM, growing with K):
    invisible per element, it adds up coherently in the column sums of the backward -- on the full-size DBP-5L step the
    worst parameter gradient moved from 6e-6 to 7e-4 of its scale, outside the 1e-4 bar."""
    return _MMx3.apply(A, W)
