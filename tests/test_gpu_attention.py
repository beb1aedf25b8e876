"""GPU: the attention export (jmac_rel_attn_edge_weights_*, ops.rel_attn_edge_weights, RelationAwareLayer.attention,
JMAC.attention) against the reference's own softmax (tests/golden/attention.npz) and against the float64 restatement of its
definition (tests/attention_ref.py) evaluated on the tables the device read.

The float64 comparisons hold every edge to the worst-case bound of an fp32 dot product of d terms in any order plus expf,

    |alpha - alpha64| <= alpha64 * (2 d 2^-24 A_i + 16 * 2^-24) + 2^-126,     A_i = max over in(i) of sum_k |a_k| |LeakyReLU(h_e[k])|
    |s - s64|         <= 2 d 2^-24 A_e + 16 * 2^-24

derived, not tuned.  The 2^-126 term is the fp32 format's: a weight below the smallest normal number (the wide-logit case has
float64 weights down to 1e-97) cannot be stored to a relative precision, whatever computes it.  Largest observed ratios to the
bounds on an MI355X: 0.13 (alpha) and 0.30 (logits), both at d = 8 with the wide logits; 0.0016 / 0.0015 at d = 256 and 300
('Attention export')."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_ref import attention_ref
from util import assert_close, load_golden, make_args, random_graph, t

U = 2.0 ** -24
SLOPE = 0.05
N_NODES, N_REL = 60, 12
HUB = 5000


# ---- the graph: every segment class of the by-destination schedule, duplicates, a self edge, a shuffled edge list ------------
def _segment_lengths(chunk):
    """In-degrees: empty, 1, 2, the wave width +-1, the schedule's chunk +-1, the cooperative class (8 < len <= 256), the first
    split length behind it, and one hub longer than one pass of a 256-thread block."""
    from jmac_amd import graph as jg
    lens = [0, 1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, jg.COOP_MIN + 1, 100, jg.COOP_MAX, 257, HUB]
    rng = np.random.default_rng(11)
    lens += rng.integers(0, 13, N_NODES - len(lens)).tolist()
    order = rng.permutation(N_NODES)                                   # the classes are not in node order
    out = np.zeros(N_NODES, dtype=np.int64)
    out[order] = lens
    return out


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(d, kind="f32", a_scale=1.0):
    """Tables, graph and the float64 reference of one configuration, built once and shared (read-only) by the tests."""
    from jmac_amd import graph as jg, ops
    chunk = jg.auto_chunk(HUB + 2000, jg.DST_CHUNK_CAP)
    lens = _segment_lengths(chunk)
    rng = np.random.default_rng(100 + d)
    gen = torch.Generator().manual_seed(200 + d)
    PQZ = torch.randn(N_NODES, 3 * d, generator=gen)
    RR = torch.randn(N_REL, 2 * d, generator=gen)
    a = torch.randn(d, generator=gen) / np.sqrt(d) * a_scale
    if kind == "bf16":
        PQZ, RR = PQZ.to(torch.bfloat16).float(), RR.to(torch.bfloat16).float()     # the values the device will read
    P64, Q64, Z64 = (PQZ[:, k * d:(k + 1) * d].double().numpy() for k in range(3))
    Rq64, Rz64, a64 = RR[:, :d].double().numpy(), RR[:, d:].double().numpy(), a.double().numpy()
    # destinations that end in an exact tie of their largest weight: one edge short, then their float64 argmax edge again
    tie_nodes = [int(np.flatnonzero(lens == L)[0]) for L in (2, chunk + 1, 100, HUB)]
    base = lens.copy()
    base[tie_nodes] -= 1
    dst = np.repeat(np.arange(N_NODES), base)
    src = rng.integers(0, N_NODES, dst.size)
    typ = rng.integers(0, N_REL, dst.size)
    src[np.flatnonzero(dst == tie_nodes[1])[0]] = tie_nodes[1]          # a self edge
    r0 = attention_ref(P64, Q64, Rq64, a64, dst, src, typ, SLOPE, N_NODES)
    top = r0.argmax[tie_nodes]
    dst, src, typ = (np.concatenate([x, x[top]]) for x in (dst, src, typ))
    p = rng.permutation(dst.size)                                        # perm is not the identity
    dst, src, typ = dst[p], src[p], typ[p]
    c = Case()
    c.d, c.kind, c.lens, c.tie_nodes, c.chunk = d, kind, lens, tie_nodes, chunk
    c.dst, c.src, c.typ = dst, src, typ
    c.Z64, c.Rz64 = Z64, Rz64
    c.ref = attention_ref(P64, Q64, Rq64, a64, dst, src, typ, SLOPE, N_NODES)
    assert (c.ref.deg == lens).all()
    ei = torch.from_numpy(np.stack([dst, src])).cuda()
    c.graph = jg.RelGraph(ei, torch.from_numpy(typ).cuda(), N_NODES, N_REL)
    assert c.graph._chunk_dst == chunk and c.graph.by_dst.n_coop > 0 and c.graph.by_dst.n_splits_max > c.graph.by_dst.n_coop
    assert not torch.equal(c.graph.perm[: c.graph.E].cpu(), torch.arange(c.graph.E, dtype=torch.int32))
    c.a = a.cuda()
    if kind == "bf16":
        c.PQZ = ops.pad_table(PQZ, d, 3).to(torch.bfloat16).cuda()
        c.RR = ops.pad_table(RR, d, 2).to(torch.bfloat16).cuda()
        assert c.PQZ.shape[1] == 3 * ops.bf16_pad(d)
    else:
        c.PQZ, c.RR = PQZ.cuda(), RR.cuda()
    return c


def _export(c, **kw):
    from jmac_amd import ops
    return ops.rel_attn_edge_weights(*ops.pqz_views(c.PQZ), c.RR, c.a, c.graph, SLOPE, **kw)


def _check_against_float64(c, got, scaled, what):
    """Every assertion of the float64 comparison; returns the largest observed ratios to the two bounds."""
    ref, d, dst = c.ref, c.d, c.dst
    alpha = got.alpha.double().cpu().numpy()
    assert np.isfinite(alpha).all()
    Ai = np.zeros(N_NODES)
    np.maximum.at(Ai, dst, ref.A)
    sq = np.sqrt(ref.deg[dst]) if scaled else 1.0
    want = ref.alpha * sq
    b_alpha = (ref.alpha * (2 * d * U * Ai[dst] + 16 * U) + 2.0 ** -126) * sq
    r_alpha = float(np.max(np.abs(alpha - want) / b_alpha))
    r_logit = 0.0
    if got.logit is not None:
        logit = got.logit.double().cpu().numpy()
        assert np.isfinite(logit).all()
        r_logit = float(np.max(np.abs(logit - ref.logit) / (2 * d * U * ref.A + 16 * U)))
    print("%s: d=%d %s  max |err| / bound: alpha %.4f, logits %.4f" % (what, d, c.kind, r_alpha, r_logit))
    assert r_alpha <= 1.0 and r_logit <= 1.0, (r_alpha, r_logit)
    # destination sums
    sums = np.zeros(N_NODES)
    np.add.at(sums, dst, alpha)
    target = np.where(ref.deg > 0, np.sqrt(ref.deg) if scaled else 1.0, 0.0)
    assert np.max(np.abs(sums - target)) <= 1e-5, np.max(np.abs(sums - target))
    # a single in-edge weighs exactly 1 (sqrt(1) = 1 when scaled); duplicate edges weigh exactly the same
    single = ref.deg[dst] == 1
    assert single.any() and (alpha[single] == 1.0).all()
    key = np.stack([dst, c.src, c.typ], axis=1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    assert (cnt > 1).sum() >= len(c.tie_nodes)
    first = np.zeros(cnt.size, dtype=np.int64)
    first[inv[::-1]] = np.arange(dst.size)[::-1]                      # first edge of every (dst, src, type) group
    assert (alpha == alpha[first[inv]]).all()
    if got.entropy is not None:
        H = got.entropy.double().cpu().numpy()
        assert np.max(np.abs(H - ref.entropy) / (1 + np.log(np.maximum(ref.deg, 1)))) <= 1e-5
        assert (H[ref.deg == 0] == 0).all()
        am = got.argmax.cpu().numpy()
        assert am.dtype == np.int64 and (am[ref.deg == 0] == -1).all()
        checked = 0
        for i in np.flatnonzero(ref.deg > 0):
            e = np.flatnonzero(dst == i)
            top = ref.alpha[e].max()
            ties, rest = e[ref.alpha[e] == top], e[ref.alpha[e] != top]
            b_top = b_alpha[ties[0]] / (sq[ties[0]] if scaled else 1.0)
            if rest.size:
                nxt = rest[np.argmax(ref.alpha[rest])]
                if top - ref.alpha[nxt] <= b_top + b_alpha[nxt] / (sq[nxt] if scaled else 1.0):
                    continue                                           # the runner-up is within the bound: either may win
            assert am[i] == ties.min(), (i, am[i], ties)
            checked += 1
        assert checked >= N_NODES // 2
        for i in c.tie_nodes:                                          # the constructed ties: the lower edge id wins
            e = np.flatnonzero(dst == i)
            ties = e[ref.alpha[e] == ref.alpha[e].max()]
            assert ties.size >= 2 and am[i] == ties.min()
    return r_alpha, r_logit


# ---- 1. the reference's own softmax ---------------------------------------------------------------------------------------------
def _golden_layer(g, name):
    from jmac_amd import layer as jl
    d = int(g["d"])
    args = make_args(float(g["slope"]))
    if name == "dbpv1":
        lay = jl.RelationalAwareLayer(d, d, int(g["nr"]), rel_dim=d, act=torch.tanh, args=args)
    else:
        lay = jl.RelationAwareLayer(d, d, rel_dim=d, act=torch.tanh, args=args)
    lay.load_state_dict({k[len("param."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}, strict=False)
    if name == "tiny":
        lay.chunk = 4                                                  # split segments on a 16-edge graph
    return lay.cuda()


@pytest.mark.parametrize("name", ["tiny", "rand200", "d300", "ja_train", "noedge", "dbpv1"])
def test_layer_attention_matches_reference_golden(name):
    g, gold = load_golden("layer_" + name), load_golden("attention")
    lay = _golden_layer(g, name)
    X, R = t(g["X"], "cuda"), t(g["R"], "cuda")
    ei, et = t(g["edge_index"], "cuda"), t(g["edge_type"], "cuda")
    got = lay.attention(X, R, ei, et, stats=True)
    scaled = lay.attention(X, R, ei, et, scale_by_degree=True)
    assert got.logit is None and scaled.entropy is None and scaled.argmax is None
    assert_close(got.alpha, gold["alpha_" + name], 1e-4, 1e-6, "alpha")
    assert_close(scaled.alpha, gold["alpha_scaled_" + name], 1e-4, 1e-6, "alpha_scaled")
    n = int(g["n"])
    assert got.entropy.shape == (n,) and got.argmax.shape == (n,)
    if name == "noedge":
        assert got.alpha.shape == (0,) and scaled.alpha.shape == (0,)
        assert (got.entropy == 0).all() and (got.argmax == -1).all()
    else:
        deg = np.bincount(g["edge_index"][0], minlength=n)
        am = got.argmax.cpu().numpy()
        assert ((am >= 0) == (deg > 0)).all() and (g["edge_index"][0][am[am >= 0]] == np.flatnonzero(deg > 0)).all()


# ---- 2. / 3. float64 on the device's own tables -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 256, 300])
def test_float64_on_the_device_tables(d):
    c = case(d)
    _check_against_float64(c, _export(c, logits=True, stats=True), False, "plain")
    _check_against_float64(c, _export(c, scale_by_degree=True, stats=True), True, "scaled")


@pytest.mark.parametrize("d", [8, 300])
def test_wide_logits(d):
    """a_att x 40: the logits of one destination span more than 2 x 88, so exp overflows or every weight underflows unless the
    destination's maximum is subtracted first."""
    c = case(d, a_scale=40.0)
    assert c.ref.logit.max() - c.ref.logit.min() > 2 * 88
    hub = c.dst == int(np.flatnonzero(c.lens == HUB)[0])
    assert c.ref.logit[hub].max() - c.ref.logit[hub].min() > 88
    _check_against_float64(c, _export(c, logits=True, stats=True), False, "wide")
    _check_against_float64(c, _export(c, scale_by_degree=True), True, "wide scaled")


# ---- 4. bf16 tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [256, 300])
def test_bf16_tables_against_float64_on_the_rounded_tables(d):
    c = case(d, "bf16")
    assert c.PQZ.dtype == torch.bfloat16 and c.PQZ.shape[1] == 3 * (304 if d == 300 else 256)
    _check_against_float64(c, _export(c, logits=True, stats=True), False, "bf16")


def test_bf16_unpadded_rows_take_the_narrow_loads():
    """d = 300 without the pad (dh == d): rows are 8-byte aligned only."""
    c = case(300, "bf16")
    from jmac_amd import ops
    d = 300
    cut = lambda tab, parts: torch.cat([tab[:, k * 304:k * 304 + d] for k in range(parts)], dim=1).contiguous()
    PQZ, RR = cut(c.PQZ, 3), cut(c.RR, 2)
    got = ops.rel_attn_edge_weights(*ops.pqz_views(PQZ), RR, c.a, c.graph, SLOPE, logits=True, stats=True)
    _check_against_float64(c, got, False, "bf16 unpadded")


def test_bf16_layer_attention_works_under_grad_mode():
    g = load_golden("layer_d300")
    lay = _golden_layer(g, "d300")
    X, R = t(g["X"], "cuda").requires_grad_(True), t(g["R"], "cuda").requires_grad_(True)
    ei, et = t(g["edge_index"], "cuda"), t(g["edge_type"], "cuda")
    ref = lay.attention(X, R, ei, et)
    lay.table_dtype = torch.bfloat16
    assert torch.is_grad_enabled()
    with pytest.raises(RuntimeError):
        lay.pre_bn(X, R, ei, et)                                       # the training path refuses bf16 tables ...
    got = lay.attention(X, R, ei, et, logits=True)                     # ... the read-out does not
    assert torch.is_grad_enabled()
    assert not got.alpha.requires_grad and got.alpha.grad_fn is None and not ref.alpha.requires_grad
    # |d alpha| <= max |d s| / 2.  bf16 rounds the GEMM operands and the three table entries of every h_e[k] to 2^-9 relative:
    # entries of ~0.2 (X ~ 0.23, xavier weights, 300 terms) move by ~1e-3 each, s = sum of 300 such terms times a_k (|a|_2 ~ 1.4)
    # by ~2e-3 (random signs), ~1e-2 at the worst of 1100 edges: 2 % of the largest weight (1.0) bounds the difference, no closer
    assert_close(got.alpha, ref.alpha, 2e-2, 1e-6, "bf16 vs fp32 alpha")
    sums = torch.zeros(int(g["n"]), device="cuda", dtype=torch.float64).index_add_(0, ei[0], got.alpha.double())
    assert ((sums - (sums > 0.5).double()).abs() <= 1e-5).all()


# ---- 5. comp_op = 'mult' ------------------------------------------------------------------------------------------------------
def test_mult_attention():
    from jmac_amd import scatter as jscatter
    from jmac_amd.layer import RelationAwareLayer
    import torch.nn.functional as F
    n, nr, d, e = 90, 7, 32, 1500
    ei_np, et_np = random_graph(np.random.default_rng(3), n, nr, e, hub=600)
    torch.manual_seed(3)
    lay = RelationAwareLayer(d, d, rel_dim=d, act=torch.tanh, args=make_args(SLOPE, "mult")).cuda()
    X, R = torch.randn(n, d, device="cuda"), torch.randn(nr, d, device="cuda")
    ei, et = t(ei_np, "cuda"), t(et_np, "cuda")
    got = lay.attention(X, R, ei, et, logits=True, stats=True)
    with torch.no_grad():
        rel = lay.transform_relations(R)
        m = X[ei[1]] * rel.index_select(0, et)
        # the per-edge row table the layer builds (torch.mm is deterministic: the same bits)
        Q = torch.mm(torch.cat((m, X * rel[-1:]), dim=0), lay.w_att[d:])
        P = torch.mm(X, lay.w_att[:d])
        ref = attention_ref(P.double().cpu().numpy(), Q.double().cpu().numpy(), np.zeros((1, d)),
                            lay.a_att.reshape(-1).double().cpu().numpy(), ei_np[0], np.arange(e), np.zeros(e, dtype=np.int64), SLOPE, n)
        # the reference's own formulation on this library's torch_scatter-compatible kernels (_pre_bn_unfactorised)
        s = torch.mm(F.leaky_relu(torch.mm(torch.cat((X[ei[0]], m), dim=1), lay.w_att), SLOPE), lay.a_att)
        alpha2 = jscatter.scatter_softmax(s, ei[0], dim=0, dim_size=n).reshape(-1)
    Ai = np.zeros(n)
    np.maximum.at(Ai, ei_np[0], ref.A)
    alpha = got.alpha.double().cpu().numpy()
    ratio = float(np.max(np.abs(alpha - ref.alpha) / (ref.alpha * (2 * d * U * Ai[ei_np[0]] + 16 * U) + 2.0 ** -126)))
    print("mult: max |err| / bound %.4f" % ratio)
    assert ratio <= 1.0
    assert_close(got.alpha, alpha2, 1e-4, 1e-6, "alpha vs scatter_softmax")
    assert_close(got.logit, s.reshape(-1), 1e-4, 1e-6, "logit")
    assert np.max(np.abs(got.entropy.double().cpu().numpy() - ref.entropy) / (1 + np.log(np.maximum(ref.deg, 1)))) <= 1e-5


# ---- 6. it is the weight the layer uses ---------------------------------------------------------------------------------------
def test_exported_weights_reproduce_the_aggregation():
    from jmac_amd import ops
    c = case(300)
    w = _export(c, scale_by_degree=True).alpha.double().cpu().numpy()
    msg = w[:, None] * (c.Z64[c.src] - c.Rz64[c.typ])
    want = np.zeros((N_NODES, c.d))
    np.add.at(want, c.dst, msg)
    with torch.no_grad():
        out = ops.rel_attn_aggregate(c.PQZ, c.RR, c.a, c.graph, SLOPE, loop_rel=-1, out_scale=1.0)
    assert_close(out, want, 1e-4, 1e-6, "aggregate from the exported weights")


# ---- 7. reproducible ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,kind", [(300, "f32"), (300, "bf16")])
def test_bitwise_reproducible_and_slot_order(d, kind):
    c = case(d, kind)
    a1, a2 = _export(c, logits=True, stats=True), _export(c, logits=True, stats=True)
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    slot = _export(c, logits=True, stats=True, slot_order=True)
    perm = c.graph.perm[: c.graph.E].long()
    assert torch.equal(a1.alpha[perm], slot.alpha) and torch.equal(a1.logit[perm], slot.logit)
    assert torch.equal(a1.entropy, slot.entropy)
    some = slot.argmax >= 0
    assert torch.equal(a1.alpha[a1.argmax[some]], slot.alpha[slot.argmax[some]])     # the same largest weight, named by slot


# ---- 8. the model -------------------------------------------------------------------------------------------------------------
def _eval_inputs(model, block):
    """Inputs of the three layers in an eval-mode, op-by-op forward_base (on a model the test owns)."""
    seen, hooks = {}, []
    for name in ("conv1_alignment", "conv1_completion", "conv2_alignment"):
        hooks.append(getattr(model, name).register_forward_pre_hook(lambda mod, inp, name=name: seen.__setitem__(name, inp)))
    model.eval()
    model.fused_encoder = False
    with torch.no_grad():
        model.forward_base(*block)
    for h in hooks:
        h.remove()
    return seen


def test_model_attention_leaves_the_model_untouched():
    from test_gpu_align_manhattan import _blocks, mini
    model, kg1, kg2, _, graphs, args = mini()
    block = _blocks(kg1, kg2, graphs)[0]
    twin, probe = copy.deepcopy(model), copy.deepcopy(model)
    for m in (model, twin, probe):
        m.completion_dropout.p = 0.3                                   # a training forward consumes the device RNG
        m.train()
        torch.manual_seed(4)
        m.forward_base(*block)                                         # BatchNorm running statistics away from their initial values
        m.conv2_alignment.eval()                                       # a mixed pattern of training flags
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flags = [m.training for m in model.modules()]
    rng = torch.cuda.get_rng_state()
    res = model.attention(*block, stats=True, logits=True)
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    assert [m.training for m in model.modules()] == flags and model.fused_encoder is True
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    # equal to the layers' own attention on the inputs they see in an eval forward
    seen = _eval_inputs(probe, block)
    assert sorted(res) == sorted(seen) == ["conv1_alignment", "conv1_completion", "conv2_alignment"]
    E = block[0].shape[1]
    for name, inp in seen.items():
        want = getattr(probe, name).attention(*inp, stats=True, logits=True)
        assert res[name].alpha.shape == (E,)
        for x, y in zip(res[name], want):
            assert torch.equal(x, y), name
    # a training-mode forward afterwards: bit for bit that of the untouched twin under the same seed
    outs = []
    for m in (model, twin):
        torch.manual_seed(5)
        align, comp, rel = m.forward_base(*block)
        outs.append([align] + list(comp) + list(rel))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    sd_m, sd_t = model.state_dict(), twin.state_dict()
    assert all(torch.equal(sd_m[k], sd_t[k]) for k in sd_m)


@pytest.mark.parametrize("no_name,layers,want", [(True, 2, ["conv1_completion"]), (True, 1, [])])
def test_model_attention_returns_the_layers_that_ran(no_name, layers, want):
    """--no_name_info runs conv1_completion alone, and with num_gcn_layer = 1 no GNN layer at all (src/jmac_model.py:207-220).
    (With name information the reference's own shapes need num_gcn_layer = 2: uni_linear1_1 is [dim * num_gcn_layer, dim].)"""
    from jmac_amd.model import JMAC
    from test_gpu_align_manhattan import _blocks, mini
    model, kg1, kg2, _, graphs, args = mini()
    a2 = copy.copy(args)
    a2.no_name_info, a2.num_gcn_layer = no_name, layers
    torch.manual_seed(1)
    m2 = JMAC(a2, model.ent_info_att.numpy(), model.rel_init_att_completion.shape[0], model.ent_init_att_completion.shape[0]).cuda()
    block = _blocks(kg1, kg2, graphs)[0]
    res = m2.attention(*block)
    assert sorted(res) == want
    for v in res.values():
        assert v.alpha.shape == (block[0].shape[1],) and v.logit is None and v.entropy is None
    assert m2.training and m2.fused_encoder is True


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from jmac_amd import ops
    from jmac_amd._lib import JmacError
    from jmac_amd.layer import RelationAwareLayer
    lay = RelationAwareLayer(8, 8, 8, act=torch.tanh, args=make_args())
    x, r = torch.randn(5, 8), torch.randn(3, 8)
    ei, et = torch.tensor([[0, 1, 1], [1, 2, 0]]), torch.tensor([0, 1, 2])
    with pytest.raises(JmacError):
        lay.attention(x, r, ei, et)                                    # CPU tensors
    lay = lay.cuda()
    x, r, ei, et = x.cuda(), r.cuda(), ei.cuda(), et.cuda()
    assert lay.attention(x, r, ei, et).alpha.shape == (3,)
    assert lay.attention(x, r, ei, torch.tensor([0, 1, 3]).cuda()).alpha.shape == (3,)      # 3 = the loop relation's row
    with pytest.raises(IndexError):
        lay.attention(x, r, ei, torch.tensor([0, 1, 4]).cuda())
    with pytest.raises(ValueError):
        lay.attention(x, torch.randn(3, 12).cuda(), ei, et)
    with pytest.raises(ValueError):
        lay.attention(torch.randn(5, 12).cuda(), r, ei, et)
    c = case(8)
    with pytest.raises(JmacError):
        ops.rel_attn_edge_weights(*ops.pqz_views(c.PQZ.cpu()), c.RR, c.a, c.graph, SLOPE)
    with pytest.raises(ValueError):
        ops.rel_attn_edge_weights(*ops.pqz_views(c.PQZ[:-1]), c.RR, c.a, c.graph, SLOPE)        # a row short of the graph
    with pytest.raises(TypeError):
        ops.rel_attn_edge_weights(*ops.pqz_views(c.PQZ), c.RR.to(torch.bfloat16), c.a, c.graph, SLOPE)
