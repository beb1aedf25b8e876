"""GPU: the one-pass completion loss (jmac_triple_l1_margin_fwd_counts_f32 + jmac_margin_counts_scale_clear_f32) against the
two-pass form it replaces in losses._LayerLoss (jmac_triple_l1_fwd_f32 + jmac_triple_l1_margin_bwd_exact2_f32): the same scores,
the same integers in the count tables, the same gradients, all bit for bit -- and the ownership of the count tables, which are
no longer zero between a node's forward and its backward."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 25, 300), (1000, 25, 256), (250, 25, 300), (64, 5, 40), (7, 1, 12)]
MODES = ["random", "repeats", "ties", "mixed_runs", "one_relation"]


def _case(B, K, d, mode, seed=0):
    """(ent, rel, h, r, t, gamma, (eoff, en), (roff, rn)) on the device: tables with rows around the windows the ids are local to.
    repeats: few distinct tails, every tenth tail equal to its head; ties: small-integer tables and an integer margin, so that
    pos - neg == -gamma happens; mixed_runs: a third of the negatives carry another (h, r) than their run's positive;
    one_relation: a relation window of one row (every r flush on one address)."""
    gen = torch.Generator().manual_seed(1000 * seed + B + K + d)
    en, rn = max(5 * B, 16), (1 if mode == "one_relation" else 17)
    eoff, roff = 3, 2
    if mode == "ties":
        ent = torch.randint(-2, 3, (en + 7, d), generator=gen).float()
        rel = torch.randint(-2, 3, (rn + 4, d), generator=gen).float()
        gamma = 3.0
    else:
        ent = torch.randn(en + 7, d, generator=gen)
        rel = torch.randn(rn + 4, d, generator=gen)
        gamma = 0.2 * d
    T = B * (K + 1)
    bh = torch.randint(0, en, (B,), generator=gen)
    br = torch.randint(0, rn, (B,), generator=gen)
    h, r = bh.repeat(K + 1), br.repeat(K + 1)
    if mode in ("repeats", "ties"):
        t = torch.randint(0, min(en, 11), (T,), generator=gen)
        t[::10] = h[::10]
    else:
        t = torch.randint(0, en, (T,), generator=gen)
    if mode == "mixed_runs":
        odd = torch.arange(T) % 3 == 1
        odd[:B] = False
        h = torch.where(odd, torch.randint(0, en, (T,), generator=gen), h)
        r = torch.where(odd, torch.randint(0, rn, (T,), generator=gen), r)
    dev = torch.device("cuda")
    return (ent.to(dev), rel.to(dev), h.to(dev), r.to(dev), t.to(dev), torch.tensor([gamma], device=dev), (eoff, en), (roff, rn))


def _counts_float64(ent, rel, h, r, t, B, K, gamma, score):
    """The integers of the exact margin adjoint, restated: G_x sgn(ent[h] + rel[r] - ent[t]) with G = 2 w per triple (w = 1, 1/2
    or 0 from the fp32 scores; the positive takes the sum over its negatives, a negative minus its own), summed in float64."""
    diff = score[:B].unsqueeze(0) - score[B:].view(K, B)               # pos_b - neg_{b,k}, fp32 as the kernels form it
    g = gamma.reshape(())
    w2 = (diff > -g).double() * 2 + (diff == -g).double()
    G = torch.cat((w2.sum(0), -w2.reshape(-1)))
    c = G[:, None] * torch.sign((ent[h] + rel[r]) - ent[t]).double()
    cnt_e = torch.zeros(ent.shape, dtype=torch.float64, device=ent.device).index_add_(0, h, c).index_add_(0, t, -c)
    cnt_r = torch.zeros(rel.shape, dtype=torch.float64, device=ent.device).index_add_(0, r, c)
    return cnt_e, cnt_r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_one_pass_kernel_equals_the_two_pass_form(B, K, d, mode):
    from jmac_amd import losses
    from jmac_amd._lib import check, lib, ptr, stream
    ent, rel, h, r, t, gamma, (eoff, en), (roff, rn) = _case(B, K, d, mode)
    dev, T = ent.device, B * (K + 1)
    rows_e, rows_r = ent.shape[0], rel.shape[0]
    ew, rw = ent[eoff:eoff + en], rel[roff:roff + rn]
    want_score = losses.triple_l1_score(ew, rw, h, r, t, period=B)
    if mode == "ties" and B * K >= 1000:
        diff = want_score[:B].unsqueeze(0) - want_score[B:].view(K, B)
        assert int((diff == -gamma).sum()) > 0, "the case is meant to hold exact ties"
    score = torch.empty(T, dtype=torch.float32, device=dev)
    cnt_e = torch.zeros((rows_e, d), dtype=torch.float32, device=dev)
    cnt_r = torch.zeros((rows_r, d), dtype=torch.float32, device=dev)
    L = lib()
    check(L.jmac_triple_l1_margin_fwd_counts_f32(losses._wptr(ent, eoff), ent.stride(0), losses._wptr(rel, roff), rel.stride(0), ptr(h),
                                                 ptr(r), ptr(t), B, K, d, ptr(gamma), eoff, roff, ptr(cnt_e), ptr(cnt_r), ptr(score),
                                                 stream()), "fwd_counts")
    assert torch.equal(score, want_score)
    we, wr = _counts_float64(ew, rw, h, r, t, B, K, gamma, want_score)
    assert torch.equal(cnt_e[eoff:eoff + en].double(), we) and torch.equal(cnt_r[roff:roff + rn].double(), wr)
    assert float(cnt_e[:eoff].abs().max()) == 0 and float(cnt_e[eoff + en:].abs().max()) == 0      # nothing outside the windows
    assert float(cnt_r[:roff].abs().max()) == 0 and float(cnt_r[roff + rn:].abs().max()) == 0
    assert float(cnt_e.abs().max()) > 0
    gloss = torch.tensor([1.7], device=dev)
    dent = torch.full((rows_e, d), 7.0, device=dev)
    drel = torch.full((rows_r, d), 7.0, device=dev)
    check(L.jmac_margin_counts_scale_clear_f32(ptr(cnt_e), ptr(cnt_r), ptr(gloss), B, K, d, ptr(dent), rows_e, 0, ptr(drel), rows_r, 0,
                                               stream()), "scale_clear")
    assert float(cnt_e.abs().max()) == 0 and float(cnt_r.abs().max()) == 0
    # the two-pass adjoint on the same inputs (its own zeroed tables)
    dent2 = torch.full((rows_e, d), 9.0, device=dev)
    drel2 = torch.full((rows_r, d), 9.0, device=dev)
    check(L.jmac_triple_l1_margin_bwd_exact2_f32(losses._wptr(ent, eoff), ent.stride(0), losses._wptr(rel, roff), rel.stride(0), ptr(h),
                                                 ptr(r), ptr(t), B, K, d, ptr(want_score), ptr(gamma), ptr(gloss), eoff, roff, ptr(cnt_e),
                                                 ptr(cnt_r), ptr(dent2), rows_e, 0, ptr(drel2), rows_r, 0, stream()), "exact2")
    assert torch.equal(dent, dent2) and torch.equal(drel, drel2)
    assert float(cnt_e.abs().max()) == 0 and float(cnt_r.abs().max()) == 0


def _node_case(B, K, d, L, seed=0):
    ent, rel, h, r, t, gamma, ew, rw = _case(B, K, d, "repeats", seed)
    links = None
    if L:
        gen = torch.Generator().manual_seed(L)
        half = ew[1] // 2
        c = torch.randint(0, half, (L, 2), generator=gen).cuda()
        links = (c[:, 0].contiguous(), c[:, 1].contiguous(), (ew[0], half), (ew[0] + half, ew[1] - half))
    return ent, rel, h, r, t, gamma, ew, rw, links


def _node_grads(ent, rel, h, r, t, gamma, ew, rw, links, B, up=1.7, retain=False):
    from jmac_amd import losses
    eg, rg = ent.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    prev = torch.tensor([0.37], device=ent.device)
    loss = losses.completion_layer_loss(eg, rg, h, r, t, B, gamma, ew, rw, links=links, add_to=prev)
    first = torch.autograd.grad((loss * up).sum(), [eg, rg], retain_graph=retain)
    if not retain:
        return loss.detach(), first
    second = torch.autograd.grad((loss * up).sum(), [eg, rg])
    return loss.detach(), first, second


@pytest.mark.parametrize("B,K,d,L", [(1000, 25, 300, 0), (1000, 25, 300, 2264), (250, 25, 300, 300), (64, 5, 40, 0), (7, 1, 12, 5)])
def test_node_gradients_equal_the_two_pass_adjoint_and_a_second_backward(B, K, d, L):
    """completion_layer_loss with table windows, links and an upstream gradient of 1.7: the first backward (the forward's counts,
    scaled) equals the second one through the retained graph (jmac_triple_l1_margin_bwd_exact2_f32 from the saved scores: the
    two-pass form) bit for bit; the loss equals the separate ops' and no count table is left non-zero."""
    from jmac_amd import losses
    ent, rel, h, r, t, gamma, ew, rw, links = _node_case(B, K, d, L)
    loss, first, second = _node_grads(ent, rel, h, r, t, gamma, ew, rw, links, B, retain=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert float(first[0].abs().max()) > 0 and float(first[1].abs().max()) > 0
    with torch.no_grad():                              # no gradient asked for: the plain forward, the same loss
        prev = torch.tensor([0.37], device=ent.device)
        plain = losses.completion_layer_loss(ent, rel, h, r, t, B, gamma, ew, rw, links=links, add_to=prev)
    assert torch.equal(plain, loss)
    assert len(losses._CNT) > 0
    for c in losses._CNT.values():
        assert float(c[0].abs().max()) == 0.0 and float(c[1].abs().max()) == 0.0


def test_two_pending_nodes_of_one_shape_hold_tables_of_their_own():
    from jmac_amd import losses
    B, K, d = 250, 25, 300
    a = _node_case(B, K, d, 0, seed=1)
    b = _node_case(B, K, d, 0, seed=2)
    want_a = _node_grads(*a, B)[1]
    want_b = _node_grads(*b, B)[1]
    ea, ra = a[0].clone().requires_grad_(True), a[1].clone().requires_grad_(True)
    eb, rb = b[0].clone().requires_grad_(True), b[1].clone().requires_grad_(True)
    la = losses.completion_layer_loss(ea, ra, a[2], a[3], a[4], B, a[5], a[6], a[7])
    lb = losses.completion_layer_loss(eb, rb, b[2], b[3], b[4], B, b[5], b[6], b[7], add_to=la)      # chained like the step's two layers
    pa, pb = la.grad_fn.lease.pair, lb.grad_fn.lease.pair
    assert pa[0].data_ptr() != pb[0].data_ptr() and pa[1].data_ptr() != pb[1].data_ptr()
    (lb * 1.7).sum().backward()
    assert torch.equal(ea.grad, want_a[0]) and torch.equal(ra.grad, want_a[1])
    assert torch.equal(eb.grad, want_b[0]) and torch.equal(rb.grad, want_b[1])
    for c in losses._CNT.values():
        assert float(c[0].abs().max()) == 0.0 and float(c[1].abs().max()) == 0.0


def test_a_forward_without_backward_does_not_poison_the_next_step():
    from jmac_amd import losses
    B, K, d = 250, 25, 300
    case = _node_case(B, K, d, 300, seed=3)
    want = _node_grads(*case, B)[1]
    ent, rel, h, r, t, gamma, ew, rw, links = case
    gc.collect()
    n0 = len(losses._CNT_DIRTY)
    for how in ("discarded", "exception"):
        eg, rg = ent.clone().requires_grad_(True), rel.clone().requires_grad_(True)
        if how == "discarded":
            loss = losses.completion_layer_loss(eg, rg, h, r, t, B, gamma, ew, rw, links=links)
            del loss
        else:
            with pytest.raises(ZeroDivisionError):
                loss = losses.completion_layer_loss(eg, rg, h, r, t, B, gamma, ew, rw, links=links)
                loss = loss / 0                        # the step dies between forward and backward
                1 // 0
            del loss
        gc.collect()
        assert len(losses._CNT_DIRTY) == n0 + 1           # the counts nobody scaled are known as such ...
        assert all(float(c[0].abs().max()) == 0.0 and float(c[1].abs().max()) == 0.0 for c in losses._CNT.values())
        held = []                                      # ... and cleared before the next node counts into those tables: take pairs of
        while len(losses._CNT_DIRTY) > n0:             # this shape (the ones at rest go first) until that one is handed out
            held.append(losses._take_tables(ent.device, ent.shape[0], rel.shape[0], d))
            assert float(held[-1].pair[0].abs().max()) == 0.0 and float(held[-1].pair[1].abs().max()) == 0.0
            assert len(held) < 64
        got = _node_grads(*case, B)[1]                 # (every table of the shape is held: this node counts into a new pair)
        for lease in held:
            lease.release(True)
        again = _node_grads(*case, B)[1]               # on one of the released pairs, the once abandoned one among them
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_a_captured_step_replays_and_eager_losses_in_between_do_not_disturb_it():
    from jmac_amd import losses
    B, K, d = 250, 25, 300
    case = _node_case(B, K, d, 300, seed=4)
    ent, rel, h, r, t, gamma, ew, rw, links = case
    other = _node_case(B, K, d, 300, seed=5)
    loss_w, want = _node_grads(*case, B)
    want_other = _node_grads(*other, B)[1]
    eg, rg = ent.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    prev = torch.tensor([0.37], device=ent.device)
    static = [torch.zeros(1, device=ent.device), torch.zeros_like(ent), torch.zeros_like(rel)]

    def step():                                        # two nodes of one shape alive at once, like the step's two layers
        l0 = losses.completion_layer_loss(eg, rg, h, r, t, B, gamma, ew, rw, links=links, add_to=prev)
        l1 = losses.completion_layer_loss(eg, rg, h, r, t, B, gamma, ew, rw, links=links, add_to=l0)
        ge, gr = torch.autograd.grad((l1 * 1.7).sum(), [eg, rg])
        return l0, ge, gr

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l0, ge, gr = step()
        static[0].copy_(l0.reshape(1))
        static[1].copy_(ge)
        static[2].copy_(gr)
    baked = {c[0].data_ptr() for k, c in losses._CNT.items() if k[4]}
    assert len(baked) == 2                             # the capture took the two eager pairs at rest: no zero fill inside the graph
    pending = None
    for i in range(4):
        for x in static:
            x.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0].detach().reshape(1)) and torch.equal(static[0], loss_w.reshape(1))
        assert torch.equal(static[1], eager[1]) and torch.equal(static[2], eager[2])
        if i == 0:                                     # an eager loss between two replays, its backward run ...
            got = _node_grads(*other, B)[1]
            assert torch.equal(got[0], want_other[0]) and torch.equal(got[1], want_other[1])
        if i == 1:                                     # ... and one left PENDING across the next replay: on tables no graph knows
            e2 = other[0].clone().requires_grad_(True)
            pending = losses.completion_layer_loss(e2, other[1], other[2], other[3], other[4], B, other[5], other[6], other[7])
            assert pending.grad_fn.lease.pair[0].data_ptr() not in baked
        if i == 2:
            (g2,) = torch.autograd.grad((pending * 1.7).sum(), [e2])
            (w2,) = torch.autograd.grad((losses.completion_layer_loss(e2, other[1], other[2], other[3], other[4], B, other[5], other[6],
                                                                      other[7]) * 1.7).sum(), [e2])
            assert torch.equal(g2, w2)
    # gradients of the doubled term: twice one node's L1 part is not what is compared -- the eager step is; sanity against one node
    assert float((static[2] - 2 * want[1]).abs().max()) <= 1e-6 * float(want[1].abs().max())
    for c in losses._CNT.values():
        assert float(c[0].abs().max()) == 0.0 and float(c[1].abs().max()) == 0.0
