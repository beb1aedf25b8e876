"""Float64 restatement, in plain torch, of what scoring.sim_lse / scoring.sinkhorn_potentials compute: log-domain Sinkhorn with
uniform marginals on S = a b^T,

    log P[i, j] = scale S[i, j] + f[i] + g[j],   from f = g = 0:   f <- -log n1 - LSE_j(scale S + g),  g <- -log n2 - LSE_i(scale S + f)

on the fp32 inputs (the products and everything behind them in float64), the same recursion in torch fp32 as a yardstick of what
an fp32 evaluation of this map can reach, and the seeded "hub" pair the tests run on.  The reference project has no Sinkhorn:
nothing here is taken from it, and nothing here shares code with the library."""
import math

import torch

F = torch.nn.functional


def lse(a, b, scale, col_add=None, row_add=None, dtype=torch.float64):
    """(row [n1], col [n2]): row[i] = -log sum_j exp(scale S[i, j] + col_add[j]), col[j] = -log sum_i exp(scale S[i, j] + row_add[i])."""
    S = scale * (a.to(dtype) @ b.to(dtype).t())
    zr = S if col_add is None else S + col_add.to(dtype).view(1, -1)
    zc = S if row_add is None else S + row_add.to(dtype).view(-1, 1)
    return -torch.logsumexp(zr, 1), -torch.logsumexp(zc, 0)


def lse_sliced(a, b, scale, col_add, row_add, rows=1024):
    """``lse`` in float64 without the whole matrix: row slices, the column sums combined by logaddexp."""
    b64 = b.double()
    row, col = [], torch.full((b.shape[0],), -math.inf, dtype=torch.float64)
    for lo in range(0, a.shape[0], rows):
        S = scale * (a[lo:lo + rows].double() @ b64.t())
        row.append(-torch.logsumexp(S + col_add.double().view(1, -1), 1))
        col = torch.logaddexp(col, torch.logsumexp(S + row_add[lo:lo + rows].double().view(-1, 1), 0))
    return torch.cat(row), -col


def potentials(a, b, scale, iters, tol=None, dtype=torch.float64):
    """(f, g, residuals): residuals[t] = max_i |f_new - f_old| of iteration t's row step; ``tol`` stops after the first iteration
    whose residual is <= tol (len(residuals) = the iterations done)."""
    S = scale * (a.to(dtype) @ b.to(dtype).t())
    n1, n2 = S.shape
    f, g = torch.zeros(n1, dtype=dtype), torch.zeros(n2, dtype=dtype)
    residuals = []
    for _ in range(iters):
        fn = -math.log(n1) - torch.logsumexp(S + g.view(1, -1), 1)
        residuals.append(float((fn - f).abs().max()))
        f = fn
        g = -math.log(n2) - torch.logsumexp(S + f.view(-1, 1), 0)
        if tol is not None and residuals[-1] <= tol:
            break
    return f, g, residuals


def potentials_fp32(a, b, scale, iters):
    """The same recursion evaluated in torch fp32 (product included)."""
    f, g, _ = potentials(a, b, scale, iters, dtype=torch.float32)
    return f, g


def log_plan(a, b, scale, f, g):
    return scale * (a.double() @ b.double().t()) + f.double().view(-1, 1) + g.double().view(1, -1)


def terms(f, g, scale):
    return -(2.0 / scale) * f, -(2.0 / scale) * g


def rescored(a, b, r1, r2):
    """c = 2 S - r1 - r2 in float64."""
    return 2.0 * (a.double() @ b.double().t()) - r1.double().view(-1, 1) - r2.double().view(1, -1)


def ranks(c, gold):
    """1-based rank of column gold[i] in row i (descending, ties -> lower index first)."""
    g = c.gather(1, gold.view(-1, 1))
    ar = torch.arange(c.shape[1]).view(1, -1)
    return ((c > g) | ((c == g) & (ar < gold.view(-1, 1)))).sum(1) + 1


def decided(c, gold, gap=1e-4):
    """The rows on which nothing but the gold itself comes within ``gap`` of the gold value: their rank survives an error < gap / 2."""
    return ((c - c.gather(1, gold.view(-1, 1))).abs() < gap).sum(1) == 1


def hub_pair(n1, n2, d, noise=1.0, seed=0):
    """(e1 [n1, d], e2 [n2, d], gold [min(n1, n2)]) fp32 unit rows: a shared base with a common offset, independent noise on both
    sides, and on 30 % of the rows of e2 one of 8 hub directions -- rows that are everybody's near neighbour, the case CSLS and
    Sinkhorn exist for.  Row i of e1 belongs to row i of e2."""
    gen = torch.Generator().manual_seed(seed)
    n = max(n1, n2)
    base = torch.randn(n, d, generator=gen) + 0.5 * torch.randn(1, d, generator=gen)
    hub = torch.randn(8, d, generator=gen)
    e1 = F.normalize(base[:n1] + noise * torch.randn(n1, d, generator=gen), dim=1)
    pick = hub[torch.randint(8, (n2,), generator=gen)]
    on = (torch.rand(n2, 1, generator=gen) < 0.3).float()
    e2 = F.normalize(base[:n2] + noise * torch.randn(n2, d, generator=gen) + 0.6 * pick * on, dim=1)
    return e1, e2, torch.arange(min(n1, n2))
