"""A numpy restatement of the bf16 screen of jmac_sim_topk_screened_f32 (jmac_amd/csrc/screen.hip) and the input
families its CPU and GPU tests share.

The screen's score sh(i, j) is the product of the operands rounded once to bf16 (round to nearest even, done here by bit
arithmetic), taken in float64.  The bound is e(i, j) = KAPPA (na_i + TAU) (nb_j + TAU) + ETA with na, nb upper bounds of the rows' l2
norms.  sample -> filter -> prune as the kernels do it: lower_i = the k-th largest sh - e over the first sample(N) columns; column j is
LISTED unless sh + e < lower_i; lower'_i = the k-th largest sh - e of the list; a listed column is KEPT (rescored exactly) unless
sh + e < lower'_i.  A row whose list is longer than CAP overflows (the kernel then recomputes the whole row)."""
import numpy as np

KAPPA, TAU, ETA = np.float32(0.008), np.float32(2.0 ** -110), np.float32(2.0 ** -110)
CAP, MIN_N, KMAX, DMAX = 1024, 8192, 64, 512


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32 (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def sample(n):
    ns = max(n // 8, 2048)
    return (ns + 127) // 128 * 128


def norm_up(x):
    """fp32 upper bounds of the rows' l2 norms (float64 sum, rounded up; at least the smallest normal for a non-zero row)."""
    root = np.sqrt((x.astype(np.float64) ** 2).sum(1)) * (1.0 + 2.0 ** -30)
    f = root.astype(np.float32)
    f = np.where(f.astype(np.float64) < root, np.nextafter(f, np.float32(np.inf)), f)
    return np.where((root > 0) & (root < 2.0 ** -126), np.float32(2.0 ** -126), f).astype(np.float32)


def bound(a, b):
    """e [L, N] float32, with the kernels' roundings: ka = KAPPA (na + TAU), nbt = nb + TAU, e = fma(ka, nbt, ETA)."""
    ka = (KAPPA * (norm_up(a) + TAU)).astype(np.float32)
    nbt = (norm_up(b) + TAU).astype(np.float32)
    return (ka.astype(np.float64)[:, None] * nbt.astype(np.float64)[None, :] + np.float64(ETA)).astype(np.float32)


def kth_largest(x, k):
    """per row; -inf where the row has fewer than k entries that are not -inf"""
    return -np.partition(-x, k - 1, axis=1)[:, k - 1]


def screen(a, b, k):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    sh = bf16_rne(a).astype(np.float64) @ bf16_rne(b).astype(np.float64).T
    e = bound(a, b).astype(np.float64)
    lo, hi = sh - e, sh + e
    lower = kth_largest(lo[:, :sample(b.shape[0])], k)
    listed = ~(hi < lower[:, None])
    lower2 = kth_largest(np.where(listed, lo, -np.inf), k)
    kept = listed & ~(hi < lower2[:, None])
    return dict(sh=sh, e=e, listed=listed, kept=kept, list_len=listed.sum(1), overflow=listed.sum(1) > CAP)


def topk64(a, b, k):
    """the float64 product's k best columns per row (ties -> lower index) [L, k]"""
    s = np.asarray(a, dtype=np.float64) @ np.asarray(b, dtype=np.float64).T
    return np.argsort(-s, axis=1, kind="stable")[:, :k]


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def families():
    """name -> dict(a, b, ks, overflow_rows): overflow_rows = the rows of a whose list MUST overflow (None: all of them)."""
    out = {}
    rng = np.random.default_rng(2024)
    # random unit rows, N not a tile multiple
    out["random_unit"] = dict(a=_unit(rng, 70, 20), b=_unit(rng, 8229, 20), ks=[1, 25, 64], overflow_rows=[])
    # two row tiles, the flagship row length
    out["two_row_tiles"] = dict(a=_unit(rng, 130, 300), b=_unit(rng, 9000, 300), ks=[25], overflow_rows=[])
    # near-duplicate columns: 5 base rows, each repeated 40 x with perturbations of 1e-5 (far below bf16's 2^-9 relative
    # resolution) at scattered positions, and 12 exact copies of base 0 (ties -> lower index); the queries are the bases and
    # perturbed bases, so the duplicates ARE their top-k: only the exact rescoring can order them
    d = 32
    b = _unit(rng, 8300, d)
    base = _unit(rng, 5, d)
    pos = rng.permutation(8300)[:5 * 40 + 12]
    for t in range(5):
        b[pos[t * 40:(t + 1) * 40]] = base[t] + np.float32(1e-5) * rng.standard_normal((40, d)).astype(np.float32)
    b[pos[200:]] = base[0]
    a = np.concatenate([base, base + np.float32(1e-3) * rng.standard_normal((5, d)).astype(np.float32), _unit(rng, 20, d)])
    out["near_duplicates"] = dict(a=a.astype(np.float32), b=b, ks=[25], overflow_rows=[])
    # sub-bound gaps: a[i] = s_i e_0, so the scores are s_i b[:, 0] whatever the contraction order; 25 columns with first coordinate
    # 0.9 + 2e-5 t, the next 200 at 0.9 - 2e-5 (t + 1): all 225 within 0.005 s_i of each other against e ~ 0.008 s_i; every other
    # column's first coordinate is <= 0
    d = 16
    b = _unit(rng, 8200, d)
    b[:, 0] = -np.abs(b[:, 0]) * np.float32(0.5)
    cols = rng.permutation(8200)[:225]
    first = np.concatenate([0.9 + 2e-5 * np.arange(25), 0.9 - 2e-5 * (np.arange(200) + 1)]).astype(np.float32)
    rest = b[cols, 1:]
    b[cols, 1:] = rest / np.linalg.norm(rest, axis=1, keepdims=True) * np.sqrt(1 - first * first)[:, None]
    b[cols, 0] = first
    a = np.zeros((8, d), dtype=np.float32)
    a[:, 0] = np.linspace(0.5, 1.0, 8, dtype=np.float32)
    out["sub_bound_gaps"] = dict(a=a, b=b.astype(np.float32), ks=[25], overflow_rows=[])
    # un-normalised rows: norms 1e-3 .. 1e3 on both sides, rows scaled by 1e-30 on both sides, zero rows on both sides.  A zero row
    # of A scores 0 against every column: all N tie, any of them may be among the k best, so its list MUST overflow (rows 0, 1)
    d = 24
    a = _unit(rng, 48, d) * (10.0 ** rng.uniform(-3, 3, (48, 1))).astype(np.float32)
    b = _unit(rng, 8200, d) * (10.0 ** rng.uniform(-3, 3, (8200, 1))).astype(np.float32)
    a[0:2] = 0
    a[2:8] *= np.float32(1e-30)
    b[rng.permutation(8200)[:300]] *= np.float32(1e-30)
    b[rng.permutation(8200)[:5]] = 0
    out["unnormalised"] = dict(a=a.astype(np.float32), b=b.astype(np.float32), ks=[10], overflow_rows=[0, 1])
    # overflow: B is one row repeated, every row's N scores tie
    out["overflow"] = dict(a=_unit(rng, 6, 16), b=np.repeat(_unit(rng, 1, 16), 8192 + 37, axis=0), ks=[25], overflow_rows=None)
    return out
