"""CPU: the bf16 screen's scheme restated in numpy (screen_ref.py) holds what jmac_sim_topk_screened_f32's exactness rests on, on
every input family its GPU test runs:
  * the bound: |sh - s| <= e = KAPPA (na + TAU) (nb + TAU) + ETA, against a float32 matmul of the unrounded operands AND against float64;
  * the pruned candidate set contains the float64 product's top-k;
  * outside the rows that must overflow (the overflow family; the zero rows of A, whose N scores all tie) the list stays within
    the kernel's capacity -- so the GPU test cannot pass by recomputing everywhere -- and those rows do overflow.
Also the constant: KAPPA covers 2u + u^2 + 2 (d + 2) 2^-23 (1 + u)^2 at d = 512 (accumulation counted at one ulp per operation, twice
the round-to-nearest figure of the issue, for a matrix core that truncates)."""
import numpy as np
import pytest

import screen_ref as R

FAMILIES = R.families()
CASES = [(name, k) for name, f in FAMILIES.items() for k in f["ks"]]


def test_bf16_rounding_is_nearest_even():
    import torch
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 2.0 ** -133, 3.0e38 / 2], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(R.bf16_rne(x).view(np.uint32), want.view(np.uint32))
    assert R.bf16_rne(np.float32(1.00390625)) == 1.0 and R.bf16_rne(np.float32(1.01171875)) == np.float32(1.015625)   # ties -> even


def test_kappa_covers_the_stated_terms():
    u = 2.0 ** -8
    for d in (4, 300, R.DMAX):
        assert float(R.KAPPA) * (1 - 2.0 ** -10) >= 2 * u + u * u + 2 * (d + 2) * 2.0 ** -23 * (1 + u) ** 2, d


@pytest.mark.parametrize("name", list(FAMILIES))
def test_bound_against_float32_and_float64(name):
    f = FAMILIES[name]
    a, b = f["a"], f["b"]
    sc = R.screen(a, b, f["ks"][0])
    s32 = (a @ b.T).astype(np.float64)
    s64 = a.astype(np.float64) @ b.astype(np.float64).T
    for ref, what in ((s32, "float32 matmul"), (s64, "float64")):
        excess = np.abs(sc["sh"] - ref) - sc["e"]
        i, j = np.unravel_index(np.argmax(excess), excess.shape)
        print("%s, %s: max(|sh - s| - e) = %.3e at (%d, %d), e there %.3e" % (name, what, excess[i, j], i, j, sc["e"][i, j]))
        assert (excess <= 0).all(), (name, what)


@pytest.mark.parametrize("name,k", CASES)
def test_pruned_set_contains_float64_topk_and_lists_fit(name, k):
    f = FAMILIES[name]
    a, b = f["a"], f["b"]
    sc = R.screen(a, b, k)
    top = R.topk64(a, b, k)
    assert np.take_along_axis(sc["kept"], top, axis=1).all()
    assert (sc["kept"].sum(1) >= k).all()
    must = np.zeros(len(a), dtype=bool)
    must[f["overflow_rows"] if f["overflow_rows"] is not None else slice(None)] = True
    print("%s k=%d: list length mean %.1f max %d, kept mean %.1f max %d (rows that fit)"
          % (name, k, sc["list_len"][~must].mean() if (~must).any() else 0, sc["list_len"][~must].max() if (~must).any() else 0,
             sc["kept"][~must].sum(1).mean() if (~must).any() else 0, sc["kept"][~must].sum(1).max() if (~must).any() else 0))
    assert (sc["list_len"][~must] <= R.CAP).all()
    assert (sc["list_len"][must] > R.CAP).all()


def test_sample_and_shapes():
    assert R.sample(8192) == 2048 and R.sample(8229) == 2048 and R.sample(30000) == 3840 and R.sample(13996) == 2048
    for f in FAMILIES.values():
        assert f["b"].shape[0] >= R.MIN_N and max(f["ks"]) <= R.KMAX and f["a"].shape[1] % 4 == 0 and f["a"].shape[1] <= R.DMAX
