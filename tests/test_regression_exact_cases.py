"""The generators and references of regression_exact_cases.py, checked on the CPU: the "exact" inputs really are exact
(two float64 summation orders and the int64 reference agree bit for bit, the values survive float32), the restated launch
plan gives the splits the GPU tests count on, and the high-precision sums agree between longdouble and mpmath."""
import numpy as np
import pytest

import regression_exact_cases as cases
import regression_oracle as orc


def block_in_order(w, y, order):
    """[G | c | s | n] in float64, the rows added one after the other in ``order``: every partial sum is rounded."""
    D = w.shape[1]
    G, c, s = np.zeros((D, D)), np.zeros(D), 0.0
    for n in order:
        G += np.outer(w[n], w[n])
        c += w[n] * y[n]
        s += y[n] * y[n]
    return np.concatenate([G.ravel(), c, [s, float(len(y))]])


def block_blas(w, y):
    return np.concatenate([(w.T @ w).ravel(), w.T @ y, [y @ y, float(len(y))]])


def assert_exact(w, y, ref):
    n = len(y)
    fwd = block_in_order(w, y, range(n))
    rev = block_in_order(w, y, np.random.default_rng(1).permutation(n))
    assert np.array_equal(fwd, rev) and np.array_equal(fwd, ref) and np.array_equal(block_blas(w, y), ref)


@pytest.mark.parametrize("D,N", ((1, 17), (33, 1500), (97, 700)))
def test_matrix_rows_are_exact(D, N):
    a, b, e = cases.matrix_case(D, N, 10 + D)
    assert a.min() >= -7 and a.max() <= 7 and (a.size < 1000 or (a.min(), a.max()) == (-7, 7))
    assert e.min() >= -20 and e.max() <= 20 and (D < 41 or (e.min(), e.max()) == (-20, 20))
    x, y = cases.scaled(a, e, np.float64), cases.scaled(b, cases.E_Y, np.float64)
    x32, y32 = cases.scaled(a, e, np.float32), cases.scaled(b, cases.E_Y, np.float32)
    assert x32.dtype == np.float32 and y32.dtype == np.float32
    assert np.array_equal(x32.astype(np.float64), x) and np.array_equal(y32.astype(np.float64), y)
    assert np.array_equal(x, a * 2.0 ** e) and np.array_equal(y, b * 2.0 ** cases.E_Y)
    assert_exact(x, y, cases.stats_reference(a, b, e, cases.E_Y))


def test_largest_sums_stay_below_2_53():
    """The worst case of the grid, every term at its largest: 49 N at N = 73729, and q at D = 256."""
    assert max(n for *_rest, n in cases.stats_grid()) == 73729 and 49 * 73729 < 2 ** 53
    assert 256 * (49 * 256) ** 2 < 2 ** 53
    a, b = np.full((73729, 2), 7), np.full(73729, -7)
    ref = cases.stats_reference(a, b, np.array([20, -20]), cases.E_Y)
    assert ref[0] == 49 * 73729 * 2.0 ** 40 and ref[1] == 49 * 73729 and ref[4] == -49 * 73729 * 2.0 ** (20 + cases.E_Y)


@pytest.mark.parametrize("p,padding", ((0, None), (5, None), (5, "zeros"), (64, "zeros"), (70, None)))
def test_window_rows_are_exact(p, padding):
    ints = cases.series_case(p + 300, 20 + p)
    x = cases.scaled(ints, cases.E_SERIES, np.float64)
    assert np.array_equal(cases.scaled(ints, cases.E_SERIES, np.float32).astype(np.float64), x)
    w, y = orc.lag_matrix(x, p, padding)
    assert w.shape == (300 + (p if padding == "zeros" else 0), p + 1)
    assert_exact(w, y, cases.window_reference(ints, p, padding))


@pytest.mark.parametrize("D", (1, 33, 256))
def test_predict_case_is_exact(D):
    Li, xi, mui = cases.predict_case(D, 40, 30 + D)
    assert np.array_equal(Li, np.tril(Li)) and np.all(np.diag(Li) > 0) and np.abs(Li).max() <= 7
    linv, x, mu = Li / 8.0, xi.astype(np.float64), mui.astype(np.float64)
    assert np.array_equal(linv * 8.0, Li) and np.array_equal(xi.astype(np.float32).astype(np.float64), x)
    m, q = cases.predict_reference(Li, xi, mui)
    perm = np.random.default_rng(2).permutation(D)
    for cols in (np.arange(D), perm):                 # the contraction in two orders, term by term
        z, mm = np.zeros((40, D)), np.zeros(40)
        for f in cols:
            z += np.outer(x[:, f], linv[:, f])
            mm += x[:, f] * mu[f]
        qq = np.zeros(40)
        for t in cols:
            qq += z[:, t] * z[:, t]
        assert np.array_equal(mm, m) and np.array_equal(qq, q)
    assert np.array_equal(np.sum((x @ linv.T) ** 2, axis=1), q)


def test_launch_plan_of_the_grid():
    """gram_max_splits per tile count as csrc/regvb_kernels.h states it, and every case of the grid really is cut into
    splits of three and of four batches with the last split of LASTS."""
    assert [cases.gram_max_splits(T) for T in range(2, 17, 2)] == [1536, 1536, 1024, 768, 256, 256, 256, 256]
    assert [cases.rows_for(T, 48, 1) for T in (2, 6, 8, 10)] == [49153, 32785, 24577, 8209]
    seen = set()
    for D, batches, last, N in cases.stats_grid():
        T = cases.even_tiles(D)
        rps, S, cut = cases.split_plan(N, T)
        assert (rps, cut) == (16 * batches, last) and S <= cases.gram_max_splits(T) and (S - 1) * rps + cut == N
        assert 16 * (batches - 1) * cases.gram_max_splits(T) < N <= 73729
        seen.add((T, batches, last))
    assert {(T, b) for T, b, _ in seen} == {(T, b) for T in range(2, 17, 2) for b in (3, 4)}
    for batches in (3, 4):
        assert {last for T, b, last in seen if b == batches and T > 4} == set(cases.LASTS)
    assert {cases.even_tiles(D) for D in cases.MIXED_DS} == set(range(2, 17, 2))


def test_wide_sums_longdouble_and_mpmath_agree(monkeypatch):
    """hp_matmul on a badly scaled case: the mpmath route (forced) agrees with longdouble to longdouble's own rounding, and
    both are far closer to each other than float64 is to either."""
    x, y = cases.scaled_rows(7, 50, 3)
    assert cases.WIDE, "numpy.longdouble is binary64 here: the GPU tests fall back to mpmath, which is slow"
    ref, mag = cases.hp_stats(x, y)
    monkeypatch.setattr(cases, "WIDE", False)
    ref_mp, mag_mp = cases.hp_stats(x, y)
    assert ref_mp.dtype == object and np.array_equal(mag, mag_mp)
    hi = ref.astype(np.float64)                       # (a longdouble as two float64: mpmath takes those exactly)
    lo = (ref - hi).astype(np.float64)
    d = np.array([abs(float(a - float(h) - float(t))) for a, h, t in zip(ref_mp, hi, lo)])
    assert np.all(d <= 50 * 2.0 ** -64 * mag / (1.0 - 100 * cases.U))
    f64 = np.concatenate([(x.T @ x).ravel(), x.T @ y, [y @ y]])
    assert np.all(cases.err(f64, ref_mp) <= cases.stats_bound(mag, 50, 2))
    monkeypatch.undo()
    assert np.all(cases.err(f64, ref) <= cases.stats_bound(mag, 50, 2))


def test_predict_bound_holds_for_float64_numpy():
    """The bounds of hp_predict are wide enough for a plain float64 evaluation of the same factor and far tighter than the
    factorisation's conditioning: about 1e-13 relative on p_lambdas where solve() is off by 1e-9."""
    from bayesml_amd._normalgamma import inverse_factor
    D, N = 49, 30
    lam, mu, s = cases.conditioned_factor(D, 5)
    assert 1e7 < np.linalg.cond(lam) < 1e9
    linv = inverse_factor(lam)
    x = cases.conditioned_rows(D, N, 6, s)
    m, pl, bm, bl = cases.hp_predict(x, mu, linv, 1.75)
    z = x @ linv.T
    q = np.sum(z * z, axis=1)
    assert np.all(cases.err(x @ mu, m) <= bm)
    assert np.all(cases.err(1.75 / (1.0 + q), pl) <= bl * np.asarray(pl, dtype=np.float64))
    assert bl.max() < 1e-12
