"""Inputs and references for the edge tests of the regression data passes, csrc/regvb_kernels.h (TEST INFRASTRUCTURE; needs
no GPU).  Everything is a seeded recipe; nothing is stored.

A. Exact inputs.  Rows x[n, j] = a[n, j] 2^e_j with integers a in -7 .. 7 and exponents e_j cycling over -20 .. 20, targets
   y[n] = b[n] 2^E_Y with integers b in -7 .. 7.  Every product a_ni a_nj 2^(e_i + e_j) is an integer of at most 49 times
   one power of two per entry, and so is every partial sum, in whatever order it is taken: at most 49 N <= 49 * 73729 < 2^53
   for the sizes used here.  G, c and s are therefore exactly representable in binary64 and a correct kernel returns them
   bit for bit; the inputs are exact in binary32 as well.  The reference is an int64 product scaled by ldexp.
   The same holds for a series of integers times one power of two under the lag window (the constant column has exponent 0)
   and for the predictive read-out of a lower triangular factor with entries (integers in -7 .. 7) / 8, positive diagonal,
   on integer x and mu: z = L x is an integer / 8, q = |z|^2 an integer / 64 below 256 (49 * 256)^2 < 2^53, m an integer.

B. Badly scaled real inputs with a derived bound per entry.  Columns scaled log-spaced over twelve decades, every other one
   offset by 1e3 of its scale, targets offset by 1e3.  The reference holds the sums of the binary64 products in
   numpy.longdouble (mpmath where that is no wider than binary64).  With u = 2^-53 the kernel's entry differs from it by at
   most (rps + S + 4) u sum_n |w_ni w_nj|: a slab accumulates its at most rps rows with one rounding each (fused multiply-add,
   the products exact), gram_reduce_kernel adds the S slabs with S - 1 roundings, and four more units cover the reference's
   own N 2^-64 (two units at N = 4097), the rounding of the exact sum to binary64 and second-order terms.  For the
   predictive read-out, with gamma_k = k u / (1 - k u) and e_t = gamma_D sum_f |L_tf x_f| the error of z_t (a contraction
   of D terms, the padded ones exactly zero):  |m - ref| <= gamma_(D+2) sum_f |x_f mu_f|,
   |q - ref| <= sum_t (2 |z_t| e_t + e_t^2) + gamma_(D+2) q, and p_lambdas moves relatively by at most
   |dq| / (1 + q) + 2 u (the sum 1 + q and the division).
"""
from __future__ import annotations

import numpy as np

import regression_oracle as orc

LD = np.longdouble
WIDE = bool(np.finfo(LD).eps < 2e-19)       # the 64-bit significand of x87; otherwise mpmath stands in
U = 2.0 ** -53                              # unit roundoff of binary64
E_Y = -9                                    # exponent of the exact targets
E_SERIES = -5                               # exponent of the exact series
LASTS = (1, 15, 16, 17, 33)                 # rows of the cut last split


# ---- the launch plan of csrc/regvb_stats.hip, restated -------------------------------------------------------------------
def even_tiles(D):
    return 2 * ((D + 31) // 32)


def gram_max_splits(T):
    return 256 if T > 8 else min(256 * (12 // (T // 2)), 1536)


def gram_slab_len(T):
    return (T * (T + 1) // 2) * 256 + 16 * T + 16


def split_plan(n_rows, T):
    """(rows per split, splits, rows of the last split): launch_gram's three lines of integer arithmetic."""
    rps = -(-n_rows // gram_max_splits(T))
    rps = -(-rps // 16) * 16
    S = -(-n_rows // rps)
    return rps, S, n_rows - (S - 1) * rps


def rows_for(T, rps, last):
    """The smallest number of rows that launch_gram cuts into splits of ``rps`` rows with ``last`` rows in the last one."""
    lo = (rps - 16) * gram_max_splits(T) + 1
    return lo + (last - lo) % rps


STATS_DS = (1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256)      # both ends of every tile count
MIXED_DS = (32, 64, 96, 128, 160, 192, 224, 256)                                         # x / y dtypes mixed: one per T


def stats_grid():
    """[(D, batches per split, rows of the last split, N)]: three and four batches per split at every D, the last split
    walking through LASTS.  Up to T = 4 four batches need N > 48 * 1536, and the exactness argument (and 38 MB of rows)
    stop at 73729: there the last split holds one row."""
    grid = []
    for k, D in enumerate(STATS_DS):
        T = even_tiles(D)
        grid.append((D, 3, LASTS[k % 5], rows_for(T, 48, LASTS[k % 5])))
        last = 1 if T <= 4 else LASTS[(k + 2) % 5]
        grid.append((D, 4, last, rows_for(T, 64, last)))
    return grid


# ---- A: exact inputs -------------------------------------------------------------------------------------------------------
def exponents(D):
    return -20 + np.arange(D) % 41


def scaled(ints, e, dtype):
    """ints * 2^e in ``dtype`` (exact in float32 and float64 for |ints| <= 7 and |e| <= 20)."""
    return np.ldexp(np.asarray(ints).astype(dtype), e)


def matrix_case(D, N, seed):
    """(a [N, D], b [N], e [D]) of the exact rows scaled(a, e, .) and targets scaled(b, E_Y, .)."""
    rng = np.random.default_rng(seed)
    return rng.integers(-7, 8, (N, D)), rng.integers(-7, 8, N), exponents(D)


def int_matmul(a, b):
    """a @ b in int64.  (torch's: NumPy's integer matmul has no blocked kernel and takes 8 s at N = 12289, D = 256)"""
    import torch
    a, b = np.ascontiguousarray(a, dtype=np.int64), np.ascontiguousarray(b, dtype=np.int64)
    return (torch.from_numpy(a) @ torch.from_numpy(b)).numpy()


def stats_reference(a, b, e, e_y):
    """[G | c | s | n] of the rows a 2^e and targets b 2^e_y, from int64 sums."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    G, c, s = int_matmul(a.T, a), a.T @ b, int(b @ b)
    assert max(np.abs(G).max(), np.abs(c).max(), s) < 2 ** 53
    e = np.asarray(e)
    return np.concatenate([np.ldexp(G.astype(np.float64), e[:, None] + e[None, :]).ravel(), np.ldexp(c.astype(np.float64), e + e_y),
                           [np.ldexp(float(s), 2 * e_y), float(a.shape[0])]])


def series_case(length, seed):
    """Integers in -7 .. 7: the exact series is scaled(., E_SERIES, .)."""
    return np.random.default_rng(seed).integers(-7, 8, length)


def window_reference(ints, p, padding, rows=slice(None)):
    """The statistics of the lag windows of scaled(ints, E_SERIES, .), or of the windows ``rows`` among them:
    regression_oracle.lag_matrix on the integers, in int64, the constant column with exponent 0."""
    w, y = orc.lag_matrix(ints, p, padding)
    wi, yi = w[rows].astype(np.int64), y[rows].astype(np.int64)
    w, y = w[rows], y[rows]
    assert np.array_equal(wi, w) and np.array_equal(yi, y)
    return stats_reference(wi, yi, np.concatenate([[0], np.full(p, E_SERIES)]), E_SERIES)


def predict_case(D, N, seed):
    """(Li [D, D], xi [N, D], mui [D]) integers: the factor is Li / 8, lower triangular with a positive diagonal."""
    rng = np.random.default_rng(seed)
    Li = np.tril(rng.integers(-7, 8, (D, D)), -1) + np.diag(rng.integers(1, 8, D))
    return Li, rng.integers(-7, 8, (N, D)), rng.integers(-7, 8, D)


def predict_reference(Li, xi, mui):
    """(m, q) of the exact case, from int64: m = x . mu, q = |Li x|^2 / 64."""
    z8 = int_matmul(xi, Li.T)
    q64 = (z8 * z8).sum(axis=1)
    assert q64.max() < 2 ** 53
    return (xi @ mui).astype(np.float64), np.ldexp(q64.astype(np.float64), -6)


# ---- B: badly scaled inputs, high-precision sums and the bounds --------------------------------------------------------------
def column_scales(D, decades):
    return 10.0 ** np.linspace(-decades, decades, D) if D > 1 else np.ones(1)


def scaled_rows(D, N, seed):
    """(x [N, D], y [N]) float64: column scales from 1e-6 to 1e6, every other column offset by 1e3 scales, y offset by 1e3."""
    rng = np.random.default_rng(seed)
    x = column_scales(D, 6) * (rng.standard_normal((N, D)) + 1e3 * (np.arange(D) % 2))
    return x, 1e3 + rng.standard_normal(N)


def hp(a):
    """The binary64 values of ``a`` in the wide type."""
    a = np.asarray(a, dtype=np.float64)
    if WIDE:
        return a.astype(LD)
    import mpmath
    mpmath.mp.dps = 50
    return np.vectorize(mpmath.mpf, otypes=[object])(a)


def hp_matmul(a, b):
    """a @ b of binary64 matrices with the products and sums in the wide type (longdouble: one plain loop per entry, in
    order; mpmath at 50 digits: the products exact, slow, only where longdouble is binary64)."""
    if WIDE:
        return np.einsum("ik,kj->ij", hp(a), hp(b))
    import mpmath
    mpmath.mp.dps = 50
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[1]), dtype=object)
    cols = [[float(v) for v in b[:, j]] for j in range(b.shape[1])]
    for i in range(a.shape[0]):
        row = [float(v) for v in a[i]]
        for j in range(b.shape[1]):
            out[i, j] = mpmath.fdot(row, cols[j])
    return out


def err(dev, ref):
    """|dev - ref| as float64, the difference taken in the wide type."""
    d = np.abs(hp(dev) - ref)
    return np.asarray(d, dtype=np.float64)


def hp_stats(w, y):
    """(ref, mag): [G | c | s] of the binary64 rows in the wide type, and the sums of the products' absolute values (a
    float64 product, low by at most a relative N u: deflated by 2 N u so that the bound stays one)."""
    w, y = np.asarray(w, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ref = np.concatenate([hp_matmul(w.T, w).ravel(), hp_matmul(w.T, y[:, None]).ravel(), hp_matmul(y[None, :], y[:, None]).ravel()])
    aw, ay = np.abs(w), np.abs(y)
    mag = np.concatenate([(aw.T @ aw).ravel(), aw.T @ ay, [ay @ ay]]) * (1.0 - 2.0 * len(y) * U)
    return ref, mag


def stats_bound(mag, n_rows, T):
    rps, S, _last = split_plan(n_rows, T)
    return (rps + S + 4) * U * mag


def gamma(k):
    return k * U / (1.0 - k * U)


def conditioned_factor(D, seed):
    """(lam, mu, scales): lam = diag(s) (I + A A^T / D) diag(s) with s log-spaced from 1e-2 to 1e2, condition number about
    1e8 (the statistics' column scales would give 1e24, which no binary64 Cholesky factorises); mu is of order 1 / s."""
    rng = np.random.default_rng(seed)
    s = column_scales(D, 2)
    a = rng.standard_normal((D, D))
    lam = s[:, None] * (np.eye(D) + a @ a.T / D) * s[None, :]
    return (lam + lam.T) / 2.0, rng.standard_normal(D) / s, s


def conditioned_rows(D, N, seed, scales):
    rng = np.random.default_rng(seed)
    return scales * (rng.standard_normal((N, D)) + 1e3 * (np.arange(D) % 2))


def hp_predict(x, mu, linv, scale):
    """The read-out of the given binary64 factor in the wide type, and the bounds of the module docstring:
    (m, p_lambdas, bound on |m - ref|, bound on the relative error of p_lambdas)."""
    x, mu, linv = (np.asarray(v, dtype=np.float64) for v in (x, mu, linv))
    D = x.shape[1]
    z = hp_matmul(x, linv.T)
    m = hp_matmul(x, mu[:, None]).ravel()
    q = (z * z).sum(axis=1)
    lam = scale / (1 + q)
    slack = 1.0 - 2.0 * D * U                                   # (the float64 products of absolute values, as in hp_stats)
    e = gamma(D) * (np.abs(x) @ np.abs(linv).T) * slack
    zf, qf = np.asarray(np.abs(z), dtype=np.float64), np.asarray(q, dtype=np.float64)
    dq = (2.0 * zf * e + e * e).sum(axis=1) + gamma(D + 2) * qf
    return m, lam, gamma(D + 2) * (np.abs(x) @ np.abs(mu)) * slack, dq / (1.0 + qf) + 2.0 * U
