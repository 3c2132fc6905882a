"""Held-out scoring and many-series passes of the regression family (csrc/regpred_kernels.h) on the GPU, against
``np.linalg.solve``, a longdouble Gram of explicitly built window rows and an mpmath Student-t log-density.

Tolerances: log-densities at 1e-10 (the line of ``regvb_predict`` in tests/test_gpu_regression.py), statistics at 1e-13
(``regvb_stats_window``'s), model quantities as tests/test_gpu_regression.py:172-173.  A fixed-order sum of n doubles of one
sign - at most 64 serial additions per lane, six butterfly levels, twice - is within 140 ulp of the exact sum: 1e-13.
"""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import regression_oracle as orc
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STATE = ("hn_mu_vec", "hn_lambda_mat", "hn_alpha", "hn_beta", "p_ms", "p_lambdas", "p_nus")


def ref_logpdf(m, w, y):
    """ln St(y | w . mu, (alpha / beta) / (1 + w^T Lambda^-1 w), 2 alpha) per row: solve in binary64, the density in mpmath."""
    w, y = np.asarray(w, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lam = m.hn_alpha / m.hn_beta / (1.0 + np.sum(w.T * np.linalg.solve(m.hn_lambda_mat, w.T), axis=0))
    mp.mp.dps = 40
    nu = mp.mpf(2.0 * m.hn_alpha)
    c0 = mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(mp.pi * nu) / 2
    return np.array([float(c0 + mp.log(l) / 2 - (nu + 1) / 2 * mp.log1p(l * (mp.mpf(a) - mp.mpf(b)) ** 2 / nu))
                     for a, b, l in zip(y, w @ m.hn_mu_vec, lam)])


def state(m):
    return {k: np.copy(getattr(m, k)) for k in STATE} | {"_n": getattr(m, "_n", None)}


def same_state(m, before):
    return all(np.array_equal(v, state(m)[k]) for k, v in before.items())


def lengths_for(p):
    """Several series in one 16-row batch, one that spans three, rowless ones between, an empty one last."""
    return [p + 2, 1, 0, p + 1, p, 17, 40, 16, 0]


def window_rows(x, lens, p, padding):
    """Per series: (rows, targets) of its own lag windows."""
    off = np.concatenate([[0], np.cumsum(lens)])
    return [orc.lag_matrix(x[a:b], p, padding) for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("D", (1, 16, 17, 32, 33, 160, 161, 256))
def test_matrix_rows_against_solve_and_mpmath(D):
    from bayesml_amd import linearregression as lr
    rng = np.random.default_rng(500 + D)
    m = lr.LearnModel(D, device=DEV)
    xf = rng.standard_normal((2 * D + 5, D))
    m.update_posterior(xf, xf @ rng.standard_normal(D) + rng.standard_normal(2 * D + 5))      # L^-1 is not the identity
    m.calc_pred_dist(xf[:3])
    before = state(m)
    for n in (1, 15, 16, 17, 63, 65):
        for xt, yt in ((np.float32, np.float64), (np.float64, np.float32)):
            x, y = rng.standard_normal((n, D + 3)).astype(xt), (5.0 + rng.standard_normal(n)).astype(yt)
            want = ref_logpdf(m, x[:, :D], y)
            lnp, tot = m.calc_pred_logpdf(np.ascontiguousarray(x[:, :D]), y, total=True)
            assert lnp.dtype == np.float64 and rel_err(lnp, want) < 1e-10, (n, xt)
            assert abs(tot - math.fsum(lnp)) <= 1e-13 * abs(math.fsum(lnp))
            xd = torch.from_numpy(x).to(DEV)[:, :D]                                 # read where it lies: ldx = D + 3
            strided = m.calc_pred_logpdf(xd, torch.from_numpy(y).to(DEV))
            assert (n == 1 or xd.stride(0) == D + 3) and strided.device.type == "cuda"
            assert np.array_equal(strided.cpu().numpy(), lnp), (n, xt)
    assert same_state(m, before)


@pytest.mark.parametrize("n", (4096, 4097, 3 * 4096 + 5))
def test_grand_total_at_the_chunk_edges(n):
    from bayesml_amd import linearregression as lr
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    m = lr.LearnModel(3, device=DEV)
    lnp, tot = m.calc_pred_logpdf(x, y, total=True)
    assert abs(tot - math.fsum(lnp)) <= 1e-13 * abs(math.fsum(lnp)) and tot == m.calc_pred_logpdf(x, y, total=True)[1]
    assert rel_err(lnp[-70:], ref_logpdf(m, x[-70:], y[-70:])) < 1e-10
    empty, zero = m.calc_pred_logpdf(x[:0], y[:0], total=True)
    assert empty.shape == (0,) and empty.dtype == np.float64 and zero == 0.0


def fitted_ar(p, rng):
    from bayesml_amd import autoregressive as ar
    return ar.LearnModel(p, device=DEV).update_posterior(0.3 + rng.standard_normal(3 * p + 20))


CASES = [(p, padding, None) for p in (0, 1, 15, 16, 31) for padding in (None, "zeros")]
CASES.append((1, "zeros", [20] + [0] * 600 + [20, 0]))          # more series in a workgroup's rows than its LDS slice holds


@pytest.mark.parametrize("p, padding, lens", CASES)
def test_windows_of_many_series_against_the_per_series_reference(p, padding, lens):
    rng = np.random.default_rng(600 + p)
    m = fitted_ar(p, rng)
    m.calc_pred_dist(np.ones(p))
    before = state(m)
    lens = lengths_for(p) if lens is None else lens
    off = np.concatenate([[0], np.cumsum(lens)])
    for dtype in (np.float64, np.float32):
        x = (0.3 + rng.standard_normal(off[-1])).astype(dtype)
        parts = [ref_logpdf(m, w, y) for w, y in window_rows(x, lens, p, padding)]
        lnp, tot = m.calc_pred_logpdf(x, padding, lengths=lens, totals=True)
        assert lnp.shape == (sum(len(v) for v in parts),) and rel_err(lnp, np.concatenate(parts)) < 1e-10, dtype
        sums = np.array([math.fsum(v) for v in parts])
        assert rel_err(tot, sums) < 1e-10 and np.all(tot[[len(v) == 0 for v in parts]] == 0.0)
        # the same positions scored as one concatenated series: only zeros before a series' own start can differ
        t0 = 0 if padding == "zeros" else p
        pos = np.concatenate([np.arange(a + t0, max(b, a + t0)) for a, b in zip(off[:-1], off[1:])])
        glued = m.calc_pred_logpdf(x, padding)[pos - t0]
        assert np.array_equal(glued, lnp) != (padding == "zeros" and p > 0)
        assert np.array_equal(m.calc_pred_logpdf(x, padding), m.calc_pred_logpdf(x, padding, lengths=[len(x)]))
        xd = torch.from_numpy(x).to(DEV)
        assert np.array_equal(m.calc_pred_logpdf(xd, padding, lengths=torch.tensor(lens)).cpu().numpy(), lnp)
    assert same_state(m, before)


@pytest.mark.parametrize("p, padding, lens", CASES)
def test_fit_from_many_series(p, padding, lens):
    from bayesml_amd import _regpred, autoregressive as ar
    from bayesml_amd._regression import PAD_NONE, PAD_ZEROS
    rng = np.random.default_rng(700 + p)
    lens = lengths_for(p) if lens is None else lens
    off = np.concatenate([[0], np.cumsum(lens)])
    x = 0.3 + rng.standard_normal(off[-1])
    rows = [wy for wy in window_rows(x, lens, p, padding) if len(wy[1])]
    w, y = (np.concatenate(v).astype(np.longdouble) for v in zip(*rows))
    want = np.concatenate([(w.T @ w).ravel(), w.T @ y, [y @ y, len(y)]]).astype(np.float64)
    eng = _regpred.RegressionScorePass(p + 1, DEV)
    pad = PAD_ZEROS if padding == "zeros" else PAD_NONE
    roff = _regpred.row_offsets(off, p, pad)
    for dtype in (np.float64, np.float32):
        args = (eng.adopt(x.astype(dtype)), pad, *eng.tables(off, roff), int(roff[-1]))
        got = eng.stats_window(*args)
        assert torch.equal(got, eng.stats_window(*args))
        if dtype == np.float64:
            assert rel_err(got.cpu().numpy(), want) < 1e-13 and got[-1].item() == len(y)
    one = ar.LearnModel(p, device=DEV).update_posterior(x, padding, lengths=lens)
    loop = ar.LearnModel(p, device=DEV)
    for a, b in zip(off[:-1], off[1:]):
        if b - a > (0 if padding == "zeros" else p):
            loop.update_posterior(x[a:b], padding, lengths=[b - a])
    assert rel_err(one.hn_lambda_mat, loop.hn_lambda_mat) < 1e-12 and rel_err(one.hn_mu_vec, loop.hn_mu_vec) < 1e-10
    assert one.hn_alpha == loop.hn_alpha and rel_err(one.hn_beta, loop.hn_beta) < 1e-10
    # one non-empty series among empty ones is today's single-series pass
    a, b = ar.LearnModel(p, device=DEV), ar.LearnModel(p, device=DEV)
    a.update_posterior(x[:40], padding, lengths=[0, 40, 0])
    b.update_posterior(x[:40], padding)
    assert a._engine.launch_info == "regvb_stats_window" and same_state(a, state(b))
