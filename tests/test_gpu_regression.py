"""The regression kernels (csrc/regvb_kernels.h) on the GPU: the statistics pass, the lag-window loader and the predictive
read-out against float64 NumPy on odd shapes, run-to-run identity, and the full-size properties of the two learners.

Tolerances: statistics against float64 NumPy at 1e-13 (both are f64 sums of the same products in a different order);
the predictive read-out against ``solve`` at 1e-10, the line tests/test_regression.py draws for p_ms / p_lambdas (it goes
through a factorisation on both sides); model quantities at the 1e-10 / 1e-12 of tests/test_mvn.py.
"""
import numpy as np
import pytest
import torch

import regression_oracle as orc
from conftest import rel_err

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 4097)
DS = (1, 2, 15, 16, 17, 49, 128, 129, 255, 256)


def dev():
    return torch.device("cuda", 0)


def engine(D):
    from bayesml_amd._regression import RegressionPass
    return RegressionPass(D, dev())


def block(w, y):
    w, y = np.asarray(w, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.concatenate([(w.T @ w).ravel(), w.T @ y, [y @ y, float(w.shape[0])]])


@pytest.mark.parametrize("D", DS)
def test_stats_against_numpy_on_odd_shapes(D):
    """f32 and f64 rows, contiguous and strided (ldx > D), every N of the grid; the Gram matrix is exactly symmetric and a
    second run gives the same bits."""
    eng = engine(D)
    rng = np.random.default_rng(100 + D)
    for N in NS:
        for dtype in (np.float32, np.float64):
            for pad in (0, 3):
                x = rng.standard_normal((N, D + pad)).astype(dtype)
                y = rng.standard_normal(N).astype(dtype)
                xd = torch.from_numpy(x).to(dev())[:, :D]
                yd = torch.from_numpy(y).to(dev())
                assert pad == 0 or N == 1 or xd.stride(0) == D + pad
                s1 = eng.stats(eng.adopt(xd), yd)
                s2 = eng.stats(eng.adopt(xd), yd)
                assert torch.equal(s1, s2), (N, dtype, pad)
                s1 = s1.cpu().numpy()
                assert rel_err(s1, block(x[:, :D], y)) < 1e-13, (N, dtype, pad)
                G = s1[:D * D].reshape(D, D)
                assert np.array_equal(G, G.T) and s1[-1] == N


@pytest.mark.parametrize("p", (0, 1, 2, 15, 16, 63))
def test_window_loader_against_explicit_lag_matrix(p):
    from bayesml_amd._regression import PAD_NONE, PAD_ZEROS
    eng = engine(p + 1)
    rng = np.random.default_rng(200 + p)
    for T in (p + 1, p + 2, 1000, 100003):
        for dtype in (np.float64, np.float32):
            x = (0.5 + rng.standard_normal(T)).astype(dtype)
            xd = torch.from_numpy(x).to(dev())
            for code, padding in ((PAD_NONE, None), (PAD_ZEROS, "zeros")):
                s1 = eng.stats_window(xd, code)
                assert torch.equal(s1, eng.stats_window(xd, code)), (T, padding)
                w, y = orc.lag_matrix(x, p, padding)
                assert rel_err(s1.cpu().numpy(), block(w, y)) < 1e-13, (T, dtype, padding)


@pytest.mark.parametrize("D", DS)
def test_predict_against_numpy_solve(D):
    from bayesml_amd._normalgamma import inverse_factor
    eng = engine(D)
    rng = np.random.default_rng(300 + D)
    a = rng.standard_normal((D, D))
    lam = a @ a.T + D * np.eye(D)
    mu = rng.standard_normal(D)
    linv = inverse_factor(lam)
    for N in NS:
        for dtype in (np.float32, np.float64):
            for pad in (0, 3):
                x = rng.standard_normal((N, D + pad)).astype(dtype)
                xd = eng.adopt(torch.from_numpy(x).to(dev())[:, :D])
                pm, pl = eng.predict(xd, mu, linv, 1.75)
                pm2, pl2 = eng.predict(xd, mu, linv, 1.75)
                assert torch.equal(pm, pm2) and torch.equal(pl, pl2), (N, dtype, pad)
                x64 = x[:, :D].astype(np.float64)
                q = np.sum(x64.T * np.linalg.solve(lam, x64.T), axis=0)
                assert rel_err(pm.cpu().numpy(), x64 @ mu) < 1e-10, (N, dtype, pad)
                assert rel_err(pl.cpu().numpy(), 1.75 / (1.0 + q)) < 1e-10, (N, dtype, pad)


@pytest.mark.parametrize("D", (1, 17, 128, 255))
def test_stats_with_different_dtypes_of_x_and_y(D):
    """x f32 / y f64 and x f64 / y f32 against float64 NumPy on the values as given: each is widened, none narrowed
    (targets with an offset, so that a y rounded to f32 would be off by 6e-8, not 1e-13)."""
    eng = engine(D)
    rng = np.random.default_rng(400 + D)
    for N in (1, 17, 4097):
        x64 = rng.standard_normal((N, D)) * (1.0 + 2.0 ** -30)
        y64 = 1000.0 + rng.standard_normal(N)
        for xt, yt in ((np.float32, np.float64), (np.float64, np.float32)):
            x, y = x64.astype(xt), y64.astype(yt)
            xd, yd = eng.adopt(x), eng.adopt(y)
            assert xd.dtype != yd.dtype
            s1 = eng.stats(xd, yd)
            assert torch.equal(s1, eng.stats(xd, yd))
            assert rel_err(s1.cpu().numpy(), block(x, y)) < 1e-13, (N, xt, yt)
            # the element that is only y: s = sum y^2, exact to rounding in the caller's values
            assert abs(s1[-2].item() - float(y.astype(np.float64) @ y.astype(np.float64))) <= 1e-13 * s1[-2].item()


def _big_linreg():
    gen = torch.Generator(device=dev()).manual_seed(7)
    D, N = 128, 4_000_000
    theta = torch.randn(D, device=dev(), generator=gen, dtype=torch.float64)
    x = torch.randn(N, D, device=dev(), generator=gen, dtype=torch.float32)
    noise = torch.randn(N, device=dev(), generator=gen, dtype=torch.float64) * 0.5
    y = (x.to(torch.float64) @ theta + noise).to(torch.float32)
    return x, y, theta.cpu().numpy()


def test_linreg_full_size_additivity_and_recovery():
    """N = 4e6 rows of D = 128 f32 on the device: one update == two sequential updates on an uneven split (the
    statistics are linear in the rows), and theta is recovered to the statistical error: the posterior mean's
    standard deviation is sigma / sqrt(N) = 0.5 / 2000 = 2.5e-4 per coefficient (unit-variance regressors), so
    six of them bound all 128 deviations unless something is wrong."""
    from bayesml_amd import linearregression as lr
    x, y, theta = _big_linreg()
    a = lr.LearnModel(128, device=dev()).update_posterior(x, y)
    b = lr.LearnModel(128, device=dev())
    b.update_posterior(x[:1_700_001], y[:1_700_001])
    b.update_posterior(x[1_700_001:], y[1_700_001:])
    assert rel_err(a.hn_lambda_mat, b.hn_lambda_mat) < 1e-12 and rel_err(a.hn_mu_vec, b.hn_mu_vec) < 1e-11
    assert a.hn_alpha == b.hn_alpha and rel_err(a.hn_beta, b.hn_beta) < 1e-10
    assert a._n == b._n == 4_000_000
    assert np.max(np.abs(a.hn_mu_vec - theta)) < 6 * 0.5 / 2000.0
    assert abs(a.estimate_params("squared")[1] - 4.0) < 0.05          # tau = 1 / 0.5^2
    # predict on all rows == predict on 10000-row slices, slice for slice (a row's result does not depend on its neighbours)
    whole = a.predict(x).copy()
    whole_l = a.p_lambdas.copy()
    assert whole.shape == (4_000_000,) and a.p_nus.shape == (4_000_000,)
    for lo in (0, 1_230_000, 3_990_000):
        part = a.predict(x[lo:lo + 10_000])
        assert np.array_equal(part, whole[lo:lo + 10_000]) and np.array_equal(a.p_lambdas, whole_l[lo:lo + 10_000])
    ref = (x[:10_000].to(torch.float64) @ torch.from_numpy(a.hn_mu_vec).to(dev())).cpu().numpy()
    assert rel_err(whole[:10_000], ref) < 1e-10


def test_ar_full_size_against_explicit_lag_matrix_on_device():
    """T = 1e7, p = 16: the window loader equals the explicit lag-matrix route done in torch f64 on the device."""
    from bayesml_amd import autoregressive as ar
    p, T = 16, 10_000_000
    gen = torch.Generator(device=dev()).manual_seed(9)
    e = torch.randn(T + 1, device=dev(), generator=gen, dtype=torch.float64)
    x = 0.3 + e[1:] + 0.6 * e[:-1]         # MA(1): the lag covariance has condition number (1.6 / 0.4)^2 = 16
    for padding in (None, "zeros"):
        m = ar.LearnModel(p, device=dev()).update_posterior(x, padding=padding)
        xp = torch.cat([torch.zeros(p, dtype=torch.float64, device=dev()), x])
        w = torch.cat([torch.ones(T, 1, dtype=torch.float64, device=dev()), xp.unfold(0, p, 1)[:T]], dim=1)
        t0 = 0 if padding == "zeros" else p
        w, y = w[t0:], x[t0:]
        g, c, s = (w.T @ w).cpu().numpy(), (w.T @ y).cpu().numpy(), float(y @ y)
        del w
        lam = np.eye(p + 1) + g
        mu = np.linalg.solve(lam, c)
        beta = 1.0 + (-mu @ lam @ mu + s) / 2.0
        assert rel_err(m.hn_lambda_mat, lam) < 1e-12 and rel_err(m.hn_mu_vec, mu) < 1e-10
        assert m.hn_alpha == 1.0 + (T - t0) / 2.0 and rel_err(m.hn_beta, beta) < 1e-10
