"""NumPy restatement of the Normal-Gamma updates and predictive of linearregression / autoregressive (TEST
INFRASTRUCTURE ONLY), pinned to reference-generated fixtures in tests/test_regression.py, plus the seeded input
recipe of the regressor matrices that are too large to store (tests/golden/make_golden_regression.py stores the recipe's
arguments and a checksum instead of the matrix)."""
import numpy as np


# ---- inputs ----------------------------------------------------------------------------------------------------------
def synth_regressors(D, N, seed, dtype):
    """(theta, x): theta ~ N(0, I) and standard normal regressors with a constant last column, rounded to ``dtype``.
    Only the Generator's own stream is used (no BLAS, no reductions), so every machine makes the same bits."""
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal(D)
    x = rng.standard_normal((N, D))
    x[:, -1] = 1.0
    return theta, x.astype(dtype), rng


def synth_linreg(D, N, seed, tau, dtype):
    """(x, y, theta) with y = x . theta + N(0, 1 / tau) rounded to ``dtype``: what the fixtures' generator calls.  y goes
    through a matrix product, whose last bits depend on the machine: fixtures store it.  c = y.y / (2 hn_beta) is about
    tau D + 1 for this recipe."""
    theta, x, rng = synth_regressors(D, N, seed, dtype)
    y = x.astype(np.float64) @ theta + rng.standard_normal(N) / np.sqrt(tau)
    return x, y.astype(dtype), theta


def checksum(a):
    """What a fixture stores of a recipe-made array: the CRC of its bytes."""
    import zlib
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def linreg_inputs(g):
    """(x, y) of a linreg fixture; x is stored, or re-made from the recipe and verified against the stored checksum."""
    if "x" in g:
        return g["x"], g["y"]
    dtype = np.float32 if str(g["dtype"]) == "float32" else np.float64
    _theta, x, _rng = synth_regressors(int(g["D"]), int(g["N"]), int(g["seed"]), dtype)
    assert checksum(x) == int(g["checksum"]), "the input recipe no longer reproduces the fixture's regressors"
    return x, g["y"]


# ---- the model -------------------------------------------------------------------------------------------------------
def lag_matrix(x, p, padding):
    """Rows [1, x[t-p], ..., x[t-1]] (oldest first) and targets x[t]; t = p .. T-1, or t = 0 .. T-1 with zeros at
    negative times when padding == "zeros"."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    xp = np.concatenate([np.zeros(p), x])
    w = np.ones((T, p + 1))
    for k in range(p):
        w[:, 1 + k] = xp[k:k + T]
    t0 = 0 if padding == "zeros" else p
    return w[t0:], x[t0:]


def update(mu, lam, alpha, beta, w, y):
    """One conjugate update from rows w [N, D] and targets y [N] (float64), in the reference's formulas."""
    w = np.asarray(w, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    lam_n = lam + w.T @ w
    mu_n = np.linalg.solve(lam_n, w.T @ y + lam @ mu)
    alpha_n = alpha + w.shape[0] / 2.0
    beta_n = beta + (-mu_n @ lam_n @ mu_n + y @ y + mu @ lam @ mu) / 2.0
    return mu_n, lam_n, alpha_n, beta_n


def pred_params(mu, lam, alpha, beta, w):
    """(p_ms, p_lambdas, p_nus) for the rows w."""
    w = np.asarray(w, dtype=np.float64)
    q = np.sum(w.T * np.linalg.solve(lam, w.T), axis=0)
    return w @ mu, alpha / beta / (1.0 + q), np.ones(w.shape[0]) * 2.0 * alpha


def log_marginal_likelihood(lam0, alpha0, beta0, lam_n, alpha_n, beta_n, n):
    from scipy.special import gammaln
    return (alpha0 * np.log(beta0) - alpha_n * np.log(beta_n) + gammaln(alpha_n) - gammaln(alpha0)
            + 0.5 * (np.linalg.slogdet(lam0)[1] - np.linalg.slogdet(lam_n)[1] - n * np.log(2 * np.pi)))
