#!/usr/bin/env python3
"""Golden fixtures for linearregression.LearnModel and autoregressive.LearnModel, produced by the REFERENCE (build
container only):

    MPLBACKEND=Agg python tests/golden/make_golden_regression.py

A regressor matrix too large to commit is not stored: the fixture keeps the arguments of the seeded recipe in
tests/regression_oracle.py and a checksum of what it made (the targets are always stored).  Every case is also evaluated in long double with the same
formulas; the script refuses a case whose reference values are off by more than 2e-12 in any compared quantity, or
whose hn_beta cancels by more than c = y.y / (2 hn_beta) = 3000 (the tests compare at 1e-10).
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import autoregressive as ref_ar            # noqa: E402
from bayesml import linearregression as ref_lr          # noqa: E402
import regression_oracle as orc                         # noqa: E402

LD = np.longdouble
N_PRED = 300            # rows whose predictive parameters are stored
MAX_C = 3000.0
MAX_REF_ERR = 2e-12


def rel_err(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))


# ---- the same formulas in long double (numpy.linalg has no long double: a plain Cholesky) ---------------------------------
def ld_cholesky(a):
    a = np.array(a, dtype=LD)
    n = a.shape[0]
    low = np.zeros((n, n), dtype=LD)
    for j in range(n):
        low[j, j] = np.sqrt(a[j, j] - low[j, :j] @ low[j, :j])
        if j + 1 < n:
            low[j + 1:, j] = (a[j + 1:, j] - low[j + 1:, :j] @ low[j, :j]) / low[j, j]
    return low


def ld_solve(low, b):
    """a^-1 b for a = low low^T; b [n] or [n, m]."""
    b = np.array(b, dtype=LD)
    n = low.shape[0]
    z = np.zeros_like(b)
    for j in range(n):
        z[j] = (b[j] - low[j, :j] @ z[:j]) / low[j, j]
    out = np.zeros_like(b)
    for j in range(n - 1, -1, -1):
        out[j] = (z[j] - low[j + 1:, j] @ out[j + 1:]) / low[j, j]
    return out


def ld_gram(w, y, chunk=2000):
    w, y = np.asarray(w), np.asarray(y)
    d = w.shape[1]
    g, c, s = np.zeros((d, d), dtype=LD), np.zeros(d, dtype=LD), LD(0)
    for i in range(0, w.shape[0], chunk):
        wl, yl = w[i:i + chunk].astype(LD), y[i:i + chunk].astype(LD)
        g += wl.T @ wl
        c += wl.T @ yl
        s += yl @ yl
    return g, c, s


def ld_update(mu, lam, alpha, beta, w, y):
    g, c, s = ld_gram(w, y)
    lam_n = lam + g
    low = ld_cholesky(lam_n)
    mu_n = ld_solve(low, c + lam @ mu)
    beta_n = beta + (-mu_n @ lam_n @ mu_n + s + mu @ lam @ mu) / 2
    return mu_n, lam_n, alpha + LD(w.shape[0]) / 2, beta_n, low, float(s)


def ld_pred(mu, low, alpha, beta, w):
    w = np.asarray(w).astype(LD)
    q = np.sum(w.T * ld_solve(low, w.T), axis=0)
    return w @ mu, alpha / beta / (1 + q)


def ld_logdet(low):
    return 2 * np.sum(np.log(np.diag(low)))


def ld_lml(lam0, alpha0, beta0, low_n, alpha_n, beta_n, n):
    from scipy.special import gammaln
    # (gammaln has no long double; its arguments are exact halves and its float64 error is far below the line drawn here)
    return (alpha0 * np.log(LD(beta0)) - alpha_n * np.log(beta_n) + LD(gammaln(float(alpha_n))) - LD(gammaln(float(alpha0)))
            + (ld_logdet(ld_cholesky(lam0)) - ld_logdet(low_n) - n * np.log(2 * LD(np.pi))) / 2)


class Audit:
    """Collects the reference's own error against the long-double evaluation, and the cancellation factor c."""

    def __init__(self, name):
        self.name, self.worst, self.c = name, {}, 0.0

    def add(self, what, ref, exact):
        self.worst[what] = max(self.worst.get(what, 0.0), rel_err(ref, exact))

    def close(self):
        print(f"  {self.name}: c = {self.c:.0f}, reference vs long double: "
              + ", ".join(f"{k} {v:.1e}" for k, v in self.worst.items()))
        assert self.c <= MAX_C, (self.name, self.c)
        assert max(self.worst.values()) <= MAX_REF_ERR, (self.name, self.worst)


def state(m):
    return dict(hn_mu_vec=m.hn_mu_vec.copy(), hn_lambda_mat=m.hn_lambda_mat.copy(), hn_alpha=float(m.hn_alpha),
                hn_beta=float(m.hn_beta))


def prior_json(prior):
    return json.dumps({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in (prior or {}).items()})


def ld_prior(D, prior, prefix="h0_"):
    prior = prior or {}
    return (np.array(prior.get(prefix + "mu_vec", np.zeros(D)), dtype=LD),
            np.array(prior.get(prefix + "lambda_mat", np.eye(D)), dtype=LD),
            LD(prior.get(prefix + "alpha", 1.0)), LD(prior.get(prefix + "beta", 1.0)))


def estimates(m, out):
    out.update(est_sq_tau=float(m.estimate_params("squared")[1]), est_01_tau=float(m.estimate_params("0-1")[1]),
               est_abs_tau=float(m.estimate_params("abs")[1]), est_theta=m.estimate_params("squared")[0].copy())


def linreg_case(name, D, n, seed, tau=1.0, dtype=np.float64, prior=None, batches=1, from_gen_model=False):
    out = dict(D=D, N=n, batches=batches, prior=prior_json(prior), dtype=np.dtype(dtype).name)
    if from_gen_model:          # small case: the reference's own GenModel, stored (the drop-in's GenModel must reproduce it)
        gen = ref_lr.GenModel(D, seed=seed)
        gen.gen_params()
        x, y = gen.gen_sample(n)
        x, y = x.astype(dtype), y.astype(dtype)
        out.update(x=x, y=y, theta_vec=gen.theta_vec.copy(), gen_tau=float(gen.tau), gen_seed=seed)
    else:
        x, y, theta = orc.synth_linreg(D, n, seed, tau, dtype)
        out.update(theta_vec=theta)
        out.update(y=y)
        if x.nbytes <= 256 * 1024:
            out.update(x=x)
        else:
            out.update(seed=seed, tau=tau, checksum=orc.checksum(x))
    audit = Audit(name)
    m = ref_lr.LearnModel(D, **(prior or {}))
    mu, lam, alpha, beta = ld_prior(D, prior)
    lam0, alpha0, beta0 = lam.copy(), alpha, beta
    x64, y64 = x.astype(np.float64), y.astype(np.float64)      # the reference is fed the float64 widening of the same values
    yy = 0.0
    for i, (xp, yp) in enumerate(zip(np.array_split(x64, batches), np.array_split(y64, batches))):
        m.update_posterior(xp, yp)
        out.update({f"b{i}_{k}": v for k, v in state(m).items()})
        mu, lam, alpha, beta, low, s = ld_update(mu, lam, alpha, beta, xp, yp)
        yy += s
        audit.add("lambda", m.hn_lambda_mat, lam)
        audit.add("mu", m.hn_mu_vec, mu)
        audit.add("beta", m.hn_beta, beta)
        assert float(alpha) == m.hn_alpha
    audit.c = yy / (2.0 * m.hn_beta)
    estimates(m, out)
    assert set(m.estimate_params("squared", dict_out=True)) == {"theta_vec", "tau"}
    rows = x64[:N_PRED]
    m.calc_pred_dist(rows)
    out.update(p_ms=m.p_ms.copy(), p_lambdas=m.p_lambdas.copy(), p_nus=m.p_nus.copy(), pred_var=m.calc_pred_var(),
               lml=float(m.calc_log_marginal_likelihood()))
    pm, pl = ld_pred(mu, low, alpha, beta, rows)
    audit.add("p_ms", m.p_ms, pm)
    audit.add("p_lambdas", m.p_lambdas, pl)
    audit.add("lml", m.calc_log_marginal_likelihood(), ld_lml(lam0, alpha0, beta0, low, alpha, beta, n))
    # sequential prediction of two further points
    rng = np.random.default_rng(seed + 1000)
    nx = rng.standard_normal((2, D)).astype(dtype).astype(np.float64)
    ny = (nx @ out["theta_vec"] + rng.standard_normal(2) / np.sqrt(tau)).astype(dtype).astype(np.float64)
    preds = [m.pred_and_update(nx[0], float(ny[0])).copy(), m.pred_and_update(nx[1], float(ny[1]), loss="0-1").copy()]
    # (after_hn_lambda_mat is left out: it is the stored matrix plus two outer products, and 0.5 MB at D = 255)
    out.update(next_x=nx, next_y=ny, preds=np.array(preds),
               **{"after_" + k: v for k, v in state(m).items() if k != "hn_lambda_mat"})
    for i in range(2):
        mu, lam, alpha, beta, low, s = ld_update(mu, lam, alpha, beta, nx[i:i + 1], ny[i:i + 1])
    audit.add("after_mu", m.hn_mu_vec, mu)
    audit.add("after_beta", m.hn_beta, beta)
    audit.close()
    np.savez_compressed(os.path.join(HERE, name), **out)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


def ar_series(p, T, seed):
    """A stable AR(p) series with a level: coefficients 0.6 / p each, unit noise."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    a = np.full(p, 0.6 / max(p, 1))
    return lfilter([1.0], np.concatenate([[1.0], -a]), 0.3 + rng.standard_normal(T))


def ar_case(name, p, T, seed, paddings=(None,), prior=None, from_gen_model=False):
    if from_gen_model:
        gen = ref_ar.GenModel(p, theta_vec=np.concatenate([[0.3], np.full(p, 0.6 / p)]), tau=2.0, seed=seed)
        x = gen.gen_sample(T)
        out = dict(gen_seed=seed, gen_theta_vec=gen.theta_vec.copy(), gen_tau=2.0)
    else:
        x = ar_series(p, T, seed)
        out = {}
    out.update(p=p, T=T, x=x, prior=prior_json(prior), paddings=json.dumps(list(paddings)))
    audit = Audit(name)
    for padding in paddings:
        tag = "zeros_" if padding == "zeros" else "none_"
        m = ref_ar.LearnModel(p, **(prior or {}))
        m.update_posterior(x, padding=padding)
        out.update({tag + k: v for k, v in state(m).items()})
        w, y = orc.lag_matrix(x, p, padding)
        mu, lam, alpha, beta = ld_prior(p + 1, prior)
        mu, lam, alpha, beta, low, s = ld_update(mu, lam, alpha, beta, w, y)
        audit.add("lambda", m.hn_lambda_mat, lam)
        audit.add("mu", m.hn_mu_vec, mu)
        audit.add("beta", m.hn_beta, beta)
        assert float(alpha) == m.hn_alpha
        audit.c = max(audit.c, s / (2.0 * m.hn_beta))
        est = {}
        estimates(m, est)
        out.update({tag + k: v for k, v in est.items()})
        m.calc_pred_dist(x[T - p:])
        out.update({tag + "p_m": float(m.p_m), tag + "p_lambda": float(m.p_lambda), tag + "p_nu": float(m.p_nu)})
        wl = np.concatenate([[1.0], x[T - p:]])[None, :]
        pm, pl = ld_pred(mu, low, alpha, beta, wl)
        audit.add("p_m", m.p_m, pm[0])
        audit.add("p_lambda", m.p_lambda, pl[0])
        from scipy.stats import t as ss_t
        out[tag + "interval"] = np.array(ss_t.interval(0.9, loc=m.p_m, scale=1.0 / np.sqrt(m.p_lambda), df=m.p_nu))
        if T > p + 2:
            # two pred_and_update steps over the series' last values (the reference feeds p + 1 values: one row, no padding)
            m2 = ref_ar.LearnModel(p, **(prior or {}))
            m2.update_posterior(x[:T - 2], padding=padding)
            preds = [float(m2.pred_and_update(x[T - 2 - p:T - 1])), float(m2.pred_and_update(x[T - 1 - p:T], loss="abs"))]
            out.update({tag + "preds": np.array(preds)}, **{tag + "after_" + k: v for k, v in state(m2).items()})
    audit.close()
    np.savez_compressed(os.path.join(HERE, name), **out)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


def run_errors(mod, cases, filename):
    res = {}
    for name, fn in cases(mod).items():
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fn()
            res[name] = None
        except Exception as e:      # noqa: BLE001
            res[name] = type(e).__name__
    with open(os.path.join(HERE, filename), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(res)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
    from regression_error_cases import ar_error_cases, linreg_error_cases
    linreg_case("linreg_d8_n1000.npz", 8, 1000, seed=1, from_gen_model=True)
    linreg_case("linreg_d64_n20000_f32_batches3.npz", 64, 20000, seed=2, tau=4.0, dtype=np.float32, batches=3,
                prior=dict(h0_mu_vec=np.full(64, 0.25), h0_lambda_mat=np.eye(64) * 2.0 + 0.01, h0_alpha=2.5, h0_beta=0.5))
    linreg_case("linreg_d128_n30000_f32.npz", 128, 30000, seed=3, dtype=np.float32)
    linreg_case("linreg_d200_n5000.npz", 200, 5000, seed=4, tau=10.0)
    linreg_case("linreg_d255_n4000_f32.npz", 255, 4000, seed=5, dtype=np.float32)
    linreg_case("linreg_d5_n1.npz", 5, 1, seed=6)
    ar_case("ar_p3_t2000.npz", 3, 2000, seed=11, paddings=(None, "zeros"), from_gen_model=True)
    ar_case("ar_p16_t50000.npz", 16, 50000, seed=12,
            prior=dict(h0_mu_vec=np.full(17, 0.1), h0_lambda_mat=np.eye(17) * 3.0, h0_alpha=2.0, h0_beta=1.5))
    ar_case("ar_p64_t30000_zeros.npz", 64, 30000, seed=13, paddings=("zeros",))
    ar_case("ar_p4_t5.npz", 4, 5, seed=14, paddings=(None, "zeros"))
    run_errors(ref_lr, linreg_error_cases, "linreg_errors.json")
    run_errors(ref_ar, ar_error_cases, "ar_errors.json")
