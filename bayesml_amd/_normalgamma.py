"""What ``linearregression`` and ``autoregressive`` share: both are the Normal-Gamma conjugate model

    y_n ~ N(theta . w_n, 1 / tau),   theta | tau ~ N(mu, (tau Lambda)^-1),   tau ~ Gamma(alpha, beta)

over rows w_n of D coefficients (the regressors, or [1, x[t-p], ..., x[t-1]]).  Validated assignment of the
hyperparameters, the closed-form update from the statistics block of ``include/regvb.h``, the estimates and the engine
seam live here; the D-sized algebra is host NumPy with the reference's formulas
(``bayesml/linearregression/_linearregression.py``, cited as ``ref-lr``, and ``bayesml/autoregressive/_autoregressive.py``,
``ref-ar``).
"""
from __future__ import annotations

import numpy as np

from . import _check
from ._exceptions import CriteriaError, ParameterFormatError
from ._native import PLOT_MSG  # noqa: F401  (the two model packages read it here)

_LOSS_MSG = "Unsupported loss function! This function supports \"squared\", \"0-1\", \"abs\", and \"KL\"."


def init_params(obj, prefixes, D):
    """Default hyperparameters (zero mean, identity precision, alpha = beta = 1) under every prefix."""
    for prefix in prefixes:
        setattr(obj, prefix + "mu_vec", np.zeros(D))
        setattr(obj, prefix + "lambda_mat", np.eye(D))
        setattr(obj, prefix + "alpha", 1.0)
        setattr(obj, prefix + "beta", 1.0)


def assign(obj, prefix, D, d_name, mu, lam, alpha, beta):
    """Validated assignment shared by set_h_params / set_h0_params / set_hn_params (ref-lr:93-114, ref-ar:92-113)."""
    if mu is not None:
        _check.float_vec(mu, prefix + "mu_vec", ParameterFormatError)
        _check.shape_consistency(mu.shape[0], prefix + "mu_vec.shape[0]", D, d_name, ParameterFormatError)
        getattr(obj, prefix + "mu_vec")[:] = mu
    if lam is not None:
        _check.pos_def_sym_mat(lam, prefix + "lambda_mat", ParameterFormatError)
        _check.shape_consistency(lam.shape[0], f"{prefix}lambda_mat.shape[0] and {prefix}lambda_mat.shape[1]", D, d_name,
                                 ParameterFormatError)
        getattr(obj, prefix + "lambda_mat")[:] = lam
    if alpha is not None:
        setattr(obj, prefix + "alpha", _check.pos_float(alpha, prefix + "alpha", ParameterFormatError))
    if beta is not None:
        setattr(obj, prefix + "beta", _check.pos_float(beta, prefix + "beta", ParameterFormatError))


def assign_params(obj, D, d_name, theta_vec, tau):
    """GenModel.set_params (ref-lr:150-160, ref-ar:149-159)."""
    if theta_vec is not None:
        _check.float_vec(theta_vec, "theta_vec", ParameterFormatError)
        _check.shape_consistency(theta_vec.shape[0], "theta_vec.shape[0]", D, d_name, ParameterFormatError)
        obj.theta_vec[:] = theta_vec
    if tau is not None:
        obj.tau = _check.pos_float(tau, "tau", ParameterFormatError)


def gen_params(obj):
    """tau ~ Gamma, then theta ~ N: the reference's call order on ``obj.rng`` (ref-lr:136-137, ref-ar:135-136)."""
    obj.tau = obj.rng.gamma(shape=obj.h_alpha, scale=1.0 / obj.h_beta)
    obj.theta_vec = obj.rng.multivariate_normal(mean=obj.h_mu_vec, cov=np.linalg.inv(obj.tau * obj.h_lambda_mat))


def split_stats(stats, D):
    """(G [D, D], c [D], s, n) of a statistics block [G | c | s | n]."""
    stats = np.asarray(stats, dtype=np.float64)
    return stats[:D * D].reshape(D, D), stats[D * D:D * D + D], float(stats[D * D + D]), int(round(stats[D * D + D + 1]))


def update(obj, stats, D):
    """The conjugate update (ref-lr:542-548, ref-ar:488-503) from G = sum w w^T, c = sum w y, s = sum y^2, n.  hn_beta
    keeps the reference's (cancelling) form on purpose: a better conditioned one would be a deviation."""
    g, c, s, n = split_stats(stats, D)
    lam0 = np.array(obj.hn_lambda_mat)
    mu0 = np.array(obj.hn_mu_vec)
    obj.hn_lambda_mat += g
    obj.hn_mu_vec[:] = np.linalg.solve(obj.hn_lambda_mat, c + lam0 @ mu0)
    obj.hn_alpha += n / 2.0
    obj.hn_beta += (-obj.hn_mu_vec @ obj.hn_lambda_mat @ obj.hn_mu_vec + s + mu0 @ lam0 @ mu0) / 2.0
    return n


def estimate(obj, loss, zero):
    """(theta_vec, tau) estimates under the four losses (ref-lr:593-621, ref-ar:532-548); ``zero`` is what "0-1" gives
    for tau when the mode does not exist (0.0 in linearregression, 0 in autoregressive)."""
    if loss == "squared":
        return obj.hn_mu_vec, obj.hn_alpha / obj.hn_beta
    if loss == "0-1":
        return obj.hn_mu_vec, ((obj.hn_alpha - 1.0) / obj.hn_beta if obj.hn_alpha >= 1.0 else zero)
    if loss == "abs":
        from scipy.stats import gamma
        return obj.hn_mu_vec, gamma.median(a=obj.hn_alpha, scale=1.0 / obj.hn_beta)
    if loss == "KL":
        from scipy.stats import gamma, multivariate_t
        return (multivariate_t(loc=obj.hn_mu_vec, shape=np.linalg.inv(obj.hn_alpha / obj.hn_beta * obj.hn_lambda_mat),
                               df=2.0 * obj.hn_alpha),
                gamma(a=obj.hn_alpha, scale=1.0 / obj.hn_beta))
    raise CriteriaError(_LOSS_MSG)


def student_t(loss, loc, lam, nu):
    """make_prediction (ref-lr:754-760, ref-ar:648-654)."""
    if loss in ("squared", "0-1", "abs"):
        return loc
    if loss == "KL":
        from scipy.stats import t
        return t(loc=loc, scale=1.0 / np.sqrt(lam), df=nu)
    raise CriteriaError(_LOSS_MSG)


def inverse_factor(lam):
    """L^-1 of lam = L L^T (lower triangular): x^T lam^-1 x = |L^-1 x|^2."""
    from scipy.linalg import solve_triangular
    chol = np.linalg.cholesky(lam)
    return np.tril(solve_triangular(chol, np.eye(lam.shape[0]), lower=True))


def data_pass(obj, D):
    """The model's RegressionPass (made on first use, kept for later calls), or the stand-in of the test seam
    ``obj._reg_pass_factory`` (tests/fake_regression_engine.py); the default is the HIP engine and has no fallback."""
    if obj._reg_pass_factory is not None:
        return obj._reg_pass_factory(D)
    if obj._engine is None:
        from ._regression import RegressionPass
        obj._engine = RegressionPass(D, obj._device)
    return obj._engine


# ---- sequential prediction (include/regseq.h; DESIGN.md 4f, "Sequential prediction") -----------------------------------------
def seq_pass(obj, D):
    """The model's RegressionSeqPass, or the stand-in of the test seam ``obj._regseq_pass_factory``
    (tests/regression_seq_oracle.py); as ``data_pass``, no fallback."""
    if obj._regseq_pass_factory is not None:
        return obj._regseq_pass_factory(D)
    if obj._seq_engine is None:
        from ._regseq import RegressionSeqPass
        obj._seq_engine = RegressionSeqPass(D, obj._device)
    return obj._seq_engine


def check_sequence_loss(loss, code_length):
    if loss is None:
        if not code_length:
            raise CriteriaError("loss=None returns the code lengths alone: pass code_length=True with it.")
    elif not (isinstance(loss, str) and loss in ("squared", "0-1", "abs", "KL")):
        raise CriteriaError(_LOSS_MSG)


def fetch(obj):
    """``obj._p`` = (p_ms, p_lambdas) as float64 ndarrays: device tensors are copied on the first read."""
    if not isinstance(obj._p[0], np.ndarray):
        obj._p = tuple(t.detach().to("cpu").double().numpy() for t in obj._p)
    return obj._p


def pred_and_update_sequence(obj, n, run, update, as_numpy, loss, code_length):
    """What the two models' ``pred_and_update_sequence`` share, after the sample has been accepted: ``run(start)`` gives
    (p_ms, p_lambdas, nats) of the n rows as device tensors from the state ``start`` (``_regseq.start_state``) and
    ``update()`` is the model's own ``update_posterior`` on the same sample, so that ``hn_*`` are its bits.  Leaves
    ``obj._p`` (on the device until first read) and ``obj.p_nus`` and returns what the method returns."""
    from ._regseq import start_state
    alpha0 = float(obj.hn_alpha)
    if n > 0:
        p_m, p_lambda, nats = run(start_state(obj.hn_mu_vec, obj.hn_lambda_mat, obj.hn_alpha, obj.hn_beta))
        update()
    else:                    # no rows: nothing to predict, nothing to learn, nothing to launch
        import torch
        p_m = p_lambda = nats = torch.zeros(0, dtype=torch.float64)
    obj._p = (p_m, p_lambda)
    # the device's own expression for alpha_i: alpha_0 + (rows before i) / 2, one rounding each
    obj.p_nus = 2.0 * (alpha0 + np.arange(n) / 2.0)
    if code_length and as_numpy:
        nats = nats.detach().to("cpu").numpy()
    if loss is None:
        return nats
    if loss == "KL":
        pred = student_t(loss, *fetch(obj), obj.p_nus)
    else:
        pred = fetch(obj)[0] if as_numpy else p_m
    return (pred, nats) if code_length else pred
