"""``normal.GenModel`` / ``LearnModel``: drop-in for ``bayesml/normal/_normal.py`` (cited below as ``ref:<lines>``).

``update_posterior(x)`` of an array is one pass of ``expfam_stats_normal`` over the sample where it lies: n, the mean and
the centred sum of squares m2 = sum (x - mean)^2, merged by the pairwise update of Chan et al. (the reference makes two
passes, ref:381-383; raw moments are never formed).  A scalar is folded in on the host.  The Normal-Gamma closed form on
(n, mean, m2) and everything else is scalar host code as in the reference.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _check, _expfam as xf, _expseq as xs, base
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError, ResultWarning

_LOSS_MSG = 'Unsupported loss function! This function supports "squared", "0-1", "abs", and "KL".'


class GenModel(base.Generative):
    """Data-generating model and its Normal-Gamma prior (ref:21-214; plotting is out of scope)."""

    def __init__(self, mu=0.0, tau=1.0, h_m=0.0, h_kappa=1.0, h_alpha=1.0, h_beta=1.0, seed=None):
        self.rng = np.random.default_rng(seed)
        self.mu = 0.0
        self.tau = 1.0
        self.h_m = 1.0
        self.h_kappa = 1.0
        self.h_alpha = 1.0
        self.h_beta = 1.0
        self.set_params(mu, tau)
        self.set_h_params(h_m, h_kappa, h_alpha, h_beta)

    def get_constants(self):
        return {}

    def set_h_params(self, h_m=None, h_kappa=None, h_alpha=None, h_beta=None):
        if h_m is not None:
            self.h_m = _check.float_(h_m, "h_m", ParameterFormatError)
        if h_kappa is not None:
            self.h_kappa = _check.pos_float(h_kappa, "h_kappa", ParameterFormatError)
        if h_alpha is not None:
            self.h_alpha = _check.pos_float(h_alpha, "h_alpha", ParameterFormatError)
        if h_beta is not None:
            self.h_beta = _check.pos_float(h_beta, "h_beta", ParameterFormatError)
        return self

    def get_h_params(self):
        return {"h_m": self.h_m, "h_kappa": self.h_kappa, "h_alpha": self.h_alpha, "h_beta": self.h_beta}

    def gen_params(self):
        """tau first, then mu given tau: the reference's order of draws (ref:112-113)."""
        self.tau = self.rng.gamma(shape=self.h_alpha, scale=1.0 / self.h_beta)
        self.mu = self.rng.normal(loc=self.h_m, scale=1.0 / np.sqrt(self.tau * self.h_kappa))
        return self

    def set_params(self, mu=None, tau=None):
        if mu is not None:
            self.mu = _check.float_(mu, "mu", ParameterFormatError)
        if tau is not None:
            self.tau = _check.pos_float(tau, "tau", ParameterFormatError)
        return self

    def get_params(self):
        return {"mu": self.mu, "tau": self.tau}

    def gen_sample(self, sample_size):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        return self.rng.normal(loc=self.mu, scale=1.0 / np.sqrt(self.tau), size=sample_size)

    def save_sample(self, filename, sample_size):
        np.savez_compressed(filename, x=self.gen_sample(sample_size))

    def visualize_model(self, sample_size=1000, hist_bins=10):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        _check.pos_int(hist_bins, "hist_bins", DataFormatError)
        self.gen_sample(sample_size)        # (the reference draws its sample and prints nothing)
        raise NotImplementedError(xf.PLOT_MSG)


class LearnModel(xf.PassOwner, base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:216-661).  Positional parameters are the reference's; keyword-only
    ``device`` selects the GPU.  The sample may be a NumPy array or a torch tensor (integer samples are widened)."""

    def __init__(self, h0_m=0.0, h0_kappa=1.0, h0_alpha=1.0, h0_beta=1.0, *, device=None):
        self._init_pass(device)
        self.h0_m = 0.0
        self.h0_kappa = 1.0
        self.h0_alpha = 1.0
        self.h0_beta = 1.0
        self.hn_m = 0.0
        self.hn_kappa = 1.0
        self.hn_alpha = 1.0
        self.hn_beta = 1.0
        self.p_mu = 1.0
        self.p_nu = 2.0
        self.p_lambda = 0.5
        self._n = 0
        self.set_h0_params(h0_m, h0_kappa, h0_alpha, h0_beta)

    def get_constants(self):
        return {}

    def set_h0_params(self, h0_m=None, h0_kappa=None, h0_alpha=None, h0_beta=None):
        if h0_m is not None:
            self.h0_m = _check.float_(h0_m, "h0_m", ParameterFormatError)
        if h0_kappa is not None:
            self.h0_kappa = _check.pos_float(h0_kappa, "h0_kappa", ParameterFormatError)
        if h0_alpha is not None:
            self.h0_alpha = _check.pos_float(h0_alpha, "h0_alpha", ParameterFormatError)
        if h0_beta is not None:
            self.h0_beta = _check.pos_float(h0_beta, "h0_beta", ParameterFormatError)
        self.reset_hn_params()
        return self

    def get_h0_params(self):
        return {"h0_m": self.h0_m, "h0_kappa": self.h0_kappa, "h0_alpha": self.h0_alpha, "h0_beta": self.h0_beta}

    def set_hn_params(self, hn_m=None, hn_kappa=None, hn_alpha=None, hn_beta=None):
        self._n = 0
        if hn_m is not None:
            self.hn_m = _check.float_(hn_m, "hn_m", ParameterFormatError)
        if hn_kappa is not None:
            self.hn_kappa = _check.pos_float(hn_kappa, "hn_kappa", ParameterFormatError)
        if hn_alpha is not None:
            self.hn_alpha = _check.pos_float(hn_alpha, "hn_alpha", ParameterFormatError)
        if hn_beta is not None:
            self.hn_beta = _check.pos_float(hn_beta, "hn_beta", ParameterFormatError)
        self.calc_pred_dist()
        return self

    def get_hn_params(self):
        return {"hn_m": self.hn_m, "hn_kappa": self.hn_kappa, "hn_alpha": self.hn_alpha, "hn_beta": self.hn_beta}

    def _moments(self, x, check):
        """(n, mean, m2) of a sample; arrays go through the device pass."""
        if not xf.is_array(x):
            if check:
                x = _check.floats(x, "x", DataFormatError)
            return 1, x, 0.0
        if check and _check.sample_kind(x) is None:
            raise DataFormatError("x" + _check.SAMPLE_MSG["floats"])
        if xf.size_of(x) == 0:
            return 0, np.float64(np.nan), 0.0          # the reference's 0 / 0
        st = self._sample_stats(xf.NORMAL, x, "f")
        return st["n"], st["mean"], st["m2"]

    def _fold(self, n, x_bar, m2):
        """The Normal-Gamma update from the sample's (n, mean, centred sum of squares) (ref:383-387)."""
        self.hn_beta += (m2 + n * self.hn_kappa / (self.hn_kappa + n) * (x_bar - self.hn_m) ** 2) / 2.0
        self.hn_m = (self.hn_kappa * self.hn_m + n * x_bar) / (self.hn_kappa + n)
        self.hn_kappa += n
        self.hn_alpha += n * 0.5
        self._n += n
        return self

    def update_posterior(self, x):
        return self._fold(*self._moments(x, True))

    def _update_posterior(self, x):
        """Update without input check (ref:390-400)."""
        return self._fold(*self._moments(x, False))

    def estimate_params(self, loss="squared", dict_out=False):
        """(mu, tau) estimated independently: means, modes, medians, or the Student-t and Gamma marginals themselves
        (ref:402-455)."""
        if loss == "squared":
            tau = self.hn_alpha / self.hn_beta
        elif loss == "0-1":
            tau = (self.hn_alpha - 1.0) / self.hn_beta if self.hn_alpha > 1.0 else 0.0
        elif loss == "abs":
            from scipy.stats import gamma as ss_gamma
            tau = ss_gamma.median(a=self.hn_alpha, scale=1 / self.hn_beta)
        elif loss == "KL":
            from scipy.stats import gamma as ss_gamma, t as ss_t
            return (ss_t(loc=self.hn_m, scale=np.sqrt(self.hn_beta / self.hn_alpha / self.hn_kappa), df=2 * self.hn_alpha),
                    ss_gamma(a=self.hn_alpha, scale=1.0 / self.hn_beta))
        else:
            raise CriteriaError(_LOSS_MSG)
        return {"mu": self.hn_m, "tau": tau} if dict_out else (self.hn_m, tau)

    def estimate_interval(self, credibility=0.95):
        from scipy.stats import gamma as ss_gamma, t as ss_t
        _check.float_in_closed01(credibility, "credibility", CriteriaError)
        return (ss_t.interval(credibility, loc=self.hn_m, scale=np.sqrt(self.hn_beta / self.hn_alpha / self.hn_kappa),
                              df=2 * self.hn_alpha),
                ss_gamma.interval(credibility, a=self.hn_alpha, scale=1.0 / self.hn_beta))

    def visualize_posterior(self):
        raise NotImplementedError(xf.PLOT_MSG)

    def get_p_params(self):
        return {"p_mu": self.p_mu, "p_lambda": self.p_lambda, "p_nu": self.p_nu}

    def calc_pred_dist(self):
        self.p_mu = self.hn_m
        self.p_nu = 2 * self.hn_alpha
        self.p_lambda = self.hn_kappa / (self.hn_kappa + 1) * self.hn_alpha / self.hn_beta
        return self

    def _calc_pred_density(self, x):
        from scipy.stats import t as ss_t
        return ss_t.pdf(x, loc=self.p_mu, scale=1.0 / np.sqrt(self.p_lambda), df=self.p_nu)

    def make_prediction(self, loss="squared"):
        if loss == "squared" or loss == "0-1" or loss == "abs":
            return self.p_mu
        if loss == "KL":
            from scipy.stats import t as ss_t
            return ss_t(loc=self.p_mu, scale=1.0 / np.sqrt(self.p_lambda), df=self.p_nu)
        raise CriteriaError(_LOSS_MSG)

    def pred_and_update(self, x, loss="squared"):
        """Predict, then fold the scalar x in: host only (ref:561-588)."""
        _check.float_(x, "x", DataFormatError)
        self.calc_pred_dist()
        prediction = self.make_prediction(loss=loss)
        self.update_posterior(x)
        return prediction

    def pred_and_update_sequence(self, x, loss="squared", *, code_length=False):
        """``[pred_and_update(x[i], loss) for i in range(n)]`` in one device pass (include/expseq.h): the exclusive prefix
        (count, mean, m2) about the pivot x[0] gives ``p_mu``, ``p_nu`` and ``p_lambda`` of every position.  x is accepted
        and refused as ``update_posterior`` does it.  Returns float64 ``p_mu`` ("squared", "0-1", "abs") or on the host
        the frozen Student-t over the parameter arrays ("KL"); with ``code_length`` also
        ``nats[i] = -ln p(x[i] | x[:i])``; ``loss=None`` returns the nats alone and leaves ``p_mu``, ``p_nu`` and
        ``p_lambda``."""
        def predict(loss, params):
            p_mu, p_nu, p_lambda = params
            if loss != "KL":
                return p_mu
            from scipy.stats import t as ss_t
            return ss_t(loc=xs.host(p_mu), scale=1.0 / np.sqrt(xs.host(p_lambda)), df=xs.host(p_nu))

        return xs.sequence(self, xs.NORMAL, x, loss, code_length, ("squared", "0-1", "abs", "KL"), _LOSS_MSG,
                           lambda: self._moments(x, True), lambda st: self._fold(*st),
                           (self.hn_m, self.hn_kappa, self.hn_alpha, self.hn_beta), predict)

    def calc_log_marginal_likelihood(self):
        from scipy.special import gammaln
        return (self.h0_alpha * np.log(self.h0_beta) - self.hn_alpha * np.log(self.hn_beta) + gammaln(self.hn_alpha)
                - gammaln(self.h0_alpha)
                + 0.5 * (np.log(self.h0_kappa) - np.log(self.hn_kappa) - self._n * np.log(2 * np.pi)))

    def calc_pred_var(self):
        if self.p_nu > 2:
            return self.p_nu / self.p_lambda / (self.p_nu - 2)
        warnings.warn("Variance of the predictive distribution cannot defined for the current p_nu.", ResultWarning)
        return np.nan

    def fit(self, x):
        self.reset_hn_params()
        self.update_posterior(x)
        return self

    def predict(self):
        self.calc_pred_dist()
        return self.make_prediction(loss="squared")
