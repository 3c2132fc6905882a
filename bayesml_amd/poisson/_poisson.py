"""``poisson.GenModel`` / ``LearnModel``: drop-in for ``bayesml/poisson/_poisson.py`` (cited below as ``ref:<lines>``).

``update_posterior(x)`` of an array is one pass of ``expfam_stats_poisson`` over the sample where it lies: the count of
negative values (the reference's ``nonneg_ints`` check), the exact int64 sum and the binary64 sum of ``lgamma(x + 1)``
(ref:296-314: one check and two passes).  A scalar is folded in on the host.  Everything else is scalar host code.
"""
from __future__ import annotations

import numpy as np

from .. import _check, _expfam as xf, _expseq as xs, base
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError

_LOSS_MSG = 'Unsupported loss function! This function supports "squared", "0-1", "abs", and "KL".'


class GenModel(base.Generative):
    """Data-generating model and its Gamma prior (ref:20-186; plotting is out of scope)."""

    def __init__(self, lambda_=1.0, h_alpha=1.0, h_beta=1.0, seed=None):
        self.rng = np.random.default_rng(seed)
        self.lambda_ = 1.0
        self.h_alpha = 1.0
        self.h_beta = 1.0
        self.set_params(lambda_)
        self.set_h_params(h_alpha, h_beta)

    def get_constants(self):
        return {}

    def set_h_params(self, h_alpha=None, h_beta=None):
        if h_alpha is not None:
            self.h_alpha = _check.pos_float(h_alpha, "h_alpha", ParameterFormatError)
        if h_beta is not None:
            self.h_beta = _check.pos_float(h_beta, "h_beta", ParameterFormatError)
        return self

    def get_h_params(self):
        return {"h_alpha": self.h_alpha, "h_beta": self.h_beta}

    def gen_params(self):
        self.lambda_ = self.rng.gamma(shape=self.h_alpha, scale=1.0 / self.h_beta)
        return self

    def set_params(self, lambda_=None):
        if lambda_ is not None:
            self.lambda_ = _check.pos_float(lambda_, "lambda_", ParameterFormatError)
        return self

    def get_params(self):
        return {"lambda_": self.lambda_}

    def gen_sample(self, sample_size):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        return self.rng.poisson(self.lambda_, sample_size)

    def save_sample(self, filename, sample_size):
        np.savez_compressed(filename, x=self.gen_sample(sample_size))

    def visualize_model(self, sample_size=20):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        print(f"lambda:{self.lambda_}")
        x = self.gen_sample(sample_size)
        print(f"x:{x}")
        raise NotImplementedError(xf.PLOT_MSG)


class LearnModel(xf.PassOwner, base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:188-551).  Positional parameters are the reference's; keyword-only
    ``device`` selects the GPU.  The sample may be a NumPy array or a torch tensor of an integer dtype."""

    def __init__(self, h0_alpha=1.0, h0_beta=1.0, *, device=None):
        self._init_pass(device)
        self.h0_alpha = 1.0
        self.h0_beta = 1.0
        self.hn_alpha = 1.0
        self.hn_beta = 1.0
        self.p_r = 1.0
        self.p_theta = 0.5
        self._sum_log_factorial = 0.0
        self.set_h0_params(h0_alpha, h0_beta)

    def get_constants(self):
        return {}

    def set_h0_params(self, h0_alpha=None, h0_beta=None):
        if h0_alpha is not None:
            self.h0_alpha = _check.pos_float(h0_alpha, "h0_alpha", ParameterFormatError)
        if h0_beta is not None:
            self.h0_beta = _check.pos_float(h0_beta, "h0_beta", ParameterFormatError)
        self.reset_hn_params()
        return self

    def get_h0_params(self):
        return {"h0_alpha": self.h0_alpha, "h0_beta": self.h0_beta}

    def set_hn_params(self, hn_alpha=None, hn_beta=None):
        self._sum_log_factorial = 0.0
        if hn_alpha is not None:
            self.hn_alpha = _check.pos_float(hn_alpha, "hn_alpha", ParameterFormatError)
        if hn_beta is not None:
            self.hn_beta = _check.pos_float(hn_beta, "hn_beta", ParameterFormatError)
        self.calc_pred_dist()
        return self

    def get_hn_params(self):
        return {"hn_alpha": self.hn_alpha, "hn_beta": self.hn_beta}

    def _sums(self, x, check):
        """(sum x, n, sum log x!) of a sample.  Arrays go through the device pass; with ``check`` a negative value
        refuses the sample before anything is changed."""
        if not xf.is_array(x):
            from scipy.special import gammaln
            if check:
                _check.nonneg_ints(x, "x", DataFormatError)
            return x, 1, gammaln(x + 1)
        if check and _check.sample_kind(x) != "i":
            raise DataFormatError("x" + _check.SAMPLE_MSG["nonneg_ints"])
        if xf.size_of(x) == 0:
            return 0, 0, 0.0
        st = self._sample_stats(xf.POISSON, x, "i")
        if check and st["bad"] > 0:
            raise DataFormatError("x" + _check.SAMPLE_MSG["nonneg_ints"])
        return st["sum"], st["n"] - st["bad"], st["sum_lgamma"]

    def _fold(self, s, n, slf):
        self.hn_alpha += s
        self.hn_beta += n
        self._sum_log_factorial += slf
        return self

    def update_posterior(self, x):
        """hn_alpha += sum x, hn_beta += n, and the running sum of log x! for the marginal likelihood (ref:299-314)."""
        return self._fold(*self._sums(x, True))

    def _update_posterior(self, x):
        """Update without input check (ref:316-321): negative values are left out of all three sums."""
        return self._fold(*self._sums(x, False))

    def estimate_params(self, loss="squared", dict_out=False):
        """Posterior mean, mode, median or the Gamma posterior itself (ref:323-371)."""
        if loss == "squared":
            est = self.hn_alpha / self.hn_beta
        elif loss == "0-1":
            est = (self.hn_alpha - 1.0) / self.hn_beta if self.hn_alpha > 1.0 else 0.0
        elif loss == "abs":
            from scipy.stats import gamma as ss_gamma
            est = ss_gamma.median(a=self.hn_alpha, scale=1 / self.hn_beta)
        elif loss == "KL":
            from scipy.stats import gamma as ss_gamma
            return ss_gamma(a=self.hn_alpha, scale=1 / self.hn_beta)
        else:
            raise CriteriaError(_LOSS_MSG)
        return {"lambda_": est} if dict_out else est

    def estimate_interval(self, credibility=0.95):
        """As the reference (ref:386-387), which hands ``hn_beta`` to SciPy as the location of the Gamma distribution."""
        from scipy.stats import gamma as ss_gamma
        _check.float_in_closed01(credibility, "credibility", CriteriaError)
        return ss_gamma.interval(credibility, self.hn_alpha, self.hn_beta)

    def visualize_posterior(self):
        raise NotImplementedError(xf.PLOT_MSG)

    def get_p_params(self):
        return {"p_r": self.p_r, "p_theta": self.p_theta}

    def calc_pred_dist(self):
        self.p_r = self.hn_alpha
        self.p_theta = 1.0 / (1.0 + self.hn_beta)
        return self

    def _calc_pred_density(self, x):
        from scipy.stats import nbinom as ss_nbinom
        return ss_nbinom.pmf(x, n=self.p_r, p=(1.0 - self.p_theta))

    def make_prediction(self, loss="squared"):
        """Mean, mode, median or the negative-binomial predictive itself (ref:434-468)."""
        if loss == "squared":
            return self.p_r * self.p_theta / (1.0 - self.p_theta)
        if loss == "0-1":
            return np.floor((self.p_r - 1.0) * self.p_theta / (1.0 - self.p_theta)) if self.p_r > 1.0 else 0
        if loss == "abs" or loss == "KL":
            from scipy.stats import nbinom as ss_nbinom
            dist = ss_nbinom(n=self.p_r, p=(1.0 - self.p_theta))
            return dist if loss == "KL" else ss_nbinom.median(n=self.p_r, p=(1.0 - self.p_theta))
        raise CriteriaError(_LOSS_MSG)

    def pred_and_update(self, x, loss="squared"):
        """Predict, then fold the scalar x in: host only (ref:471-498)."""
        _check.nonneg_int(x, "x", DataFormatError)
        self.calc_pred_dist()
        prediction = self.make_prediction(loss=loss)
        self.update_posterior(x)
        return prediction

    def pred_and_update_sequence(self, x, loss="squared", *, code_length=False):
        """``[pred_and_update(x[i], loss) for i in range(n)]`` in one device pass (include/expseq.h): the exclusive prefix
        sums give ``p_r`` and ``p_theta`` of every position.  x is accepted and refused as ``update_posterior`` does it.
        Returns the float64 means ("squared") or modes ("0-1"), on the host the medians ("abs") or the frozen
        negative-binomial over the parameter arrays ("KL"); with ``code_length`` also ``nats[i] = -ln p(x[i] | x[:i])``;
        ``loss=None`` returns the nats alone and leaves ``p_r`` and ``p_theta``."""
        def predict(loss, params):
            p_r, p_theta = params
            if loss == "squared":
                return p_r * p_theta / (1.0 - p_theta)
            if loss == "0-1":
                xp = xs.xp_of(p_r)
                return xp.where(p_r > 1.0, xp.floor((p_r - 1.0) * p_theta / (1.0 - p_theta)), xp.zeros_like(p_r))
            from scipy.stats import nbinom as ss_nbinom
            p_r, p_theta = xs.host(p_r), xs.host(p_theta)
            dist = ss_nbinom(n=p_r, p=(1.0 - p_theta))
            return dist if loss == "KL" else ss_nbinom.median(n=p_r, p=(1.0 - p_theta))

        return xs.sequence(self, xs.POISSON, x, loss, code_length, ("squared", "0-1", "abs", "KL"), _LOSS_MSG,
                           lambda: self._sums(x, True), lambda st: self._fold(*st), (self.hn_alpha, self.hn_beta), predict)

    def calc_log_marginal_likelihood(self):
        from scipy.special import gammaln
        return (self.h0_alpha * np.log(self.h0_beta) - gammaln(self.h0_alpha) - self.hn_alpha * np.log(self.hn_beta)
                + gammaln(self.hn_alpha) - self._sum_log_factorial)

    def fit(self, x):
        self.reset_hn_params()
        self.update_posterior(x)
        return self

    def predict(self):
        self.calc_pred_dist()
        return self.make_prediction(loss="squared")
