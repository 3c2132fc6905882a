"""``exponential.GenModel`` / ``LearnModel``: drop-in for ``bayesml/exponential/_exponential.py`` (cited below as
``ref:<lines>``).

``update_posterior(x)`` of an array is one pass of ``expfam_stats_exponential`` over the sample where it lies: the count of
values for which ``x > 0`` is false (the reference's ``pos_floats`` check; NaN, 0 and -0.0 count) and the binary64 sum
(ref:296-313).  A scalar is folded in on the host.  Everything else is scalar host code.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _check, _expfam as xf, _expseq as xs, base
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError, ResultWarning

_LOSS_MSG = 'Unsupported loss function! This function supports "squared", "0-1", "abs", and "KL".'


class GenModel(base.Generative):
    """Data-generating model and its Gamma prior (ref:19-189; plotting is out of scope)."""

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
        self.lambda_ = self.rng.gamma(self.h_alpha, 1.0 / self.h_beta)
        return self

    def set_params(self, lambda_=None):
        if lambda_ is not None:
            self.lambda_ = _check.pos_float(lambda_, "lambda_", ParameterFormatError)
        return self

    def get_params(self):
        return {"lambda_": self.lambda_}

    def gen_sample(self, sample_size):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        return self.rng.exponential(1.0 / self.lambda_, sample_size)

    def save_sample(self, filename, sample_size):
        np.savez_compressed(filename, x=self.gen_sample(sample_size))

    def visualize_model(self, sample_size=100, hist_bins=10):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        _check.pos_int(hist_bins, "hist_bins", DataFormatError)
        self.gen_sample(sample_size)        # (the reference draws before it prints: the stream stays the same)
        print(f"lambda_:{self.lambda_}")
        raise NotImplementedError(xf.PLOT_MSG)


class LearnModel(xf.PassOwner, base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:192-546).  Positional parameters are the reference's; keyword-only
    ``device`` selects the GPU.  The sample may be a NumPy array or a torch tensor (integer samples are widened)."""

    def __init__(self, h0_alpha=1.0, h0_beta=1.0, *, device=None):
        self._init_pass(device)
        self.h0_alpha = 1.0
        self.h0_beta = 1.0
        self.hn_alpha = 1.0
        self.hn_beta = 1.0
        self.p_kappa = 1.0
        self.p_lambda = 1.0
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
        if hn_alpha is not None:
            self.hn_alpha = _check.pos_float(hn_alpha, "hn_alpha", ParameterFormatError)
        if hn_beta is not None:
            self.hn_beta = _check.pos_float(hn_beta, "hn_beta", ParameterFormatError)
        self.calc_pred_dist()
        return self

    def get_hn_params(self):
        return {"hn_alpha": self.hn_alpha, "hn_beta": self.hn_beta}

    def _sums(self, x, check):
        """(n, sum x) of a sample.  Arrays go through the device pass; with ``check`` a value that is not positive
        refuses the sample before anything is changed."""
        if not xf.is_array(x):
            if check:
                x = _check.pos_floats(x, "x", DataFormatError)
            return 1, x
        if check and _check.sample_kind(x) is None:
            raise DataFormatError("x" + _check.SAMPLE_MSG["pos_floats"])
        if xf.size_of(x) == 0:
            return 0, 0.0
        st = self._sample_stats(xf.EXPONENTIAL, x, "f")
        if check and st["bad"] > 0:
            raise DataFormatError("x" + _check.SAMPLE_MSG["pos_floats"])
        return st["n"] - st["bad"], st["sum"]

    def update_posterior(self, x):
        """hn_alpha += n, hn_beta += sum x (ref:299-313)."""
        n, s = self._sums(x, True)
        self.hn_alpha += n
        self.hn_beta += s
        return self

    def _update_posterior(self, x):
        """Update without input check (ref:315-319): values that are not positive are left out."""
        n, s = self._sums(x, False)
        self.hn_alpha += n
        self.hn_beta += s
        return self

    def estimate_params(self, loss="squared", dict_out=False):
        """Posterior mean, mode, median or the Gamma posterior itself (ref:321-369)."""
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
        from scipy.stats import gamma as ss_gamma
        _check.float_in_closed01(credibility, "credibility", CriteriaError)
        return ss_gamma.interval(credibility, a=self.hn_alpha, scale=1 / self.hn_beta)

    def visualize_posterior(self):
        raise NotImplementedError(xf.PLOT_MSG)

    def get_p_params(self):
        return {"p_kappa": self.p_kappa, "p_lambda": self.p_lambda}

    def calc_pred_dist(self):
        self.p_kappa = self.hn_alpha
        self.p_lambda = self.hn_beta
        return self

    def _calc_pred_density(self, x):
        from scipy.stats import lomax as ss_lomax
        return ss_lomax.pdf(x, c=self.p_kappa, scale=self.p_lambda)

    def make_prediction(self, loss="squared"):
        """Mean, mode, median or the Lomax predictive itself (ref:430-465)."""
        if loss == "squared":
            if self.p_kappa > 1:
                return self.p_lambda / (self.p_kappa - 1)
            warnings.warn("Mean doesn't exist for the current p_kappa.", ResultWarning)
            return None
        if loss == "0-1":
            return 0
        if loss == "abs":
            return self.p_lambda * (2.0 ** (1.0 / self.p_kappa) - 1)
        if loss == "KL":
            from scipy.stats import lomax as ss_lomax
            return ss_lomax(c=self.p_kappa, scale=self.p_lambda)
        raise CriteriaError(_LOSS_MSG)

    def pred_and_update(self, x, loss="squared"):
        """Predict, then fold the scalar x in: host only (ref:467-494)."""
        _check.pos_float(x, "x", DataFormatError)
        self.calc_pred_dist()
        prediction = self.make_prediction(loss=loss)
        self.update_posterior(x)
        return prediction

    def pred_and_update_sequence(self, x, loss="squared", *, code_length=False):
        """``[pred_and_update(x[i], loss) for i in range(n)]`` in one device pass (include/expseq.h): the exclusive prefix
        sums give ``p_kappa`` and ``p_lambda`` of every position.  x is accepted and refused as ``update_posterior`` does
        it.  Returns float64 means ("squared": NaN where ``p_kappa <= 1``, where the loop returns None, with one
        ``ResultWarning`` for the call), zeros ("0-1"), medians ("abs"), or on the host the frozen Lomax over the
        parameter arrays ("KL"); with ``code_length`` also ``nats[i] = -ln p(x[i] | x[:i])``; ``loss=None`` returns the
        nats alone and leaves ``p_kappa`` and ``p_lambda``."""
        def fold(st):
            self.hn_alpha += st[0]
            self.hn_beta += st[1]

        def predict(loss, params):
            p_kappa, p_lambda = params
            xp = xs.xp_of(p_kappa)
            if loss == "squared":
                none = ~(p_kappa > 1)
                if bool(none.any()):
                    warnings.warn("Mean doesn't exist for the current p_kappa.", ResultWarning)
                mean = p_lambda / xp.where(none, xp.ones_like(p_kappa), p_kappa - 1)
                return xp.where(none, xp.full_like(p_kappa, np.nan), mean)
            if loss == "0-1":
                return xp.zeros_like(p_kappa)
            if loss == "abs":
                return p_lambda * (2.0 ** (1.0 / p_kappa) - 1)
            from scipy.stats import lomax as ss_lomax
            return ss_lomax(c=xs.host(p_kappa), scale=xs.host(p_lambda))

        return xs.sequence(self, xs.EXPONENTIAL, x, loss, code_length, ("squared", "0-1", "abs", "KL"), _LOSS_MSG,
                           lambda: self._sums(x, True), fold, (self.hn_alpha, self.hn_beta), predict)

    def calc_log_marginal_likelihood(self):
        from scipy.special import gammaln
        return (self.h0_alpha * np.log(self.h0_beta) - gammaln(self.h0_alpha) - self.hn_alpha * np.log(self.hn_beta)
                + gammaln(self.hn_alpha))

    def fit(self, x):
        self.reset_hn_params()
        self.update_posterior(x)
        return self

    def predict(self):
        self.calc_pred_dist()
        return self.make_prediction(loss="squared")
