"""``bernoulli.GenModel`` / ``LearnModel``: drop-in for ``bayesml/bernoulli/_bernoulli.py`` (cited below as ``ref:<lines>``).

``update_posterior(x)`` of an array is one pass of ``expfam_stats_bernoulli`` over the sample where it lies: it counts the
ones, the zeros and the values that are neither (the reference's ``ints_of_01`` check and its two ``count_nonzero`` passes,
ref:296-310).  A scalar is folded in on the host.  Everything else is scalar host code as in the reference.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _check, _expfam as xf, _expseq as xs, base
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError, ResultWarning

_LOSS_MSG = 'Unsupported loss function! This function supports "squared", "0-1", "abs", and "KL".'


class GenModel(base.Generative):
    """Data-generating model and its Beta prior (ref:15-193; plotting is out of scope)."""

    def __init__(self, theta=0.5, h_alpha=0.5, h_beta=0.5, seed=None):
        self.rng = np.random.default_rng(seed)
        self.theta = 0.5
        self.h_alpha = 0.5
        self.h_beta = 0.5
        self.set_params(theta)
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
        self.theta = self.rng.beta(self.h_alpha, self.h_beta)
        return self

    def set_params(self, theta=None):
        if theta is not None:
            self.theta = _check.float_in_closed01(theta, "theta", ParameterFormatError)
        return self

    def get_params(self):
        return {"theta": self.theta}

    def gen_sample(self, sample_size):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        return self.rng.binomial(1, self.theta, sample_size)

    def save_sample(self, filename, sample_size):
        np.savez_compressed(filename, x=self.gen_sample(sample_size))

    def visualize_model(self, sample_size=20, sample_num=5):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        _check.pos_int(sample_num, "sample_num", DataFormatError)
        print(f"theta:{self.theta}")
        raise NotImplementedError(xf.PLOT_MSG)


class LearnModel(xf.PassOwner, base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:195-558).  Positional parameters are the reference's; keyword-only
    ``device`` selects the GPU.  The sample may be a NumPy array or a torch tensor of an integer dtype (a device tensor
    is used in place)."""

    def __init__(self, h0_alpha=0.5, h0_beta=0.5, *, device=None):
        self._init_pass(device)
        self.h0_alpha = 0.5
        self.h0_beta = 0.5
        self.hn_alpha = 0.5
        self.hn_beta = 0.5
        self.p_theta = 0.5
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

    def _counts(self, x, check):
        """(ones, zeros) of a sample.  Arrays go through the device pass; with ``check`` a value outside {0, 1} refuses
        the sample before anything is changed."""
        if not xf.is_array(x):
            if check:
                _check.int_of_01(x, "x", DataFormatError)
            return int(x == 1), int(x == 0)
        if check and _check.sample_kind(x) != "i":
            raise DataFormatError("x" + _check.SAMPLE_MSG["ints_of_01"])
        if xf.size_of(x) == 0:
            return 0, 0
        st = self._sample_stats(xf.BERNOULLI, x, "i")
        if check and st["bad"] > 0:
            raise DataFormatError("x" + _check.SAMPLE_MSG["ints_of_01"])
        return st["n1"], st["n0"]

    def update_posterior(self, x):
        """hn_alpha += #ones, hn_beta += #zeros (ref:299-310)."""
        n1, n0 = self._counts(x, True)
        self.hn_alpha += n1
        self.hn_beta += n0
        return self

    def _update_posterior(self, x):
        """Update without input check (ref:312-316): values that are neither 0 nor 1 count for nothing."""
        n1, n0 = self._counts(x, False)
        self.hn_alpha += n1
        self.hn_beta += n0
        return self

    def estimate_params(self, loss="squared", dict_out=False):
        """Posterior mean, mode, median or the Beta posterior itself (ref:318-377)."""
        a, b = self.hn_alpha, self.hn_beta
        if loss == "squared":
            est = a / (a + b)
        elif loss == "0-1":
            if a > 1.0 and b > 1.0:
                est = (a - 1.0) / (a + b - 2.0)
            elif a > 1.0:
                est = 1.0
            elif b > 1.0:
                est = 0.0
            else:
                warnings.warn("MAP estimate doesn't exist for the current hn_alpha and hn_beta.", ResultWarning)
                est = None
        elif loss == "abs":
            from scipy.stats import beta as ss_beta
            est = ss_beta.median(a, b)
        elif loss == "KL":
            from scipy.stats import beta as ss_beta
            return ss_beta(a, b)
        else:
            raise CriteriaError(_LOSS_MSG)
        return {"theta": est} if dict_out else est

    def estimate_interval(self, credibility=0.95):
        from scipy.stats import beta as ss_beta
        _check.float_in_closed01(credibility, "credibility", CriteriaError)
        return ss_beta.interval(credibility, self.hn_alpha, self.hn_beta)

    def visualize_posterior(self):
        raise NotImplementedError(xf.PLOT_MSG)

    def get_p_params(self):
        return {"p_theta": self.p_theta}

    def calc_pred_dist(self):
        self.p_theta = self.hn_alpha / (self.hn_alpha + self.hn_beta)
        return self

    def _calc_pred_density(self, x):
        return np.where(x == 1, self.p_theta, 1.0 - self.p_theta)

    def make_prediction(self, loss="squared"):
        if loss == "squared":
            return self.p_theta
        if loss == "0-1" or loss == "abs":
            return 1 if self.p_theta > 0.5 else 0
        if loss == "KL":
            return np.array((1.0 - self.p_theta, self.p_theta))
        raise CriteriaError(_LOSS_MSG)

    def pred_and_update(self, x, loss="squared"):
        """Predict, then fold the scalar x in: host only (ref:466-488)."""
        _check.int_of_01(x, "x", DataFormatError)
        self.calc_pred_dist()
        prediction = self.make_prediction(loss=loss)
        self.update_posterior(x)
        return prediction

    def pred_and_update_sequence(self, x, loss="squared", *, code_length=False):
        """``[pred_and_update(x[i], loss) for i in range(n)]`` in one device pass (include/expseq.h): the exclusive prefix
        counts of ones and zeros give ``p_theta`` of every position.  x is accepted and refused as ``update_posterior``
        does it.  Returns float64 ``p_theta`` ("squared"), int64 ``p_theta > 0.5`` ("0-1", "abs") or float64 [n, 2]
        ("KL"); with ``code_length`` also ``nats[i] = -ln p(x[i] | x[:i])``; ``loss=None`` returns the nats alone and
        leaves ``p_theta``.  NumPy in, NumPy out; a tensor in, tensors on the device out."""
        def fold(st):
            self.hn_alpha += st[0]
            self.hn_beta += st[1]

        def predict(loss, params):
            p_theta, = params
            if loss == "squared":
                return p_theta
            if loss == "KL":
                return xs.xp_of(p_theta).stack((1.0 - p_theta, p_theta), 1)
            return xs.as_int64(p_theta > 0.5)

        return xs.sequence(self, xs.BERNOULLI, x, loss, code_length, ("squared", "0-1", "abs", "KL"), _LOSS_MSG,
                           lambda: self._counts(x, True), fold, (self.hn_alpha, self.hn_beta), predict)

    def calc_log_marginal_likelihood(self):
        from scipy.special import gammaln
        return (gammaln(self.h0_alpha + self.h0_beta) - gammaln(self.h0_alpha) - gammaln(self.h0_beta)
                - gammaln(self.hn_alpha + self.hn_beta) + gammaln(self.hn_alpha) + gammaln(self.hn_beta))

    def fit(self, x):
        self.reset_hn_params()
        self.update_posterior(x)
        return self

    def predict(self):
        self.calc_pred_dist()
        return self.make_prediction(loss="0-1")

    def predict_proba(self):
        self.calc_pred_dist()
        return self.make_prediction(loss="KL")
