"""``autoregressive.GenModel`` / ``LearnModel``: drop-in for ``bayesml/autoregressive/_autoregressive.py`` (cited below
as ``ref:<lines>``).

``update_posterior(x, padding)`` is the Normal-Gamma update over the lag windows [1, x[t-p], ..., x[t-1]] -> x[t] of the
series.  The reference builds the [T, p+1] window matrix in a Python loop over T (ref:481-486); here ``regvb_stats_window``
forms the windows on the GPU, a batch at a time, and accumulates the same sums in one pass.  The single-vector predictive
and everything else (p+1)-sized is host NumPy as in the reference (``_normalgamma``).  No CPU fallback for the pass.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _check, _normalgamma as ng, base
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError

_D_NAME = "self.c_degree+1"


class GenModel(base.Generative):
    """Data-generating model and its Normal-Gamma prior (ref:16-261; plotting is out of scope)."""

    def __init__(self, c_degree, theta_vec=None, tau=1.0, h_mu_vec=None, h_lambda_mat=None, h_alpha=1.0, h_beta=1.0,
                 seed=None):
        self.c_degree = _check.nonneg_int(c_degree, "c_degree", ParameterFormatError)
        self.rng = np.random.default_rng(seed)
        self.theta_vec = np.zeros(self.c_degree + 1)
        self.tau = 1.0
        ng.init_params(self, ("h_",), self.c_degree + 1)
        self.set_params(theta_vec, tau)
        self.set_h_params(h_mu_vec, h_lambda_mat, h_alpha, h_beta)

    def get_constants(self):
        return {"c_degree": self.c_degree}

    def set_h_params(self, h_mu_vec=None, h_lambda_mat=None, h_alpha=None, h_beta=None):
        ng.assign(self, "h_", self.c_degree + 1, _D_NAME, h_mu_vec, h_lambda_mat, h_alpha, h_beta)
        return self

    def get_h_params(self):
        return {"h_mu_vec": self.h_mu_vec, "h_lambda_mat": self.h_lambda_mat, "h_alpha": self.h_alpha, "h_beta": self.h_beta}

    def gen_params(self):
        ng.gen_params(self)
        return self

    def set_params(self, theta_vec=None, tau=None):
        ng.assign_params(self, self.c_degree + 1, _D_NAME, theta_vec, tau)
        return self

    def get_params(self):
        return {"theta_vec": self.theta_vec, "tau": self.tau}

    def gen_sample(self, sample_length, initial_values=None):
        """The recursion x[n] ~ N(theta . [1, x[n-p..n-1]], 1 / tau) (ref:190-203): sequential by nature, one scalar draw
        per step in the reference's order."""
        _check.pos_int(sample_length, "sample_length", DataFormatError)
        p = self.c_degree
        x = np.zeros(sample_length + p)
        if initial_values is not None:
            _check.float_vec(initial_values, "initial_values", DataFormatError)
            if initial_values.shape != (p,):
                raise DataFormatError("initial_values must be a 1 dimensional float array whose size coincide with "
                                      "``self.c_degree``")
            x[:p] = initial_values
        w = np.ones(p + 1)
        scale = 1.0 / np.sqrt(self.tau)
        for n in range(p, sample_length + p):
            w[1:] = x[n - p:n]
            x[n] = self.rng.normal(loc=self.theta_vec @ w, scale=scale)
        return x[p:]

    def save_sample(self, filename, sample_length, initial_values=None):
        np.savez_compressed(filename, x=self.gen_sample(sample_length, initial_values))

    def visualize_model(self, sample_length=50, sample_num=5, initial_values=None):
        _check.pos_int(sample_length, "sample_length", DataFormatError)
        _check.pos_int(sample_num, "sample_num", DataFormatError)
        print(f"theta_vec:{self.theta_vec}")
        print(f"tau:{self.tau}")
        raise NotImplementedError(ng.PLOT_MSG)


class LearnModel(base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:263-698).  Positional parameters are the reference's:
    ``c_degree, h0_mu_vec=None, h0_lambda_mat=None, h0_alpha=1.0, h0_beta=1.0``; keyword-only ``device`` selects the GPU.
    The series may be a NumPy array or a 1-dimensional torch tensor (a device tensor is used in place)."""

    def __init__(self, c_degree, h0_mu_vec=None, h0_lambda_mat=None, h0_alpha=1.0, h0_beta=1.0, *, device=None):
        self.c_degree = _check.nonneg_int(c_degree, "c_degree", ParameterFormatError)
        from .._regression import check_features
        check_features(self.c_degree + 1, "autoregressive")
        self._device = device
        self._engine = None
        self._reg_pass_factory = None        # test seam only (tests/fake_regression_engine.py)
        self._seq_engine = None
        self._regseq_pass_factory = None     # test seam only (tests/regression_seq_oracle.py)
        ng.init_params(self, ("h0_", "hn_"), self.c_degree + 1)
        self.p_m = 0.0
        self.p_lambda = 0.5
        self.p_nu = 2.0
        # what pred_and_update_sequence leaves: (p_ms, p_lambdas) as ndarrays, or device tensors fetched on first read
        self._p = (np.zeros(1), np.full(1, 0.5))
        self.p_nus = np.full(1, 2.0)
        self.set_h0_params(h0_mu_vec, h0_lambda_mat, h0_alpha, h0_beta)

    @property
    def p_ms(self):
        return ng.fetch(self)[0]

    @property
    def p_lambdas(self):
        return ng.fetch(self)[1]

    def __getstate__(self):
        ng.fetch(self)
        state = dict(self.__dict__)
        state["_engine"] = state["_seq_engine"] = None
        return state

    def get_constants(self):
        return {"c_degree": self.c_degree}

    def set_h0_params(self, h0_mu_vec=None, h0_lambda_mat=None, h0_alpha=None, h0_beta=None):
        ng.assign(self, "h0_", self.c_degree + 1, _D_NAME, h0_mu_vec, h0_lambda_mat, h0_alpha, h0_beta)
        self.reset_hn_params()
        return self

    def get_h0_params(self):
        return {"h0_mu_vec": self.h0_mu_vec, "h0_lambda_mat": self.h0_lambda_mat, "h0_alpha": self.h0_alpha,
                "h0_beta": self.h0_beta}

    def get_hn_params(self):
        return {"hn_mu_vec": self.hn_mu_vec, "hn_lambda_mat": self.hn_lambda_mat, "hn_alpha": self.hn_alpha,
                "hn_beta": self.hn_beta}

    def set_hn_params(self, hn_mu_vec=None, hn_lambda_mat=None, hn_alpha=None, hn_beta=None):
        ng.assign(self, "hn_", self.c_degree + 1, _D_NAME, hn_mu_vec, hn_lambda_mat, hn_alpha, hn_beta)
        self.calc_pred_dist(np.zeros(self.c_degree))
        return self

    def _check_series(self, x):
        if isinstance(x, torch.Tensor):
            if not (x.dtype.is_floating_point and x.dim() == 1):
                raise DataFormatError("x must be a 1-dimensional numpy.ndarray.")
        else:
            _check.float_vec(x, "x", DataFormatError)
        if x.shape[0] <= self.c_degree:
            raise DataFormatError("The length of x must greater than self.c_degree")

    def update_posterior(self, x, padding=None):
        """Conjugate update over the lag windows (ref:477-504).  As in the reference, any ``padding`` other than
        ``"zeros"`` means none: the first ``c_degree`` values only serve as initial values."""
        self._check_series(x)
        from .._regression import PAD_NONE, PAD_ZEROS
        eng = ng.data_pass(self, self.c_degree + 1)
        stats = eng.stats_window(eng.adopt(x), PAD_ZEROS if padding == "zeros" else PAD_NONE)
        ng.update(self, stats.detach().to("cpu").numpy(), self.c_degree + 1)
        return self

    def estimate_params(self, loss="squared"):
        return ng.estimate(self, loss, 0)

    def visualize_posterior(self):
        if self.c_degree != 1:
            raise ParameterFormatError("if self.c_degree != 1, it is impossible to visualize posterior by this function.")
        raise NotImplementedError(ng.PLOT_MSG)

    def get_p_params(self):
        return {"p_m": self.p_m, "p_lambda": self.p_lambda, "p_nu": self.p_nu}

    def calc_pred_dist(self, x):
        """Student-t predictive parameters of the next value after the c_degree values x (ref:617-625): (p+1)-sized host
        work."""
        _check.float_vec(x, "x", DataFormatError)
        if x.shape != (self.c_degree,):
            raise DataFormatError("x must be a 1 dimensional float array whose size coincide with ``self.c_degree``")
        w = np.ones(self.c_degree + 1)
        w[1:] = x
        self.p_m = self.hn_mu_vec @ w
        self.p_lambda = self.hn_alpha / self.hn_beta / (1.0 + w @ np.linalg.solve(self.hn_lambda_mat, w))
        self.p_nu = 2.0 * self.hn_alpha
        return self

    def make_prediction(self, loss="squared"):
        return ng.student_t(loss, self.p_m, self.p_lambda, self.p_nu)

    def predict_interval(self, credibility=0.95):
        """Credible interval of the prediction (ref:669-670).  The reference passes ``alpha=`` to
        ``scipy.stats.t.interval``, which SciPy >= 1.11 rejects; the level goes positionally here."""
        from scipy.stats import t
        _check.float_in_closed01(credibility, "credibility", CriteriaError)
        return t.interval(credibility, loc=self.p_m, scale=1.0 / np.sqrt(self.p_lambda), df=self.p_nu)

    def pred_and_update(self, x, loss="squared"):
        """Predict x[-1] from x[:-1], then fold it in (ref:692-698).  Like the reference this hands the p+1 values to
        ``update_posterior`` without padding: one window, one row."""
        _check.float_vec(x, "x", DataFormatError)
        if x.shape != (self.c_degree + 1,):
            raise DataFormatError("x must be a 1 dimensional float array whose size coincide with ``self.c_degree + 1``")
        self.calc_pred_dist(x[:self.c_degree])
        prediction = self.make_prediction(loss=loss)
        self.update_posterior(x)
        return prediction

    def pred_and_update_sequence(self, x, padding=None, loss="squared", *, code_length=False, chunk_bytes=None):
        """One-step-ahead prediction over the rows of ``update_posterior(x, padding)``, in order, in one device pass
        (``_regseq.RegressionSeqPass``, DESIGN.md 4f "Sequential prediction"): value x[t] is predicted from its lag window
        and the posterior of the windows before it, then learnt - ``pred_and_update(x[t - c_degree:t + 1], loss)`` for
        t = c_degree .. len(x) - 1, or for every t with zeros at negative times when ``padding == "zeros"``.

        ``x`` is accepted and refused as ``update_posterior`` does it (NumPy or torch, f32 or f64, a device tensor is read
        where it lies); a refused sample changes nothing.  The return is the float64 ``[n]`` predictive means for ``loss``
        "squared", "0-1" and "abs" - a NumPy array for NumPy input, a tensor on the model's device otherwise - and the
        frozen ``scipy.stats.t`` over the n parameter arrays for "KL".  With ``code_length=True`` it is
        ``(prediction, nats)``, ``nats[i] = -ln p(x[t_i] | earlier values)`` float64 ``[n]``; ``loss=None`` needs
        ``code_length=True`` and returns ``nats`` alone.  Afterwards ``p_ms``, ``p_lambdas`` and ``p_nus`` hold the n
        sequential parameter arrays, ``p_m``, ``p_lambda`` and ``p_nu`` the last position's, and ``hn_*`` are bit for bit
        what ``update_posterior(x, padding)`` leaves: they come from that very pass over the series.  ``chunk_bytes``
        bounds the workspace (default 256 MiB): the rows are cut into blocks, ``_regseq.plan_blocks(...)`` blocks go into
        one pass, and the cut does not change a bit of the result."""
        ng.check_sequence_loss(loss, code_length)
        self._check_series(x)
        from .._regression import PAD_NONE, PAD_ZEROS
        as_numpy = not isinstance(x, torch.Tensor)
        pad = PAD_ZEROS if padding == "zeros" else PAD_NONE
        eng = ng.seq_pass(self, self.c_degree + 1)
        xd = eng.adopt(x)
        n = x.shape[0] - (0 if pad == PAD_ZEROS else self.c_degree)
        out = ng.pred_and_update_sequence(
            self, n, lambda start: eng.run_window(xd, pad, start, bool(code_length), chunk_bytes),
            lambda: self.update_posterior(xd, padding), as_numpy, loss, code_length)
        self.p_m, self.p_lambda = (np.float64(float(t[-1])) for t in self._p)
        self.p_nu = float(self.p_nus[-1])
        return out
