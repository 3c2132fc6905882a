"""``linearregression.GenModel`` / ``LearnModel``: drop-in for ``bayesml/linearregression/_linearregression.py`` (cited
below as ``ref:<lines>``).

``update_posterior(x, y)`` needs x^T x, x^T y, y^T y and n - one pass over the rows (``regvb_stats``); ``calc_pred_dist(x)``
needs x_n . mu and x_n^T Lambda^-1 x_n per row (``regvb_predict``, from the inverse Cholesky factor of Lambda instead of the
reference's D x N solve).  Everything D-sized stays on the host in NumPy as in the reference (``_normalgamma``).  No CPU
fallback: without the library or a GPU both calls raise ``EngineUnavailableError``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _check, _normalgamma as ng, base
from .._exceptions import DataFormatError, ParameterFormatError

_D_NAME = "self.c_degree"
_GEN_PLOT_MSG = ("This function supports only the following cases: c_degree = 2 and constant = True; "
                 "c_degree = 1 and constant = False.")


class GenModel(base.Generative):
    """Data-generating model and its Normal-Gamma prior (ref:19-299; plotting is out of scope)."""

    def __init__(self, c_degree, theta_vec=None, tau=1.0, h_mu_vec=None, h_lambda_mat=None, h_alpha=1.0, h_beta=1.0,
                 seed=None):
        self.c_degree = _check.pos_int(c_degree, "c_degree", ParameterFormatError)
        self.rng = np.random.default_rng(seed)
        self.theta_vec = np.zeros(self.c_degree)
        self.tau = 1.0
        ng.init_params(self, ("h_",), self.c_degree)
        self.set_params(theta_vec, tau)
        self.set_h_params(h_mu_vec, h_lambda_mat, h_alpha, h_beta)

    def get_constants(self):
        return {"c_degree": self.c_degree}

    def set_h_params(self, h_mu_vec=None, h_lambda_mat=None, h_alpha=None, h_beta=None):
        ng.assign(self, "h_", self.c_degree, _D_NAME, h_mu_vec, h_lambda_mat, h_alpha, h_beta)
        return self

    def get_h_params(self):
        return {"h_mu_vec": self.h_mu_vec, "h_lambda_mat": self.h_lambda_mat, "h_alpha": self.h_alpha, "h_beta": self.h_beta}

    def gen_params(self):
        ng.gen_params(self)
        return self

    def set_params(self, theta_vec=None, tau=None):
        ng.assign_params(self, self.c_degree, _D_NAME, theta_vec, tau)
        return self

    def get_params(self):
        return {"theta_vec": self.theta_vec, "tau": self.tau}

    def gen_sample(self, sample_size=None, x=None, constant=True):
        """(x, y) with y_i ~ N(x_i . theta_vec, 1 / tau) (ref:201-217).  The noise is one array draw: ``Generator.normal``
        fills an array element by element from the same stream as the reference's per-row scalar calls."""
        if x is not None:
            _check.float_vecs(x, "x", DataFormatError)
            x = x.reshape([-1, self.c_degree])
            sample_size = x.shape[0]
        elif sample_size is not None:
            _check.pos_int(sample_size, "sample_size", DataFormatError)
            x = self.rng.multivariate_normal(np.zeros(self.c_degree), np.eye(self.c_degree), size=sample_size)
            if constant:
                x[:, -1] = 1.0
        else:
            raise DataFormatError("Either of the sample_size and the x must be given as an input.")
        y = self.rng.normal(loc=x @ self.theta_vec, scale=1.0 / np.sqrt(self.tau))
        return x, y

    def save_sample(self, filename, sample_size=None, x=None, constant=True):
        x, y = self.gen_sample(sample_size, x, constant)
        np.savez_compressed(filename, x=x, y=y)

    def visualize_model(self, sample_size=100, constant=True):
        if not ((self.c_degree == 2 and constant is True) or (self.c_degree == 1 and constant is False)):
            raise ParameterFormatError(_GEN_PLOT_MSG)
        if self.c_degree == 2:
            print(f"theta_vec:\n{self.theta_vec}")
            print(f"tau:\n{self.tau}")
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        raise NotImplementedError(ng.PLOT_MSG)


class LearnModel(base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:303-876).  Positional parameters are the reference's:
    ``c_degree, h0_mu_vec=None, h0_lambda_mat=None, h0_alpha=1.0, h0_beta=1.0``; keyword-only ``device`` selects the GPU.
    ``x`` / ``y`` may be NumPy arrays or torch tensors (a device tensor is used in place)."""

    def __init__(self, c_degree, h0_mu_vec=None, h0_lambda_mat=None, h0_alpha=1.0, h0_beta=1.0, *, device=None):
        self.c_degree = _check.pos_int(c_degree, "c_degree", ParameterFormatError)
        from .._regression import check_features
        check_features(self.c_degree, "linearregression")
        self._device = device
        self._engine = None
        self._reg_pass_factory = None        # test seam only (tests/fake_regression_engine.py)
        self._seq_engine = None
        self._regseq_pass_factory = None     # test seam only (tests/regression_seq_oracle.py)
        ng.init_params(self, ("h0_", "hn_"), self.c_degree)
        self._p = (np.zeros(1), np.ones(1))  # (p_ms, p_lambdas): ndarrays, or device tensors fetched on first read
        self.p_nus = np.full(1, 2.0)
        self._n = 0
        self.set_h0_params(h0_mu_vec, h0_lambda_mat, h0_alpha, h0_beta)

    # p_ms / p_lambdas are float64 ndarrays to the caller; after calc_pred_dist they live on the device until first read
    def _fetch(self):
        return ng.fetch(self)

    @property
    def p_ms(self):
        return self._fetch()[0]

    @property
    def p_lambdas(self):
        return self._fetch()[1]

    def __getstate__(self):
        self._fetch()
        state = dict(self.__dict__)
        state["_engine"] = state["_seq_engine"] = None
        return state

    def get_constants(self):
        return {"c_degree": self.c_degree}

    def set_h0_params(self, h0_mu_vec=None, h0_lambda_mat=None, h0_alpha=None, h0_beta=None):
        ng.assign(self, "h0_", self.c_degree, _D_NAME, h0_mu_vec, h0_lambda_mat, h0_alpha, h0_beta)
        self.reset_hn_params()
        return self

    def get_h0_params(self):
        return {"h0_mu_vec": self.h0_mu_vec, "h0_lambda_mat": self.h0_lambda_mat, "h0_alpha": self.h0_alpha,
                "h0_beta": self.h0_beta}

    def set_hn_params(self, hn_mu_vec=None, hn_lambda_mat=None, hn_alpha=None, hn_beta=None):
        self._n = 0
        ng.assign(self, "hn_", self.c_degree, _D_NAME, hn_mu_vec, hn_lambda_mat, hn_alpha, hn_beta)
        # the reference ends with calc_pred_dist(zeros) (ref:493): for the zero row that is exactly this, without a data pass
        self._p = (np.zeros(1), np.full(1, self.hn_alpha / self.hn_beta))
        self.p_nus = np.full(1, 2.0 * self.hn_alpha)
        return self

    def get_hn_params(self):
        return {"hn_mu_vec": self.hn_mu_vec, "hn_lambda_mat": self.hn_lambda_mat, "hn_alpha": self.hn_alpha,
                "hn_beta": self.hn_beta}

    # ------------------------------------------------------------------ validation (ref:509-526)
    def _check_sample_x(self, x):
        if isinstance(x, torch.Tensor):
            if not (x.dtype.is_floating_point and x.dim() >= 1):
                raise DataFormatError("x must be a numpy.ndarray whose ndim >= 1.")
        else:
            _check.float_vecs(x, "x", DataFormatError)
        if x.shape[-1] != self.c_degree:
            raise DataFormatError(f"x.shape[-1] must be c_degree:{self.c_degree}")
        return x.reshape(-1, self.c_degree)

    def _check_sample(self, x, y):
        rows = self._check_sample_x(x)
        if isinstance(y, torch.Tensor):
            if not y.dtype.is_floating_point:
                raise DataFormatError("y must be float or a numpy.ndarray.")
            if tuple(x.shape[:-1]) != tuple(y.shape):
                raise DataFormatError("x.shape[:-1] and y.shape must be same.")
            return rows, y.reshape(-1)
        y = _check.floats(y, "y", DataFormatError)
        if type(y) is np.ndarray:
            if tuple(x.shape[:-1]) != y.shape:
                raise DataFormatError("x.shape[:-1] and y.shape must be same.")
        elif tuple(x.shape[:-1]) != ():
            raise DataFormatError("If y is a scaler, x.shape[:-1] must be the empty tuple ().")
        return rows, np.ravel(y)

    # ------------------------------------------------------------------ the data passes
    def update_posterior(self, x, y):
        """Conjugate update (ref:539-550): the N-sized sums come from the GPU in one pass, the closed form is the
        reference's."""
        x, y = self._check_sample(x, y)
        if x.shape[0] == 0:          # no rows: nothing to add (the reference's sums are empty), and nothing to launch
            return self
        eng = ng.data_pass(self, self.c_degree)
        stats = eng.stats(eng.adopt(x), eng.adopt(y))
        self._n += ng.update(self, stats.detach().to("cpu").numpy(), self.c_degree)
        return self

    def estimate_params(self, loss="squared", dict_out=False):
        est = ng.estimate(self, loss, 0.0)
        if dict_out and loss != "KL":
            return {"theta_vec": est[0], "tau": est[1]}
        return est

    def visualize_posterior(self):
        if self.c_degree > 2:
            raise ParameterFormatError("if self.c_degree > 2, it is impossible to visualize posterior by this function.")
        raise NotImplementedError(ng.PLOT_MSG)

    def get_p_params(self):
        return {"p_ms": self.p_ms, "p_lambdas": self.p_lambdas, "p_nus": self.p_nus}

    def calc_pred_dist(self, x):
        """Student-t predictive parameters per row of x (ref:716-720)."""
        x = self._check_sample_x(x)
        eng = ng.data_pass(self, self.c_degree)
        self._p = tuple(eng.predict(eng.adopt(x), self.hn_mu_vec, ng.inverse_factor(self.hn_lambda_mat),
                                    self.hn_alpha / self.hn_beta))
        self.p_nus = np.ones(x.shape[0]) * 2.0 * self.hn_alpha
        return self

    def make_prediction(self, loss="squared"):
        return ng.student_t(loss, self.p_ms, self.p_lambdas, self.p_nus)

    def pred_and_update(self, x, y, loss="squared"):
        self.calc_pred_dist(x)
        prediction = self.make_prediction(loss=loss)
        self.update_posterior(x, y)
        return prediction

    def pred_and_update_sequence(self, x, y, loss="squared", *, code_length=False, chunk_bytes=None):
        """``[pred_and_update(x[i], y[i], loss) for i in range(n)]`` over the rows of ``update_posterior(x, y)``, in order, in
        one device pass (``_regseq.RegressionSeqPass``, DESIGN.md 4f "Sequential prediction"): prediction i is made from
        the posterior of the rows before i, then row i is learnt.

        ``x`` and ``y`` are accepted and refused as ``update_posterior`` does it (NumPy or torch, f32 or f64, a device
        tensor is read where it lies); a refused sample changes nothing.  The return is the float64 ``[n]`` predictive
        means for ``loss`` "squared", "0-1" and "abs" - a NumPy array for NumPy input, a tensor on the model's device
        otherwise - and the frozen ``scipy.stats.t`` over the n parameter arrays for "KL".  With ``code_length=True`` it
        is ``(prediction, nats)``, ``nats[i] = -ln p(y[i] | rows before i)`` float64 ``[n]``; ``loss=None`` needs
        ``code_length=True`` and returns ``nats`` alone.  Afterwards ``p_ms``, ``p_lambdas`` and ``p_nus`` hold the n
        sequential parameter arrays, and ``hn_*`` are bit for bit what ``update_posterior(x, y)`` leaves: they come from
        that very pass over the sample.  ``chunk_bytes`` bounds the workspace (default 256 MiB): the rows are cut into
        blocks, ``_regseq.plan_blocks(...)`` blocks go into one pass, and the cut does not change a bit of the result."""
        ng.check_sequence_loss(loss, code_length)
        as_numpy = not isinstance(x, torch.Tensor)
        x, y = self._check_sample(x, y)
        eng = ng.seq_pass(self, self.c_degree) if x.shape[0] > 0 else None
        xd, yd = (eng.adopt(x), eng.adopt(y)) if eng is not None else (x, y)
        return ng.pred_and_update_sequence(
            self, x.shape[0], lambda start: eng.run(xd, yd, start, bool(code_length), chunk_bytes),
            lambda: self.update_posterior(xd, yd), as_numpy, loss, code_length)

    def calc_log_marginal_likelihood(self):
        """ref:802-812."""
        from scipy.special import gammaln
        return (self.h0_alpha * np.log(self.h0_beta) - self.hn_alpha * np.log(self.hn_beta)
                + gammaln(self.hn_alpha) - gammaln(self.h0_alpha)
                + 0.5 * (np.linalg.slogdet(self.h0_lambda_mat)[1] - np.linalg.slogdet(self.hn_lambda_mat)[1]
                         - self._n * np.log(2 * np.pi)))

    def calc_pred_var(self):
        """ref:823-827."""
        indices = self.p_nus > 2
        var = np.empty(self.p_nus.shape[0])
        var[indices] = self.p_nus[indices] / self.p_lambdas[indices] / (self.p_nus[indices] - 2)
        var[~indices] = np.nan
        return var

    def fit(self, x, y):
        self.reset_hn_params()
        self.update_posterior(x, y)
        return self

    def predict(self, x):
        self.calc_pred_dist(x)
        return self.make_prediction(loss="squared")
