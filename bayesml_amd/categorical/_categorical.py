"""``categorical.GenModel`` / ``LearnModel``: drop-in for ``bayesml/categorical/_categorical.py`` (cited below as
``ref:<lines>``).

``update_posterior(x, onehot)`` of an array is one pass over the sample where it lies: ``expfam_stats_onehot`` checks every
row (no negative entry, sum 1) and forms the column sums (ref:329-333, 360); ``expfam_stats_counts`` checks every index
(0 <= x < c_degree), keeps the maximum and fills the histogram that the reference builds in a Python loop of
``count_nonzero`` over c_degree (ref:335-341, 362-363).  A single index is folded in on the host.  The Dirichlet closed
forms are c_degree-sized host NumPy as in the reference.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _check, _expfam as xf, _expseq as xs, base
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError, ResultWarning

_LOSS_MSG = 'Unsupported loss function! This function supports "squared", "0-1", and "KL".'


class GenModel(base.Generative):
    """Data-generating model and its Dirichlet prior (ref:25-232; plotting is out of scope)."""

    def __init__(self, c_degree, theta_vec=None, h_alpha_vec=None, seed=None):
        self.c_degree = _check.pos_int(c_degree, "c_degree", ParameterFormatError)
        self.rng = np.random.default_rng(seed)
        self.theta_vec = np.ones(self.c_degree) / self.c_degree
        self.h_alpha_vec = np.ones(self.c_degree) / 2.0
        self.set_params(theta_vec)
        self.set_h_params(h_alpha_vec)

    def get_constants(self):
        return {"c_degree": self.c_degree}

    def set_h_params(self, h_alpha_vec=None):
        if h_alpha_vec is not None:
            _check.pos_floats(h_alpha_vec, "h_alpha_vec", ParameterFormatError)
            self.h_alpha_vec[:] = h_alpha_vec
        return self

    def get_h_params(self):
        return {"h_alpha_vec": self.h_alpha_vec}

    def gen_params(self):
        self.theta_vec[:] = self.rng.dirichlet(self.h_alpha_vec)
        return self

    def set_params(self, theta_vec=None):
        if theta_vec is not None:
            _check.float_vec_sum_1(theta_vec, "theta_vec", ParameterFormatError)
            _check.shape_consistency(theta_vec.shape[0], "theta_vec.shape[0]", self.c_degree, "self.c_degree",
                                     ParameterFormatError)
            self.theta_vec[:] = theta_vec
        return self

    def get_params(self):
        return {"theta_vec": self.theta_vec}

    def gen_sample(self, sample_size, onehot=True):
        """Indices drawn by ``Generator.choice`` as in the reference (ref:146-151), one-hot encoded on request."""
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        x = self.rng.choice(self.c_degree, sample_size, p=self.theta_vec)
        return np.eye(self.c_degree, dtype=int)[x] if onehot else x

    def save_sample(self, filename, sample_size, onehot=True):
        np.savez_compressed(filename, x=self.gen_sample(sample_size, onehot))

    def visualize_model(self, sample_size=20, sample_num=5):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        _check.pos_int(sample_num, "sample_num", DataFormatError)
        print(f"theta_vec:{self.theta_vec}",)
        raise NotImplementedError(xf.PLOT_MSG)


class LearnModel(xf.PassOwner, base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:234-639).  Positional parameters are the reference's; keyword-only
    ``device`` selects the GPU.  ``c_degree`` is limited to ``_expfam.MAX_DEGREE`` (``EngineLimitError`` beyond)."""

    def __init__(self, c_degree, h0_alpha_vec=None, *, device=None):
        self.c_degree = _check.pos_int(c_degree, "c_degree", ParameterFormatError)
        xf.check_degree(self.c_degree, "categorical")
        self._init_pass(device)
        self.h0_alpha_vec = np.ones(self.c_degree) / 2.0
        self.hn_alpha_vec = np.ones(self.c_degree) / 2.0
        self.p_theta_vec = np.ones(self.c_degree) / self.c_degree
        self.set_h0_params(h0_alpha_vec)

    def get_constants(self):
        return {"c_degree": self.c_degree}

    def set_h0_params(self, h0_alpha_vec=None):
        if h0_alpha_vec is not None:
            _check.pos_floats(h0_alpha_vec, "h0_alpha_vec", ParameterFormatError)
            self.h0_alpha_vec[:] = h0_alpha_vec
        self.reset_hn_params()
        return self

    def get_h0_params(self):
        return {"h0_alpha_vec": self.h0_alpha_vec}

    def set_hn_params(self, hn_alpha_vec=None):
        if hn_alpha_vec is not None:
            _check.pos_floats(hn_alpha_vec, "hn_alpha_vec", ParameterFormatError)
            self.hn_alpha_vec[:] = hn_alpha_vec
        self.calc_pred_dist()
        return self

    def get_hn_params(self):
        return {"hn_alpha_vec": self.hn_alpha_vec}

    def _max_error(self, mx):
        return DataFormatError("np.max(x) must be smaller than self.c_degree: "
                               f"np.max(x) = {mx}, self.c_degree = {self.c_degree}")

    def _index_counts(self, x, check):
        """Histogram of an index sample over 0 .. c_degree-1 (ref:335-341 and the loop of ref:362-363)."""
        counts = np.zeros(self.c_degree, dtype=np.int64)
        if not xf.is_array(x):
            if check:
                _check.nonneg_ints(x, "x", DataFormatError)
                if x >= self.c_degree:
                    raise self._max_error(x)
            if 0 <= x < self.c_degree:
                counts[int(x)] = 1
            return counts
        if check and _check.sample_kind(x) != "i":
            raise DataFormatError("x" + _check.SAMPLE_MSG["nonneg_ints"])
        if xf.size_of(x) == 0:
            if check:
                np.max(np.zeros(0))          # the reference's np.max of an empty sample: ValueError
            return counts
        st = self._sample_stats(xf.COUNTS, x, "i", self.c_degree)
        if check and st["bad"] > 0:
            # (the reference looks for negative values first; a sample with both kinds of bad value gets the second message)
            if st["max"] >= self.c_degree:
                raise self._max_error(st["max"])
            raise DataFormatError("x" + _check.SAMPLE_MSG["nonneg_ints"])
        return st["counts"]

    def _onehot_counts(self, x):
        """Column sums of a one-hot sample [N, c_degree] or [c_degree] (ref:329-333, 360)."""
        if _check.sample_kind(x) != "i" or x.ndim < 1:
            raise DataFormatError("x" + _check.SAMPLE_MSG["onehot_vecs"])
        if x.shape[-1] != self.c_degree:
            if type(x) is np.ndarray:
                _check.onehot_vecs(x, "x", DataFormatError)      # the reference's order: the rows first, then the shape
            raise DataFormatError(f"x.shape[-1] must be c_degree:{self.c_degree}")
        if type(x) is np.ndarray and x.ndim == 1:      # one observation: host work, as a single index is
            return _check.onehot_vec(x, "x", lambda m: DataFormatError("x" + _check.SAMPLE_MSG["onehot_vecs"])).astype(np.int64)
        if xf.size_of(x) == 0:
            return np.zeros(self.c_degree, dtype=np.int64)
        st = self._sample_stats(xf.ONEHOT, x, "i", self.c_degree, cols=self.c_degree)
        if st["bad"] > 0:
            raise DataFormatError("x" + _check.SAMPLE_MSG["onehot_vecs"])
        return st["counts"]

    def update_posterior(self, x, onehot=True):
        """hn_alpha_vec += category counts (ref:343-364); a refused sample changes nothing."""
        self.hn_alpha_vec[:] += self._onehot_counts(x) if onehot else self._index_counts(x, True)
        return self

    def _update_posterior(self, x):
        """Update from indices without input check (ref:366-370): an index outside 0 .. c_degree-1 counts for nothing."""
        self.hn_alpha_vec[:] += self._index_counts(x, False)
        return self

    def estimate_params(self, loss="squared", dict_out=False):
        """Posterior mean, mode or the Dirichlet posterior itself (ref:372-420).  As in the reference the mode divides by
        ``sum(alpha) - c_degree``."""
        if loss == "squared":
            est = self.hn_alpha_vec / np.sum(self.hn_alpha_vec)
        elif loss == "0-1":
            if np.all(self.hn_alpha_vec > 1):
                est = (self.hn_alpha_vec - 1) / (np.sum(self.hn_alpha_vec) - self.c_degree)
            else:
                warnings.warn("MAP estimate of theta_vec doesn't exist for the current hn_alpha_vec.", ResultWarning)
                est = None
        elif loss == "KL":
            from scipy.stats import dirichlet as ss_dirichlet
            return ss_dirichlet(alpha=self.hn_alpha_vec)
        else:
            raise CriteriaError(_LOSS_MSG)
        return {"theta_vec": est} if dict_out else est

    def visualize_posterior(self):
        print(f"hn_alpha_vec:{self.hn_alpha_vec}")
        if self.c_degree not in (2, 3):
            raise ParameterFormatError("if c_degree != 2 or c_degree != 3, it is impossible to visualize the model by this function.")
        raise NotImplementedError(xf.PLOT_MSG)

    def get_p_params(self):
        return {"p_theta_vec": self.p_theta_vec}

    def calc_pred_dist(self):
        self.p_theta_vec[:] = self.hn_alpha_vec / self.hn_alpha_vec.sum()
        return self

    def _calc_pred_density(self, x):
        return self.p_theta_vec[x]

    def make_prediction(self, loss="squared", onehot=True):
        if loss == "squared" or loss == "KL":
            return self.p_theta_vec
        if loss == "0-1":
            if not onehot:
                return np.argmax(self.p_theta_vec)
            tmp = np.zeros(self.c_degree, dtype=int)
            tmp[np.argmax(self.p_theta_vec)] = 1
            return tmp
        raise CriteriaError(_LOSS_MSG)

    def pred_and_update(self, x, loss="squared", onehot=True):
        """Predict, then fold x in (ref:533-558): one index or one one-hot row, host work only."""
        self.calc_pred_dist()
        prediction = self.make_prediction(loss, onehot)
        self.update_posterior(x, onehot)
        return prediction

    def pred_and_update_sequence(self, x, loss="squared", onehot=True, *, code_length=False, chunk_bytes=None):
        """``[pred_and_update(x[i], loss, onehot) for i in range(n)]`` in one device pass (include/expseq.h), x[i] being
        the rows of a one-hot matrix or, with ``onehot=False``, indices.  x is accepted and refused as
        ``update_posterior(x, onehot)`` does it.  Returns float64 rows [n, c_degree] ("squared", "KL"), or for "0-1" the
        int64 one-hot rows of the first maximum (``onehot=False``: the int64 argmax [n]); with ``code_length`` also
        ``nats[i] = -ln p(x[i] | x[:i])``; ``loss=None`` returns the nats alone, forms no [n, c_degree] array anywhere and
        leaves ``p_theta_vec``.  The normaliser of position i is ``hn_alpha_vec.sum() + i``: it grows by exactly one per
        position.  The sample is taken in chunks whose scratch stays within ``chunk_bytes`` (default 256 MiB); the counts
        carried between chunks are integers, so the cut changes no bit."""
        import torch
        xs.check_sequence_loss(loss, code_length, ("squared", "0-1", "KL"), _LOSS_MSG)
        counts = self._onehot_counts(x) if onehot else self._index_counts(x, True)
        as_numpy = not isinstance(x, torch.Tensor)
        c = self.c_degree
        if not xf.is_array(x):
            x = np.asarray([x], dtype=np.int64)
        n = xf.size_of(x) // c if onehot else xf.size_of(x)
        want = {"squared": "rows", "KL": "rows", "0-1": "argmax", None: None}[loss]
        if n == 0:
            zeros = (lambda shape, dt: np.zeros(shape, dtype=getattr(np, dt))) if as_numpy else (
                lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device=xs.out_device(self, x)))
            pred = zeros((0, c), "float64") if want == "rows" else zeros((0,), "int64") if want == "argmax" else None
            nats = zeros((0,), "float64")
        else:
            eng = self._seq_pass()
            alpha0 = self.hn_alpha_vec.copy()
            xd = eng.adopt(x, "i", c) if onehot else eng.adopt(x, "i")
            pred, nats, _, _ = eng.run_categorical(xd, onehot, alpha0, want, bool(code_length), chunk_bytes)
            if want is not None:
                # the parameters of the last prediction, by the pass's own expression
                last = int(xd[-1].argmax()) if onehot else int(xd[-1])
                before = np.asarray(counts, dtype=np.int64).copy()
                before[last] -= 1
                self.p_theta_vec[:] = (alpha0 + before) / (alpha0.sum() + float(n - 1))
            self.hn_alpha_vec[:] += counts
            if as_numpy:
                pred, nats = (None if t is None else xs.host(t) for t in (pred, nats))
        if loss is None:
            return nats
        if loss == "0-1" and onehot:
            if isinstance(pred, torch.Tensor):
                pred = torch.zeros((n, c), dtype=torch.int64, device=pred.device).scatter_(1, pred[:, None], 1)
            else:
                am, pred = pred, np.zeros((n, c), dtype=np.int64)
                pred[np.arange(n), am] = 1
        return (pred, nats) if code_length else pred

    def calc_log_marginal_likelihood(self):
        from scipy.special import gammaln
        return (gammaln(self.h0_alpha_vec.sum()) - gammaln(self.h0_alpha_vec).sum()
                - gammaln(self.hn_alpha_vec.sum()) + gammaln(self.hn_alpha_vec).sum())

    def fit(self, x, onehot=True):
        self.reset_hn_params()
        self.update_posterior(x, onehot)
        return self

    def predict(self, onehot=True):
        self.calc_pred_dist()
        return self.make_prediction(loss="0-1", onehot=onehot)

    def predict_proba(self):
        self.calc_pred_dist()
        return self.make_prediction(loss="KL")
