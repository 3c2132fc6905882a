#!/usr/bin/env python3
"""Golden fixtures for the five scalar conjugate models (bernoulli, categorical, poisson, exponential, normal), produced
by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_expfam.py

writes tests/golden/expfam_*.npz (one per case of tests/expfam_oracle.py: CASES) and expfam_errors.json.  A sample of more
than a few thousand values is not stored: the fixture keeps a checksum of what the seeded recipe made.

Long-double audit.  Every case is walked twice by the same driver (expfam_oracle.drive): once through the reference as it
is, once through the reference with its sums over the sample, its posterior update and its log marginal likelihood
evaluated in long double (the subclasses below; lgamma in long double is libm's lgammal).  Quantities SciPy evaluates
(medians, intervals, moments of the frozen distributions) have no long-double form: there the second walk hands SciPy the
long-double hyperparameters rounded once to binary64, so the difference is what the reference's own rounding of hn_* does
to them.  Per quantity the fixture stores err = |reference - long double| / |long double| and
tol = max(8 * err, 32 eps): both the reference and the engine are binary64 sums of the same terms in a different order,
and 32 eps is the allowance for reassociating positive sums of this length.  The tests read tol from the fixture.
"""
import ctypes
import ctypes.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import bernoulli, categorical, exponential, normal, poisson          # noqa: E402
import expfam_oracle as orc                                                      # noqa: E402

LD = np.longdouble
REF = {"bernoulli": bernoulli, "categorical": categorical, "poisson": poisson, "exponential": exponential, "normal": normal}

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.lgammal.restype = ctypes.c_longdouble
_libm.lgammal.argtypes = [ctypes.c_longdouble]


def lgammal(v):
    """lgamma in long double, element-wise (arrays go through their unique values)."""
    a = np.atleast_1d(np.asarray(v, dtype=LD))
    u, inv = np.unique(a, return_inverse=True)
    lg = np.array([_libm.lgammal(ctypes.c_longdouble(e)) for e in u], dtype=LD)
    r = lg[inv].reshape(a.shape)
    return r if np.ndim(v) else r[0]


def ld_sum(a):
    return np.sum(np.asarray(a).astype(LD))


def _f64(v):
    return np.float64(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)


class _F64Scipy:
    """The reference's SciPy calls cannot take long double: hand them hn_* rounded once to binary64."""

    def _with_f64(self, names, fn):
        saved = {k: getattr(self, k) for k in names}
        for k, v in saved.items():
            setattr(self, k, _f64(v))
        try:
            return fn()
        finally:
            for k, v in saved.items():
                setattr(self, k, v)


class LdBernoulli(bernoulli.LearnModel, _F64Scipy):
    def set_h0_params(self, h0_alpha=None, h0_beta=None):
        return super().set_h0_params(None if h0_alpha is None else LD(h0_alpha), None if h0_beta is None else LD(h0_beta))

    def estimate_params(self, loss="squared", dict_out=False):
        if loss in ("abs", "KL"):
            return self._with_f64(("hn_alpha", "hn_beta"), lambda: super(LdBernoulli, self).estimate_params(loss, dict_out))
        return super().estimate_params(loss, dict_out)

    def estimate_interval(self, credibility=0.95):
        return self._with_f64(("hn_alpha", "hn_beta"), lambda: super(LdBernoulli, self).estimate_interval(credibility))

    def calc_log_marginal_likelihood(self):
        return (lgammal(self.h0_alpha + self.h0_beta) - lgammal(self.h0_alpha) - lgammal(self.h0_beta)
                - lgammal(self.hn_alpha + self.hn_beta) + lgammal(self.hn_alpha) + lgammal(self.hn_beta))


class LdCategorical(categorical.LearnModel, _F64Scipy):
    def __init__(self, c_degree, h0_alpha_vec=None):
        super().__init__(c_degree, h0_alpha_vec)
        for k in ("h0_alpha_vec", "hn_alpha_vec", "p_theta_vec"):
            setattr(self, k, getattr(self, k).astype(LD))
        self.reset_hn_params()

    def estimate_params(self, loss="squared", dict_out=False):
        if loss == "KL":
            return self._with_f64(("hn_alpha_vec",), lambda: super(LdCategorical, self).estimate_params(loss, dict_out))
        return super().estimate_params(loss, dict_out)

    def calc_log_marginal_likelihood(self):
        return (lgammal(self.h0_alpha_vec.sum()) - lgammal(self.h0_alpha_vec).sum()
                - lgammal(self.hn_alpha_vec.sum()) + lgammal(self.hn_alpha_vec).sum())


class LdPoisson(poisson.LearnModel, _F64Scipy):
    def set_h0_params(self, h0_alpha=None, h0_beta=None):
        return super().set_h0_params(None if h0_alpha is None else LD(h0_alpha), None if h0_beta is None else LD(h0_beta))

    def set_hn_params(self, hn_alpha=None, hn_beta=None):
        super().set_hn_params(hn_alpha, hn_beta)
        self._sum_log_factorial = LD(0)
        return self

    def update_posterior(self, x):
        x = self._check_sample(x)
        self.hn_alpha += ld_sum(x)
        self.hn_beta += np.size(x)
        self._sum_log_factorial += np.sum(lgammal(np.asarray(x).astype(LD) + 1))
        return self

    def estimate_params(self, loss="squared", dict_out=False):
        if loss in ("abs", "KL"):
            return self._with_f64(("hn_alpha", "hn_beta"), lambda: super(LdPoisson, self).estimate_params(loss, dict_out))
        return super().estimate_params(loss, dict_out)

    def estimate_interval(self, credibility=0.95):
        return self._with_f64(("hn_alpha", "hn_beta"), lambda: super(LdPoisson, self).estimate_interval(credibility))

    def make_prediction(self, loss="squared"):
        if loss in ("abs", "KL"):
            return self._with_f64(("p_r", "p_theta"), lambda: super(LdPoisson, self).make_prediction(loss))
        return super().make_prediction(loss)

    def calc_log_marginal_likelihood(self):
        return (self.h0_alpha * np.log(self.h0_beta) - lgammal(self.h0_alpha) - self.hn_alpha * np.log(self.hn_beta)
                + lgammal(self.hn_alpha) - self._sum_log_factorial)


class LdExponential(exponential.LearnModel, _F64Scipy):
    def set_h0_params(self, h0_alpha=None, h0_beta=None):
        return super().set_h0_params(None if h0_alpha is None else LD(h0_alpha), None if h0_beta is None else LD(h0_beta))

    def update_posterior(self, x):
        x = self._check_sample(x)
        self.hn_alpha += np.size(x)
        self.hn_beta += ld_sum(x)
        return self

    def estimate_params(self, loss="squared", dict_out=False):
        if loss in ("abs", "KL"):
            return self._with_f64(("hn_alpha", "hn_beta"), lambda: super(LdExponential, self).estimate_params(loss, dict_out))
        return super().estimate_params(loss, dict_out)

    def estimate_interval(self, credibility=0.95):
        return self._with_f64(("hn_alpha", "hn_beta"), lambda: super(LdExponential, self).estimate_interval(credibility))

    def make_prediction(self, loss="squared"):
        if loss == "KL":
            return self._with_f64(("p_kappa", "p_lambda"), lambda: super(LdExponential, self).make_prediction(loss))
        if loss == "abs":
            return self.p_lambda * (LD(2) ** (1 / self.p_kappa) - 1)
        return super().make_prediction(loss)

    def calc_log_marginal_likelihood(self):
        return (self.h0_alpha * np.log(self.h0_beta) - lgammal(self.h0_alpha) - self.hn_alpha * np.log(self.hn_beta)
                + lgammal(self.hn_alpha))


class LdNormal(normal.LearnModel, _F64Scipy):
    _HN = ("hn_m", "hn_kappa", "hn_alpha", "hn_beta")

    def set_h0_params(self, h0_m=None, h0_kappa=None, h0_alpha=None, h0_beta=None):
        return super().set_h0_params(*[None if v is None else LD(v) for v in (h0_m, h0_kappa, h0_alpha, h0_beta)])

    def update_posterior(self, x):
        x = np.asarray(self._check_sample(x)).astype(LD)
        n = x.size
        x_bar = np.sum(x) / n
        self.hn_beta += (np.sum((x - x_bar) ** 2) + n * self.hn_kappa / (self.hn_kappa + n) * (x_bar - self.hn_m) ** 2) / 2
        self.hn_m = (self.hn_kappa * self.hn_m + n * x_bar) / (self.hn_kappa + n)
        self.hn_kappa += n
        self.hn_alpha += LD(n) / 2
        self._n += n
        return self

    def estimate_params(self, loss="squared", dict_out=False):
        if loss in ("abs", "KL"):
            return self._with_f64(self._HN, lambda: super(LdNormal, self).estimate_params(loss, dict_out))
        return super().estimate_params(loss, dict_out)

    def estimate_interval(self, credibility=0.95):
        return self._with_f64(self._HN, lambda: super(LdNormal, self).estimate_interval(credibility))

    def make_prediction(self, loss="squared"):
        if loss == "KL":
            return self._with_f64(("p_mu", "p_lambda", "p_nu"), lambda: super(LdNormal, self).make_prediction(loss))
        return super().make_prediction(loss)

    def calc_log_marginal_likelihood(self):
        return (self.h0_alpha * np.log(self.h0_beta) - self.hn_alpha * np.log(self.hn_beta) + lgammal(self.hn_alpha)
                - lgammal(self.h0_alpha)
                + (np.log(self.h0_kappa) - np.log(self.hn_kappa) - self._n * np.log(2 * LD(np.pi))) / 2)


class _Pkg:
    def __init__(self, learn):
        self.LearnModel = learn


LDM = {"bernoulli": _Pkg(LdBernoulli), "categorical": _Pkg(LdCategorical), "poisson": _Pkg(LdPoisson),
       "exponential": _Pkg(LdExponential), "normal": _Pkg(LdNormal)}


def make_case(name):
    family, ctor, prior, ukw, recipes = orc.CASES[name]
    out = {}
    if recipes is None:
        bs = orc.gen_batches(REF[family], name)
        out.update(x0=bs[0], x1=bs[1])
    else:
        bs = [orc.make(r) for r in recipes]
        for i, b in enumerate(bs):
            assert b.size <= 400000
            out[f"checksum{i}"] = np.int64(orc.checksum(b))
    ref = orc.drive(REF[family], name, bs, to_input=orc.widen)
    exact = orc.drive(LDM[family], name, bs, to_input=orc.widen, as_array=lambda v: np.asarray(v, dtype=LD), lenient=True)
    worst = {}
    for k, v in ref.items():
        out[k] = v
        if not orc.is_number_key(k):
            assert exact[k] == v, (name, k)
            continue
        err = orc.rel_err(v, exact[k]) if k in exact else 0.0
        assert np.isfinite(err), (name, k, v, exact.get(k))
        out["err__" + k] = np.float64(err)
        out["tol__" + k] = np.float64(max(8.0 * err, 32.0 * orc.EPS))
        worst[k] = err
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"  {name}: reference vs long double, worst: " + ", ".join(f"{k} {v:.1e}" for k, v in top))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", name, os.path.getsize(path), "bytes")


def run_errors():
    res = {}
    for name, fn in orc.error_cases(REF).items():
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fn()
            res[name] = None
        except Exception as e:      # noqa: BLE001
            res[name] = type(e).__name__
    with open(os.path.join(HERE, "expfam_errors.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(res)


if __name__ == "__main__":
    for case in orc.CASES:
        make_case(case)
    run_errors()
