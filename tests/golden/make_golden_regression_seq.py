#!/usr/bin/env python3
"""Golden fixtures for ``pred_and_update_sequence`` of linearregression / autoregressive, produced by the REFERENCE's own
loops (build container only; the path of a bayesml v0.3.1 checkout is the argument):

    MPLBACKEND=Agg python tests/golden/make_golden_regression_seq.py <path to the reference>

linearregression: ``calc_pred_dist`` then ``update_posterior`` per row; autoregressive: ``pred_and_update`` per window.
Cases: D in {1, 3, 17} and p in {0, 1, 4}, n = 150 rows, each from the default prior, from a diffuse prior
(Lambda_0 = 1e-6 I) and from the posterior a first ``update_posterior`` leaves on a given prior.  The state at the first row is
stored (``start_*``: tests set it with ``set_hn_params``), so every implementation starts from the same bits.  Stored per
case: the inputs, the reference's three parameter traces and the code lengths they imply (scipy's Student-t), the final
``hn_*``, the traces of the same loop in long double (tests/regression_seq_oracle.py: ld_row_loop), and ``ref_vs_exact``:
the reference's error against them per output (oracle ``errors``), separately for the first 2 D rows and for the rest.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import autoregressive as ref_ar            # noqa: E402
from bayesml import linearregression as ref_lr          # noqa: E402
import regression_oracle as orc                         # noqa: E402
import regression_seq_oracle as seq                     # noqa: E402

N = 150
N_FIRST = 40


def priors(D, rng):
    a = rng.standard_normal((D, D))
    return {"default": {}, "diffuse": dict(h0_lambda_mat=np.eye(D) * 1e-6),
            "posterior": dict(h0_mu_vec=rng.standard_normal(D) * 0.3, h0_lambda_mat=np.eye(D) * 2.0 + a @ a.T / D,
                              h0_alpha=2.5, h0_beta=0.75)}


def finish(name, m, out, traces, w, y, D):
    from scipy.stats import t as student
    start = (out["start_mu_vec"], out["start_lambda_mat"], out["start_alpha"], out["start_beta"])
    ref = [np.array(t, dtype=np.float64) for t in traces]
    ref.append(-student.logpdf(y, loc=ref[0], scale=1.0 / np.sqrt(ref[1]), df=ref[2]))
    exact = seq.ld_row_loop(w, y, *start)
    out.update(hn_mu_vec=m.hn_mu_vec.copy(), hn_lambda_mat=m.hn_lambda_mat.copy(), hn_alpha=float(m.hn_alpha),
               hn_beta=float(m.hn_beta))
    for k, r, e in zip(seq.NAMES, ref, exact):
        out["ref_" + k] = r
        out["exact_" + k] = np.asarray(e, dtype=np.longdouble)
    for part, rows in (("head", slice(0, 2 * D)), ("rest", slice(2 * D, None))):
        err = seq.errors(ref, exact, y, rows)
        out["ref_vs_exact_" + part] = np.array([err[k] for k in seq.NAMES])
        print(f"  {name} [{part}] reference vs long double: " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
    np.savez_compressed(os.path.join(HERE, name), **out)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


def start_of(m):
    return dict(start_mu_vec=m.hn_mu_vec.copy(), start_lambda_mat=m.hn_lambda_mat.copy(), start_alpha=float(m.hn_alpha),
                start_beta=float(m.hn_beta))


def linreg_case(D, kind, seed):
    rng = np.random.default_rng(seed)
    prior = priors(D, rng)[kind]
    x, y, _theta = orc.synth_linreg(D, N + N_FIRST, seed, 2.0, np.float64)
    m = ref_lr.LearnModel(D, **prior)
    if kind == "posterior":
        m.update_posterior(x[:N_FIRST], y[:N_FIRST])
    x, y = x[N_FIRST:], y[N_FIRST:]
    out = dict(D=D, x=x, y=y, **start_of(m))
    traces = ([], [], [])
    for i in range(N):
        m.calc_pred_dist(x[i])
        for t, v in zip(traces, (m.p_ms, m.p_lambdas, m.p_nus)):
            t.append(float(np.ravel(v)[0]))
        m.update_posterior(x[i], y[i])
    finish(f"regression_seq_linreg_d{D}_{kind}.npz", m, out, traces, x, y, D)


def ar_case(p, kind, seed):
    rng = np.random.default_rng(seed)
    prior = priors(p + 1, rng)[kind]
    a = np.full(p, 0.6 / max(p, 1))
    noise = 0.3 + rng.standard_normal(N + N_FIRST + p)
    x = np.zeros(len(noise))
    for t in range(len(x)):                   # a stable AR(p) series with a level
        x[t] = noise[t] + sum(a[k] * x[t - 1 - k] for k in range(p) if t - 1 - k >= 0)
    m = ref_ar.LearnModel(p, **prior)
    if kind == "posterior":
        m.update_posterior(x[:N_FIRST + p])
    x = x[N_FIRST:]                           # N + p values: N windows
    out = dict(p=p, x=x, **start_of(m))
    traces = ([], [], [])
    for t in range(p, N + p):
        m.pred_and_update(x[t - p:t + 1])
        for tr, v in zip(traces, (m.p_m, m.p_lambda, m.p_nu)):
            tr.append(float(v))
    w, y = orc.lag_matrix(x, p, None)
    finish(f"regression_seq_ar_p{p}_{kind}.npz", m, out, traces, w, y, p + 1)


if __name__ == "__main__":
    for i, D in enumerate((1, 3, 17)):
        for j, kind in enumerate(("default", "diffuse", "posterior")):
            linreg_case(D, kind, seed=100 + 10 * i + j)
    for i, p in enumerate((0, 1, 4)):
        for j, kind in enumerate(("default", "diffuse", "posterior")):
            ar_case(p, kind, seed=200 + 10 * i + j)
