#!/usr/bin/env python3
"""Golden fixtures for ``pred_and_update_sequence`` of multivariate_normal, produced by the REFERENCE's own loop (build
container only; the path of a bayesml v0.3.1 checkout is the argument):

    MPLBACKEND=Agg python tests/golden/make_golden_mvn_seq.py <path to the reference>

Per row ``calc_pred_dist``, the read-outs, then ``update_posterior`` of that row.  Cases: D in {1, 3, 17}, n = 150 rows, each
from the default prior, from a diffuse prior (h0_w_mat = 1e6 I) and from the posterior a first ``update_posterior`` of 40
rows leaves on a given prior.  The state at the first row is stored (``start_*``), so every implementation starts from the
same bits.  Stored per case: the inputs, the reference's traces (p_m_vec, p_nu, slogdet(p_v_mat), the quadratic form and
-multivariate_t.logpdf), the final ``hn_*``, the traces of the same loop in long double (tests/mvn_seq_oracle.py:
ld_row_loop), and ``ref_vs_exact``: the reference's error against them per output (oracle ``errors``), separately for the
first 2 D rows and for the rest.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import multivariate_normal as ref_mvn      # noqa: E402
import mvn_seq_oracle as seq                            # noqa: E402

N = 150
N_FIRST = 40


def priors(D, rng):
    a = rng.standard_normal((D, D))
    return {"default": {}, "diffuse": dict(h0_w_mat=np.eye(D) * 1e6),
            "posterior": dict(h0_m_vec=rng.standard_normal(D) * 0.3, h0_kappa=2.5, h0_nu=D + 1.5,
                              h0_w_mat=np.linalg.inv(np.eye(D) * 2.0 + a @ a.T / D))}


def case(D, kind, seed):
    from scipy.stats import multivariate_t
    rng = np.random.default_rng(seed)
    prior = priors(D, rng)[kind]
    mix = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    x = 0.7 + rng.standard_normal((N + N_FIRST, D)) @ mix.T
    m = ref_mvn.LearnModel(D, **prior)
    if kind == "posterior":
        m.update_posterior(x[:N_FIRST])
    x = x[N_FIRST:]
    out = dict(D=D, x=x, start_m_vec=m.hn_m_vec.copy(), start_kappa=float(m.hn_kappa), start_nu=float(m.hn_nu),
               start_w_mat_inv=m.hn_w_mat_inv.copy())
    start = (out["start_m_vec"], out["start_kappa"], out["start_nu"], out["start_w_mat_inv"])
    means, p_nus, logdets, quads, nats = np.zeros((N, D)), np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    for i in range(N):
        m.calc_pred_dist()
        means[i], p_nus[i] = m.p_m_vec, m.p_nu
        logdets[i] = np.linalg.slogdet(m.p_v_mat)[1]
        diff = x[i] - m.p_m_vec
        quads[i] = diff @ m.p_v_mat @ diff
        nats[i] = -multivariate_t.logpdf(x[i], loc=m.p_m_vec, shape=m.p_v_mat_inv, df=m.p_nu)
        m.update_posterior(x[i:i + 1])
    ref = (means, logdets, quads, nats)
    exact = seq.pick(seq.ld_row_loop(x, *start))
    out.update(hn_m_vec=m.hn_m_vec.copy(), hn_kappa=float(m.hn_kappa), hn_nu=float(m.hn_nu),
               hn_w_mat_inv=m.hn_w_mat_inv.copy(), ref_p_nu=p_nus)
    name = f"mvn_seq_d{D}_{kind}.npz"
    for k, r, e in zip(seq.NAMES, ref, exact):
        out["ref_" + k] = r
        out["exact_" + k] = np.asarray(e, dtype=np.longdouble)
    for part, rows in (("head", slice(0, 2 * D)), ("rest", slice(2 * D, None))):
        err = seq.errors(ref, exact, x, rows)
        out["ref_vs_exact_" + part] = np.array([err[k] for k in seq.NAMES])
        print(f"  {name} [{part}] reference vs long double: " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
    np.savez_compressed(os.path.join(HERE, name), **out)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    for i, D in enumerate((1, 3, 17)):
        for j, kind in enumerate(("default", "diffuse", "posterior")):
            case(D, kind, seed=300 + 10 * i + j)
