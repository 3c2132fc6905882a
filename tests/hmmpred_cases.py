"""The recipes of the HMM sequence-predictive tests: parameters (a, w0, mu, nu, u) and a sequence x drawn from the chain, small
enough for the exact oracle (tests/hmmpred_oracle.py).  The emission parameters are stmix_cases' (same factors, same means),
the rows follow a state path of the chain instead of independent draws.

ORDINARY cases must keep the bound below 1e-9 (1 + |ln p_t|) at every step (tests/test_hmmpred.py asserts it); HARD names
the only exemptions.  STICKY are the two chains on which forgetting fails: three states with a_ii = 1 - 1e-3 and emission
means 0.5 sigma apart, run at chunk_len = 32, sweep_len = 8.
"""
import numpy as np

import stmix_cases as sc


def transition(rng, K, stay=0.6, band=None):
    """Row-stochastic [K, K]: ``stay`` on the diagonal, the rest spread at random - over all states, or with ``band`` over the
    next ``band`` states only (zeros elsewhere: the oracle skips them, which keeps K = 256 affordable)."""
    if K == 1:
        return np.ones((1, 1))
    a = np.zeros((K, K))
    for i in range(K):
        others = [(i + d) % K for d in range(1, (band or K - 1) + 1)]
        w = rng.uniform(0.5, 1.5, len(others))
        a[i, others] = (1.0 - stay) * w / w.sum()
        a[i, i] = 1.0 - a[i, others].sum()
    return a


def path(rng, a, w0, T):
    z = np.empty(T, dtype=np.int64)
    z[0] = rng.choice(len(w0), p=w0)
    for t in range(1, T):
        z[t] = rng.choice(len(w0), p=a[z[t - 1]])
    return z


def make(K, D, T, seed=0, *, stay=0.6, band=None, cond=10.0, centre=0.0, spread=1.0, sep=4.0, nu=None, f32=False, w0=None):
    """dict(a, w0, mu, nu, u, x, z): T >= 1 rows along a state path of the chain."""
    rng = np.random.default_rng([seed, K, D, 7])
    mu = centre + spread * sep * rng.standard_normal((K, D))
    if f32:
        mu = mu.astype(np.float32).astype(np.float64)
    u = sc.factors(rng, K, D, cond, spread)
    nu = np.asarray(rng.uniform(1.0, 9.0, K) if nu is None else np.broadcast_to(nu, (K,)), dtype=np.float64).copy()
    a = transition(rng, K, stay, band)
    if w0 is None:
        w0 = rng.uniform(0.5, 1.5, K)
        w0 = w0 / w0.sum()
    w0 = np.asarray(w0, dtype=np.float64)
    z = path(rng, a, w0, T)
    x = mu[z] + spread * rng.standard_normal((T, D))
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    return dict(a=a, w0=w0, mu=mu, nu=nu, u=u, x=x, z=z)


def sticky(T=200, flat=None, seed=11):
    """Three states that stay with 1 - 1e-3, unit-variance emissions in one dimension with means 0.5 apart.  ``flat`` = (lo, hi):
    the rows lo .. hi - 1 lie 1e4 sigma away, where the Student-t kernels (nu = 3) of the three states agree to 1e-4 - an
    uninformative stretch."""
    rng = np.random.default_rng(seed)
    a = np.full((3, 3), 0.5e-3)
    np.fill_diagonal(a, 1.0 - 1e-3)
    mu = np.array([[-0.5], [0.0], [0.5]])
    w0 = np.full(3, 1.0 / 3.0)
    z = path(rng, a, w0, T)
    z[T // 2:] = (z[T // 2 - 1] + 1) % 3                       # (one switch, so that the filter has something to find)
    x = mu[z] + rng.standard_normal((T, 1))
    if flat is not None:
        x[flat[0]:flat[1]] = 1e4
    return dict(a=a, w0=w0, mu=mu, nu=np.full(3, 3.0), u=np.ones((3, 1, 1)), x=x, z=z)


def duplicate_state(case, src, dst):
    """State ``dst`` made a bit-for-bit copy of state ``src`` - emission, transitions out of it and into it, start weight: the
    filtered posteriors of the two are equal bit for bit, and the arg-max must name the lower."""
    for key in ("mu", "nu", "u"):
        case[key][dst] = case[key][src]
    a = case["a"]
    a[dst] = a[src]
    both = 0.5 * (a[:, src] + a[:, dst])
    a[:, src] = both
    a[:, dst] = both
    case["w0"][dst] = case["w0"][src] = 0.5 * (case["w0"][src] + case["w0"][dst])
    return case


CHUNK = dict(chunk_len=32, sweep_len=8)

# name -> recipe; the exact oracle costs K T D^2 integer products and K^2 T mpmath products
ORDINARY = {
    "k3_d2": lambda: make(3, 2, 100, 1),
    "k1_d3": lambda: make(1, 3, 40, 2),
    "k5_d17_cond1e4": lambda: make(5, 17, 70, 3, cond=1e4),
    "k8_d33_cond1e4": lambda: make(8, 33, 40, 4, cond=1e4),
    "k4_d64": lambda: make(4, 64, 24, 5),
    "k2_d128": lambda: make(2, 128, 12, 6),
    "k17_d3": lambda: make(17, 3, 80, 7),
    "k3_d130_plain": lambda: make(3, 130, 10, 8),
    "zero_start_entries": lambda: make(4, 3, 70, 9, w0=np.array([0.0, 0.75, 0.0, 0.25])),
}
HARD = {
    "far_means": lambda: make(4, 16, 70, 10, centre=1e6, spread=1e-2),
    "nu_1_and_1e8": lambda: make(4, 16, 70, 11, nu=np.array([1.0, 1.0, 1e8, 1e8])),
    "badly_scaled": lambda: make(3, 24, 70, 12, cond=1e6),
}
STICKY = {
    "sticky": lambda: sticky(200),
    "sticky_flat_stretch": lambda: sticky(200, flat=(60, 70)),      # across the boundary behind step 64
}
RECIPES = {**ORDINARY, **HARD, **STICKY}
