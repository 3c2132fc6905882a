"""The recipes of the Student-t mixture log-density tests: parameters (pi, mu, nu, u) and rows x, small enough for the exact
oracle (tests/stmix_oracle.py) and built so that every recipe takes the branch it is named after - the tests assert that.

Every sample has row 0 as an ordinary row (it is the default pivot), rows 1 and 2 exactly at the first and the last mean
(q = 0 there) and row 3 fifty spreads away from the first mean.  With ``f32=True`` the means and the rows are binary32
values, so the same rows can be stored either way and the rows at a mean stay exactly there.
"""
import numpy as np


def factors(rng, K, D, cond, spread):
    """Lower triangular U_k with U_k^T U_k of condition about ``cond`` and scale 1 / spread^2."""
    s = np.logspace(0.0, 0.5 * np.log10(cond), D) if D > 1 else np.ones(1)
    u = np.zeros((K, D, D))
    for k in range(K):
        low = np.tril(rng.standard_normal((D, D)), -1) * (0.3 / np.sqrt(D))
        u[k] = (rng.permutation(s)[:, None] * (np.eye(D) + low)) / spread
    return u


def make(K, D, N, seed=0, *, cond=10.0, centre=0.0, spread=1.0, sep=4.0, nu=None, pi=None, f32=False, far_rows=0.0, special=True):
    """dict(pi, mu, nu, u, x): N >= 1 rows drawn around the K means; ``far_rows`` > 0 puts every row that many spreads (times
    sqrt(D)) away from its mean; ``special=False`` leaves rows 1 to 3 ordinary rows."""
    rng = np.random.default_rng([seed, K, D])
    mu = centre + spread * sep * rng.standard_normal((K, D))
    if f32:
        mu = mu.astype(np.float32).astype(np.float64)
    u = factors(rng, K, D, cond, spread)
    nu = np.asarray(rng.uniform(1.0, 9.0, K) if nu is None else np.broadcast_to(nu, (K,)), dtype=np.float64).copy()
    if pi is None:
        pi = rng.uniform(0.5, 1.5, K)
        pi = pi / pi.sum()
    pi = np.asarray(pi, dtype=np.float64)
    which = rng.integers(0, K, N)
    x = mu[which] + spread * rng.standard_normal((N, D))
    if far_rows:
        step = rng.standard_normal((N, D))
        x = mu[which] + far_rows * spread * step / np.linalg.norm(step, axis=1, keepdims=True) * np.sqrt(D)
    if special and N > 1:
        x[1] = mu[0]
    if special and N > 2:
        x[2] = mu[K - 1]
    if special and N > 3:
        step = rng.standard_normal(D)
        x[3] = mu[0] + 50.0 * spread * step / np.linalg.norm(step)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    return dict(pi=pi, mu=mu, nu=nu, u=u, x=x)


def duplicate_component(case, src, dst):
    """Component ``dst`` made a bit-for-bit copy of component ``src`` (weights included): the arg-max must name the lower."""
    for key in ("pi", "mu", "nu", "u"):
        case[key][dst] = case[key][src]
    return case


# name -> recipe; N is small: the exact oracle costs K N D^2 integer products
RECIPES = {
    "k3_d2": lambda: make(3, 2, 40, 1),
    "k5_d17_cond1e4": lambda: make(5, 17, 24, 2, cond=1e4),
    "k8_d33_cond1e4": lambda: make(8, 33, 24, 3, cond=1e4),
    "far_means": lambda: make(4, 16, 24, 4, centre=1e6, spread=1e-2),
    "k4_d64": lambda: make(4, 64, 12, 5),
    "k2_d128": lambda: make(2, 128, 8, 6),
    "nu_across_lgamma_threshold": lambda: make(4, 16, 16, 7, nu=np.array([1.0, 127.0, 128.0, 1e8])),
    "tiny_weights": lambda: make(4, 3, 16, 8, pi=np.array([1.0 - 1e-3, 1e-300, 1e-150, 1e-3])),
    "outliers": lambda: make(3, 4, 16, 9, nu=np.array([1.0, 1.0, 2.0]), far_rows=3e6),
    "all_far_below": lambda: make(3, 8, 16, 10, nu=1e8, far_rows=400.0, special=False),
    "cond1e6": lambda: make(3, 24, 16, 11, cond=1e6),
}
